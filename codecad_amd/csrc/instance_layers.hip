// codecad_amd/csrc/instance_layers.hip
//
// The LAYERED OUTLINES of an assembly (codecad_amd/layer_outlines.py): the outlines of instance_outline.hip on a stack of
// parallel planes, every layer in ONE traversal.  The layers share the instance table, the frame (u, v), the step, the
// lattice of squares and the windows; they differ in the 3D position of the section's sample (0, 0) alone, and a tile's row
// says which layer it belongs to in its second word: {a0 | b0 << 16, layer, mask lo, mask hi}.  The corners are a table of
// n_layers float4 {x, y, z, unused} in global memory; one wavefront takes one tile, so the layer is wave-uniform and the
// corner arrives through constant_uniform by one scalar load, like the windows and the programs.  A row whose layer is not
// below n_layers is treated as absent: nothing is read past the table.  Children inherit their parent's layer word, and a
// segment is a 16-byte record {a | b << 16, k | e_from << 8 | e_to << 10 | layer << 12, t_from, t_to}.
//
// Everything else -- the shifted indices, the squares and their edges, strict insideness, the crossing t, the direction
// of a segment, the saddles, the keep rule of k_layer_tiles and the two passes, the 81 values in the wavefront's own 128
// floats of LDS and the ballot-prefix placement of k_layer_leaf -- is that of k_outline_tiles and k_outline_leaf, whose
// file's head defines it.  THE BODIES ARE DUPLICATES of instance_outline.hip's, kept apart on purpose: that unit's
// register counts are recorded (tests/test_section_outlines_host.py) and it stays byte for byte as
// it is; a change to either body belongs in both.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the end of
// this file.
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

struct Point {
    float x, y, z;
};
// the point of the layer's plane at the SHIFTED lattice indices (fs, ft): the section's formula from the layer's corner at
// the sample indices fs - 1, ft - 1 (whole and half-integer shifted indices below 2^17: the subtraction is exact)
__device__ __forceinline__ Point plane_point(const LayerArgs& t, const float4& corner, float fs, float ft)
{
    const float a = t.c.step * (fs - 1.0f), b = t.c.step * (ft - 1.0f);
    return Point{(corner.x + t.u[0] * a) + t.v[0] * b, (corner.y + t.u[1] * a) + t.v[1] * b, (corner.z + t.u[2] * a) + t.v[2] * b};
}

// the corner of a row's layer (wave-uniform, below n_layers), by scalar load
__device__ __forceinline__ float4 layer_corner(const LayerArgs& t, uint32_t layer)
{
    return constant_uniform(t.layer_corners)[layer];
}

template <bool DO>
__global__ void __launch_bounds__(256) k_layer_tiles(const LayerArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const bool have = row.have & (row.z0 < t.n_layers);           // wave-uniform; a row of no layer is no row
    const uint32_t layer = have ? row.z0 : 0u;                    // (n_layers >= 1: entry 0 exists)
    const uint64_t mask = have ? row.mask : 0ull;
    const float4 corner = layer_corner(t, layer);
    const uint32_t s = a.child_side;
    const uint32_t x = row.x0 + (lane >> 3) * s, y = row.y0 + (lane & 7u) * s;
    const bool live = have & (x < a.dims[0]) & (y < a.dims[1]);
    const float h = 0.5f * (float)s;
    const Point p = plane_point(t, corner, (float)x + h, (float)y + h);
    const uint32_t* windows = constant_uniform(a.windows);
    uint64_t keep = 0ull;
    for (uint64_t m = mask; m != 0ull; m &= m - 1ull) {           // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool reach = (x <= win[3]) & (x + s - 1u >= win[0]) & (y <= win[4]) & (y + s - 1u >= win[1]);
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        if (reach && !(w >= a.thr) && !(w <= -a.thr)) keep |= 1ull << n;   // may cross an edge of the child (a NaN keeps its candidate)
    }
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(mask)));
    const bool flag[1] = {live && keep != 0ull};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity) a.children[slot[0]] = make_uint4(x | (y << 16), layer, (uint32_t)keep, (uint32_t)(keep >> 32));
}

// The segments of a square by its case, bit c set when corner c is inside: corner 0 at (a, b), 1 at (a + 1, b), 2 at
// (a, b + 1), 3 at (a + 1, b + 1).  A segment is e_from << 2 | e_to, four bits per case.  One inside corner is walked
// round counter-clockwise, one outside corner clockwise; two on a side give the segment across, the inside on its left.
// The saddles 6 (corners 1, 2) and 9 (corners 0, 3) have a second segment: each cuts off one inside corner.
constexpr uint32_t seg(uint32_t from, uint32_t to) { return from << 2 | to; }
constexpr uint64_t kFirst =
    (uint64_t)seg(0, 3) << 4 | (uint64_t)seg(1, 0) << 8 | (uint64_t)seg(1, 3) << 12 | (uint64_t)seg(3, 2) << 16 | (uint64_t)seg(0, 2) << 20 |
    (uint64_t)seg(1, 0) << 24 | (uint64_t)seg(1, 2) << 28 | (uint64_t)seg(2, 1) << 32 | (uint64_t)seg(0, 3) << 36 | (uint64_t)seg(2, 0) << 40 |
    (uint64_t)seg(2, 3) << 44 | (uint64_t)seg(3, 1) << 48 | (uint64_t)seg(0, 1) << 52 | (uint64_t)seg(3, 0) << 56;
constexpr uint32_t kSecond6 = seg(3, 2), kSecond9 = seg(2, 1);

// the crossing of an edge from the sample with wp to the sample with wq
__device__ __forceinline__ float crossing(float wp, float wq)
{
    const float t = wp / (wp - wq);
    return t != t ? 0.5f : t;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_layer_leaf(const LayerArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    const CellRow row = cell_row(a);
    if (!row.have || row.z0 >= t.n_layers) return;                // wave-uniform; this kernel has no barrier
    const uint32_t layer = row.z0;
    const float4 corner = layer_corner(t, layer);
    const uint32_t lane = threadIdx.x & 63u;
    // the wavefront's 81 values, [9 j + i] of the sample (a0 + i, b0 + j), in its 128 floats after the register file
    float* wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 128u;
    const uint32_t i = lane & 7u, j = lane >> 3;
    const uint32_t x = row.x0 + i, y = row.y0 + j;
    const bool live = (x < a.dims[0]) & (y < a.dims[1]);          // the lane's square exists: so do its four samples
    // the second pass: lanes 0..8 take the column i = 8, lanes 9..16 the row j = 8; the others repeat their own sample
    const bool rim = lane < 17u;
    const uint32_t ri = lane < 9u ? 8u : lane - 9u, rj = lane < 9u ? lane : 8u;
    const uint64_t below = (1ull << lane) - 1ull;
    unsigned long long* totals = static_cast<unsigned long long*>(a.pairs);
    // samples exist up to the shifted index dims (one more than squares)
    const uint64_t first_lives = __ballot((x <= a.dims[0]) & (y <= a.dims[1]));
    const uint64_t rim_lives = __ballot(rim & (row.x0 + ri <= a.dims[0]) & (row.y0 + rj <= a.dims[1]));
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {       // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
#pragma unroll 1
        for (uint32_t pass = 0u; pass < 2u; ++pass) {             // the one interpreter call site, used twice
            const bool second = (pass != 0u) & rim;
            const uint32_t si = second ? ri : i, sj = second ? rj : j;
            const Point p = plane_point(t, corner, (float)(row.x0 + si), (float)(row.y0 + sj));
            const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
            if ((pass == 0u) | rim) wl[9u * sj + si] = w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float w0 = wl[9u * j + i], w1 = wl[9u * j + i + 1u], w2 = wl[9u * j + i + 9u], w3 = wl[9u * j + i + 10u];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // (the next candidate's values overwrite these)
        __builtin_amdgcn_wave_barrier();
        const uint32_t c = (w0 < 0.0f ? 1u : 0u) | (w1 < 0.0f ? 2u : 0u) | (w2 < 0.0f ? 4u : 0u) | (w3 < 0.0f ? 8u : 0u);
        const bool one = live & (c != 0u) & (c != 15u), two = live & ((c == 6u) | (c == 9u));
        const uint64_t b1 = __ballot(one), b2 = __ballot(two);
        const uint32_t total = (uint32_t)(__popcll(b1) + __popcll(b2));
        if (total == 0u) continue;                                // wave-uniform
        unsigned long long base = 0ull;
        if (lane == 0u) {
            base = atomicAdd(&totals[0], (unsigned long long)total);
            atomicAdd(&totals[1u + n], (unsigned long long)total);
        }
        base = ((unsigned long long)uniform((uint32_t)(base >> 32)) << 32) | uniform((uint32_t)base);
        const unsigned long long slot = base + (unsigned long long)(__popcll(b1 & below) + __popcll(b2 & below));
        // the four edges' crossings (those of edges not crossed are not used)
        const float t0 = crossing(w0, w1), t1 = crossing(w1, w3), t2 = crossing(w2, w3), t3 = crossing(w0, w2);
        const uint32_t where = x | (y << 16), whose = n | (layer << 12);
        for (uint32_t r = 0u; r < 2u; ++r) {
            const uint32_t code = r == 0u ? (uint32_t)(kFirst >> (4u * c)) & 15u : (c == 6u ? kSecond6 : kSecond9);
            const uint32_t from = code >> 2, to = code & 3u;
            const float tf = from == 0u ? t0 : from == 1u ? t1 : from == 2u ? t2 : t3;
            const float tt = to == 0u ? t0 : to == 1u ? t1 : to == 2u ? t2 : t3;
            if ((r == 0u ? one : two) && slot + r < t.segment_capacity)
                t.segments[slot + r] = make_uint4(where, whose | (from << 8) | (to << 10), __float_as_uint(tf), __float_as_uint(tt));
        }
    }
    if (lane == 0u) atomicAdd(a.evaluations, (unsigned long long)((__popcll(first_lives) + __popcll(rim_lives)) * __popcll(row.mask)));
}

// [leaf][distance_only]
void (*const kLayerTable[2][2])(LayerArgs) = {
    {k_layer_tiles<false>, k_layer_tiles<true>},
    {k_layer_leaf<false>, k_layer_leaf<true>},
};

constexpr uint32_t kMaxLayers = 1u << 20;     // (a record keeps the layer in the 20 bits from bit 12)

// What both entry points of the layered outlines check and fill: cells_args() of a lattice of squares {dims a, dims b, 1}
// with windows, the planes' frame and the table of the layers' corners.  `corner` is checked and otherwise unused.
int layer_args(const void* table_dev, uint32_t n, const uint32_t* windows_dev, const void* parents_dev, const uint32_t* n_parents_dev,
               uint32_t max_parents, const uint32_t dims[2], const float corner[3], const float u[3], const float v[3],
               const float* layer_corners_dev, uint32_t n_layers, float step, uint64_t* evaluations_dev, LayerArgs& t)
{
    if (!dims || !u || !v || !layer_corners_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (n_layers == 0u || n_layers > kMaxLayers) return hu_fail(HU_ERR_BAD_ARG, "1..2^20 layers");
    const uint32_t dims3[3] = {dims[0], dims[1], 1u};
    std::memset(&t, 0, sizeof(t));
    int rc;
    if ((rc = cells_args(true, table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims3, corner, step, evaluations_dev, t.c)))
        return rc;
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(u[i]) || !std::isfinite(v[i]) || !std::isfinite(corner[i])) return hu_fail(HU_ERR_BAD_ARG, "the plane's frame must be finite");
        t.u[i] = u[i];
        t.v[i] = v[i];
    }
    t.layer_corners = reinterpret_cast<const float4*>(layer_corners_dev);
    t.n_layers = n_layers;
    return HU_OK;
}

}  // namespace

hipError_t hu_cells::allow_big_lds_layers(size_t bytes)
{
    hipError_t e = hipSuccess;
    for (const auto& level : kLayerTable)
        for (const auto variant : level)
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)variant, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

extern "C" {

int hu_layer_tiles(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                   const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, uint32_t child_side,
                   const uint32_t dims[2], const float corner[3], const float u[3], const float v[3], const float* layer_corners_dev,
                   uint32_t n_layers, float step, float radius, uint32_t* counter_dev, void* children_dev, uint32_t capacity,
                   uint64_t* evaluations_dev, void* stream)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, layer_corners_dev, n_layers,
                         step, evaluations_dev, t)))
        return rc;
    if ((rc = cells_children(t.c, child_side, radius, counter_dev, children_dev, capacity))) return rc;
    if (child_side < 8u || child_side > 8192u || (child_side & (child_side - 1u)))
        return hu_fail(HU_ERR_BAD_ARG, "child_side must be a power of two in 8..8192");
    if (std::isnan(radius) || radius < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    return cells_launch(kLayerTable[0][distance_only_kernel != 0], t, t.c, lane_bytes, 0u, stream);
}

int hu_layer_leaf(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                  const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, const uint32_t dims[2],
                  const float corner[3], const float u[3], const float v[3], const float* layer_corners_dev, uint32_t n_layers,
                  float step, void* segments_dev, uint32_t segment_capacity, uint64_t* totals_dev, uint64_t* evaluations_dev,
                  void* stream)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, layer_corners_dev, n_layers,
                         step, evaluations_dev, t)))
        return rc;
    if (!totals_dev || (!segments_dev && segment_capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = totals_dev;
    t.segments = static_cast<uint4*>(segments_dev);
    t.segment_capacity = segment_capacity;
    // the 81 values of a tile: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kLayerTable[1][distance_only_kernel != 0], t, t.c, lane_bytes, 8u, stream);
}

}  // extern "C"
