// codecad_amd/csrc/instance_mesh.hip
//
// The SURFACE MESHES of an assembly's parts (codecad_amd/assembly_meshes.py): per instance k, the marching-cubes surface of
// w_k on the lattice of interference() with a ring of samples around it.  Samples carry the SHIFTED index s = index + 1,
// 0 .. n + 1 per axis, and sit at corner + step * ((float)s - 1.0f) per axis: kernels.hpp sample() for s >= 1, the same
// formula at -1 for s = 0.  CUBE (a, b, c), 0 <= a <= nx and likewise b, c, has its corner m at the shifted index
// (a, b, c) + CORNERS[m] and its edges EDGES[e] in the numbering of tools/gen_mc_table.py (mc_table.hpp).  Inside is w < 0,
// strictly; bit m of the case is set when corner m is inside; the triangles of a cube are kMcTriangles[case], in the table's
// order and winding.  An edge with exactly one end inside is crossed at t = w_p / (w_p - w_q), p the end with the LOWER
// lattice index along the edge's axis: one binary32 subtraction and one correctly rounded binary32 division (this unit is
// built with -fhip-fp32-correctly-rounded-divide-sqrt like every other: the plain `/`), 0.5 where that is no number.  A
// triangle is a 32-byte record, two uint4: {a | b << 16, c | k << 16 | which << 24, case | e0 << 8 | e1 << 16 | e2 << 24, 0}
// {t0, t1, t2, 0}, `which` its number within the case.  Nothing is filtered or merged here: degenerate triangles are kept.
//
// Args describes the lattice of CUBES: dims = samples + 1 per axis, a row is a cell {a0 | b0 << 16, c0, mask lo, mask hi} of
// 4^k cubes a side, windows (n x 6) the cubes an instance may cross.  One WAVEFRONT takes one cell, lane = 16 x + 4 y + z.
//   k_mesh_cells (child side S >= 4): a lane is the child at (a0 + x S, b0 + y S, c0 + z S).  Every candidate is evaluated at
//     the child's centre, the shifted index a + S / 2 per axis.  The child's corner samples lie within S * step * sqrt(3) / 2
//     of it; r = a.thr is (S + 1) * step * sqrt(3) / 2 times (1 + 2^-10).  w >= r: outside at every corner sample; w <= -r:
//     inside at every one -- no crossing either way.  A child keeps k when its window reaches the child and neither holds;
//     a value that is no number keeps its candidate.
//   k_mesh_leaf (4^3 cubes, 5^3 samples): per candidate, the 64 samples at the lanes' own corners, then the 61 of the cell's
//     three far faces on lanes 0..60, through the ONE interpreter call site; the 125 values go to the wavefront's own 128
//     floats of LDS after the register file, [25 i + 5 j + k] of the sample (a0 + i, b0 + j, c0 + k).  Each lane reads its
//     cube's eight, forms the case and takes its row of the case table: 0-5 triangles.  The slot prefix comes from three
//     ballots of the count's bits; one atomic on the triangle counter and one on the instance's count per wavefront and
//     candidate.  A triangle's crossings are computed from the two ends of each of its edges, read from LDS again by the
//     edge's number: no array of twelve.  Records at or past the capacity are counted and not stored.
// The case table is a __constant__ array of 256 uint64 (five triangles of three 4-bit edges, the count in the top four
// bits): one 8-byte load per lane and candidate, and no fill, barrier or LDS of its own in a kernel whose wavefronts return
// early and share nothing.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the end of
// this file.
#include "instance_cells.hpp"
#include "mc_table.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// the coordinate of the sample with the SHIFTED index fs along an axis (whole numbers below 2^17: the subtraction is exact)
__device__ __forceinline__ float ring_sample(float corner, float step, float fs) { return corner + step * (fs - 1.0f); }

template <bool DO>
__global__ void __launch_bounds__(256) k_mesh_cells(const MeshArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    const ChildLane q = child_lane(a, row, lane);
    const uint32_t x = q.x, y = q.y, z = q.z;
    const bool live = q.live;
    const float h = 0.5f * (float)s;
    const float px = ring_sample(a.corner[0], a.step, (float)x + h);
    const float py = ring_sample(a.corner[1], a.step, (float)y + h);
    const float pz = ring_sample(a.corner[2], a.step, (float)z + h);
    const uint32_t* windows = constant_uniform(a.windows);
    uint64_t keep = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool reach = reaches(win, q, s);
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        if (reach && !(w >= a.thr) && !(w <= -a.thr)) keep |= 1ull << n;   // may cross an edge of the child (a NaN keeps its candidate)
    }
    // (the count and the child-row store stay spelled out: through a shared function this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && keep != 0ull};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity) a.children[slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
}

// The case table, a row per case: triangle r is the twelve bits from 12 r, its three edges four bits each in the table's
// order; the top four bits are the number of triangles (at most five).
struct MeshCases {
    unsigned long long row[256];
};
constexpr MeshCases make_mesh_cases()
{
    constexpr signed char tri[256][MC_TABLE_WIDTH] = MC_TRIANGLES_INIT;
    MeshCases p{};
    for (int c = 0; c < 256; ++c) {
        unsigned long long v = 0ull;
        int k = 0;
        for (; k < 15 && tri[c][k] >= 0; ++k) v |= (unsigned long long)tri[c][k] << (4 * k);
        p.row[c] = v | (unsigned long long)(k / 3) << 60;
    }
    return p;
}
static_assert(MC_TABLE_WIDTH == 16, "a case has at most five triangles: sixty bits of edges");
__device__ __constant__ MeshCases kMeshCases = make_mesh_cases();

// Where the ends of edge e are among a wavefront's 125 values, relative to the cube's corner 0: the end with the lower
// lattice index at kEdgeLower (five bits per edge: 25 dx + 5 dy + dz of CORNERS), the other one stride further along the
// edge's axis (25, 5 or 1).  EDGES lists 2, 3, 6 and 7 from their higher end: here every edge starts at its lower one.
constexpr unsigned long long edge_words(bool stride)
{
    constexpr unsigned char lower[12] = {0, 25, 5, 0, 1, 26, 6, 1, 0, 25, 30, 5};
    constexpr unsigned char along[12] = {25, 5, 25, 5, 25, 5, 25, 5, 1, 1, 1, 1};
    unsigned long long v = 0ull;
    for (int e = 0; e < 12; ++e) v |= (unsigned long long)(stride ? along[e] : lower[e]) << (5 * e);
    return v;
}
constexpr unsigned long long kEdgeLower = edge_words(false), kEdgeStride = edge_words(true);

// the crossing of edge e of the cube whose corner 0 is wl[base]
__device__ __forceinline__ float crossing(const float* wl, uint32_t base, uint32_t e)
{
    const uint32_t p = base + ((uint32_t)(kEdgeLower >> (5u * e)) & 31u), q = p + ((uint32_t)(kEdgeStride >> (5u * e)) & 31u);
    const float wp = wl[p], wq = wl[q];
    const float t = wp / (wp - wq);
    return t != t ? 0.5f : t;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_mesh_leaf(const MeshArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const uint32_t lane = threadIdx.x & 63u;
    // the wavefront's 125 values, [25 i + 5 j + k] of the sample (a0 + i, b0 + j, c0 + k), in its 128 floats after the register file
    float* wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 128u;
    const uint32_t i = lane >> 4, j = (lane >> 2) & 3u, k = lane & 3u;
    const LeafLane l = leaf_lane(a, row);
    const uint32_t x = l.x, y = l.y, z = l.z;
    const bool live = l.live;                                     // the lane's cube exists: so do its eight samples
    // the second pass: lanes 0..24 take the face i = 4, lanes 25..44 the rest of j = 4, lanes 45..60 the rest of k = 4; the
    // others repeat their own sample
    const bool far = lane < 61u;
    const uint32_t l1 = lane - 25u, l2 = lane - 45u;
    const uint32_t ri = lane < 25u ? 4u : lane < 45u ? l1 / 5u : (l2 >> 2) & 3u;
    const uint32_t rj = lane < 25u ? lane / 5u : lane < 45u ? 4u : l2 & 3u;
    const uint32_t rk = lane < 25u ? lane % 5u : lane < 45u ? l1 % 5u : 4u;
    const uint32_t base = 25u * i + 5u * j + k;
    const uint64_t below = (1ull << lane) - 1ull;
    unsigned long long* totals = static_cast<unsigned long long*>(a.pairs);
    // samples exist up to the shifted index dims (one more than cubes)
    const uint64_t first_lives = __ballot((x <= a.dims[0]) & (y <= a.dims[1]) & (z <= a.dims[2]));
    const uint64_t far_lives = __ballot(far & (row.x0 + ri <= a.dims[0]) & (row.y0 + rj <= a.dims[1]) & (row.z0 + rk <= a.dims[2]));
    const uint32_t where = x | (y << 16);
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {       // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
#pragma unroll 1
        for (uint32_t pass = 0u; pass < 2u; ++pass) {             // the one interpreter call site, used twice
            const bool second = (pass != 0u) & far;
            const uint32_t si = second ? ri : i, sj = second ? rj : j, sk = second ? rk : k;
            const float px = ring_sample(a.corner[0], a.step, (float)(row.x0 + si));
            const float py = ring_sample(a.corner[1], a.step, (float)(row.y0 + sj));
            const float pz = ring_sample(a.corner[2], a.step, (float)(row.z0 + sk));
            const float w = instance_dist<DO>(a, n, px, py, pz, lds);
            if ((pass == 0u) | far) wl[25u * si + 5u * sj + sk] = w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // corner m of the cube at base + 25 dx + 5 dy + dz of CORNERS[m]
        const uint32_t c = (wl[base] < 0.0f ? 1u : 0u) | (wl[base + 25u] < 0.0f ? 2u : 0u) | (wl[base + 30u] < 0.0f ? 4u : 0u) |
                           (wl[base + 5u] < 0.0f ? 8u : 0u) | (wl[base + 1u] < 0.0f ? 16u : 0u) | (wl[base + 26u] < 0.0f ? 32u : 0u) |
                           (wl[base + 31u] < 0.0f ? 64u : 0u) | (wl[base + 6u] < 0.0f ? 128u : 0u);
        const unsigned long long tri = kMeshCases.row[live ? c : 0u];
        const uint32_t count = (uint32_t)(tri >> 60);             // 0..5; none where the cube does not exist
        const uint64_t b0 = __ballot((count & 1u) != 0u), b1 = __ballot((count & 2u) != 0u), b2 = __ballot((count & 4u) != 0u);
        const uint32_t total = (uint32_t)(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
        if (total != 0u) {                                        // wave-uniform
            unsigned long long first = 0ull;
            if (lane == 0u) {
                first = atomicAdd(&totals[0], (unsigned long long)total);
                atomicAdd(&totals[1u + n], (unsigned long long)total);
            }
            first = ((unsigned long long)uniform((uint32_t)(first >> 32)) << 32) | uniform((uint32_t)first);
            const unsigned long long slot = first + (unsigned long long)(__popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below));
#pragma unroll 1
            for (uint32_t r = 0u; r < 5u; ++r) {
                const bool mine = r < count;
                if (__ballot(mine) == 0ull) break;                // wave-uniform
                const uint32_t edges = (uint32_t)(tri >> (12u * r)) & 0xfffu;
                const uint32_t e0 = edges & 15u, e1 = (edges >> 4) & 15u, e2 = edges >> 8;
                // (lanes without a triangle r read edge 0 of their own cube: inside the 125 values)
                const float t0 = crossing(wl, base, e0), t1 = crossing(wl, base, e1), t2 = crossing(wl, base, e2);
                if (mine && slot + r < t.triangle_capacity) {
                    uint4* record = t.triangles + 2ull * (slot + r);
                    record[0] = make_uint4(where, z | (n << 16) | (r << 24), c | (e0 << 8) | (e1 << 16) | (e2 << 24), 0u);
                    record[1] = make_uint4(__float_as_uint(t0), __float_as_uint(t1), __float_as_uint(t2), 0u);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // (the next candidate's values overwrite these)
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0u) atomicAdd(a.evaluations, (unsigned long long)((__popcll(first_lives) + __popcll(far_lives)) * __popcll(row.mask)));
}

// [leaf][distance_only]
void (*const kMeshTable[2][2])(MeshArgs) = {
    {k_mesh_cells<false>, k_mesh_cells<true>},
    {k_mesh_leaf<false>, k_mesh_leaf<true>},
};
HU_BIG_LDS(kMeshTable);

}  // namespace

extern "C" {

int hu_mesh_cells(const hu_cells_launch* launch, const hu_cells_children* children)
{
    MeshArgs t;
    std::memset(&t, 0, sizeof(t));
    int rc;
    if ((rc = cells_args(kWindows | kStrict, launch, t.c))) return rc;
    if ((rc = cells_children(t.c, children))) return rc;
    if ((rc = check_child_side(t.c.child_side, 4u, 16384u))) return rc;
    if (std::isnan(t.c.thr) || t.c.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    return cells_launch(kMeshTable[0][launch->distance_only != 0], t, t.c, *launch, 0u);
}

int hu_mesh_leaf_instances(const hu_cells_launch* launch, void* triangles_dev, uint32_t triangle_capacity, uint64_t* totals_dev)
{
    MeshArgs t;
    std::memset(&t, 0, sizeof(t));
    int rc;
    if ((rc = cells_args(kWindows | kStrict, launch, t.c))) return rc;
    if (!totals_dev || (!triangles_dev && triangle_capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = totals_dev;
    t.triangles = static_cast<uint4*>(triangles_dev);
    t.triangle_capacity = triangle_capacity;
    // the 125 values of a cell: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kMeshTable[1][launch->distance_only != 0], t, t.c, *launch, 8u);
}

}  // extern "C"
