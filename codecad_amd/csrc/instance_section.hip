// codecad_amd/csrc/instance_section.hip
//
// The planar SECTION of an assembly (codecad_amd/section.py): a 2D lattice of samples on a plane, and per sample which
// instances it is inside of.  Sample (i, j) sits at
//     p = (corner + u * (step * (float)i)) + v * (step * (float)j)        per coordinate, every operation rounded in binary32
// (plane_point(), the one statement of it; u = (1, 0, 0), v = (0, 1, 0) gives kernels.hpp sample() on both axes).  With
// w_k(p) the distance of instance k alone, as in instance_pairs.hip:
//     inside mask(p) = {k : w_k(p) < 0}, strictly;  part_ids = its lowest index, -1 for none;  inside_count = its size;
//     distance(p) = min_k w_k(p), the hardware minimum chain;  nearest(p) = the LOWEST index that attains it
// (the tie rule of instance_rays.hip), and the samples inside k, and inside both i and j, add to accumulators of the kind
// interference keeps, at pairs[k * n + k] and pairs[i * n + j].
//
// The lattice is cut into square TILES of 8^k x 8^k samples, a 16-byte row {x0 | y0 << 16, unused, mask lo, mask hi} each:
// the cell rows of instance_cells.hpp one dimension down.  One WAVEFRONT takes one tile.
//   k_section_tiles (side > 8): lane 8 i + j is the child tile at (x0 + i * s, y0 + j * s), s = child_side.  Every candidate
//     of the parent is evaluated at the child's CENTRE, plane_point((float)x + h, (float)y + h), h = (s - 1) / 2.  The
//     child's samples lie within (s - 1) * step * sqrt(2) / 2 of it in the plane; r = a.thr is s * step * sqrt(2) / 2 times
//     (1 + 2^-10), the slack the cell levels leave for the rounding of positions and of w (section.py).  With |grad w| <= 1
//     a candidate k with w_k(centre) >= r has no sample inside the child, and one with w_k(centre) > m + 2 r, m the
//     least w of the parent's candidates at the centre, is greater than the least everywhere in the child: it can
//     neither be the minimum nor tie with it.  A child keeps k when w_k < r and (without WITH_DISTANCE) k's window
//     reaches the child, or (WITH_DISTANCE) when w_k <= m + 2 r; a value that is no number keeps its candidate.
//     Children with a candidate are compacted into the next list (kernels.hpp wg_compact_slots).
//   k_section_leaf (side 8): lane 8 j + i is the sample (x0 + i, y0 + j) -- the eight lanes of a tile's row store 32
//     contiguous bytes of an int32 map, a wavefront's store eight such segments.  Every candidate is evaluated there; the maps
//     are stored with ordinary vector stores, and each accumulator gets ONE atomic per wavefront.  Lanes past the lattice's
//     rim compute and neither store nor count.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the end of
// this file.
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// the point of the plane at the lattice indices (fi, fj): whole numbers for a sample, half-integers for a tile's centre
__device__ __forceinline__ Point plane_point(const SectionArgs& t, float fi, float fj)
{
    const float a = t.c.step * fi, b = t.c.step * fj;
    return Point{(t.c.corner[0] + t.u[0] * a) + t.v[0] * b, (t.c.corner[1] + t.u[1] * a) + t.v[1] * b,
                 (t.c.corner[2] + t.u[2] * a) + t.v[2] * b};
}

template <bool DO, bool WITH_DISTANCE>
__global__ void __launch_bounds__(256) k_section_tiles(const SectionArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    // after the register file: (WITH_DISTANCE) every candidate's w, [wavefront][instance][lane]; then the compaction's scratch
    float* wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 64u * a.n_instances;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset +
                                                    (WITH_DISTANCE ? 4u * a.n_instances * blockDim.x : 0u));
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    const uint32_t x = row.x0 + (lane >> 3) * s, y = row.y0 + (lane & 7u) * s;
    const bool live = row.have & (x < a.dims[0]) & (y < a.dims[1]);
    const float h = 0.5f * (float)(s - 1u);
    const Point p = plane_point(t, (float)x + h, (float)y + h);
    const uint32_t* windows = WITH_DISTANCE ? nullptr : constant_uniform(a.windows);
    uint64_t keep = 0ull;
    float least = __builtin_inff();
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        bool reach = true;
        if constexpr (!WITH_DISTANCE) {
            const uint32_t* win = windows + 6u * n;
            reach = (x <= win[3]) & (x + s - 1u >= win[0]) & (y <= win[4]) & (y + s - 1u >= win[1]);
        }
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        if (reach && !(w >= a.thr)) keep |= 1ull << n;            // may be inside somewhere in the child (a NaN keeps its candidate)
        if constexpr (WITH_DISTANCE) {
            wl[n * 64u + lane] = w;
            least = __builtin_fminf(least, w);                    // (of the numbers among them)
        }
    }
    if constexpr (WITH_DISTANCE) {
        const float bound = least + (a.thr + a.thr);
        for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {
            const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
            if (!(wl[n * 64u + lane] > bound)) keep |= 1ull << n; // may be the least, or tie with it, somewhere in the child
        }
    }
    // (the count and the child-row store stay spelled out: through a shared function this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && keep != 0ull};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity) a.children[slot[0]] = make_uint4(x | (y << 16), 0u, (uint32_t)keep, (uint32_t)(keep >> 32));
}

// least and greatest sample index per axis among the lanes of `b` (lane = 8 j + i of the tile at (x0, y0)); the third is 0
__device__ __forceinline__ void tile_box(uint64_t b, uint32_t x0, uint32_t y0, uint32_t (&lo)[3], uint32_t (&hi)[3])
{
    uint32_t columns = (uint32_t)(b | (b >> 32));
    columns |= columns >> 16;
    columns = (columns | (columns >> 8)) & 0xffu;                 // i of any j
    lo[0] = x0 + (uint32_t)__builtin_ctz(columns);
    hi[0] = x0 + 31u - (uint32_t)__builtin_clz(columns);
    lo[1] = y0 + ((uint32_t)__builtin_ctzll(b) >> 3);
    hi[1] = y0 + ((63u - (uint32_t)__builtin_clzll(b)) >> 3);
    lo[2] = hi[2] = 0u;
}

template <bool DO, bool WITH_DISTANCE>
__global__ void __launch_bounds__(256) k_section_leaf(const SectionArgs t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = row.x0 + (lane & 7u), y = row.y0 + (lane >> 3);
    const bool live = (x < a.dims[0]) & (y < a.dims[1]);
    const Point p = plane_point(t, (float)x, (float)y);
    uint64_t inside = 0ull, present = 0ull;                       // per lane; wave-uniform
    float best = __builtin_inff();
    uint32_t best_id = 0u;
    bool none = true;                                             // wave-uniform: no instance evaluated yet
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {       // the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        const bool in = live & (w < 0.0f);
        inside |= in ? 1ull << n : 0ull;
        present |= __ballot(in) ? 1ull << n : 0ull;
        if constexpr (WITH_DISTANCE) {
            // the first value as it is, then the hardware minimum of the chain; indices ascend, so the first to attain
            // the least value is the lowest
            const float least = none ? w : __builtin_fminf(best, w);
            const bool take = none | ((w == least) & (best != least));
            best = least;
            best_id = take ? n : best_id;
            none = false;
        }
    }
    // (spelled out: through instance_cells.hpp count_evaluations this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    if (live) {
        const size_t at = (size_t)y * a.dims[0] + x;
        t.part_ids[at] = inside ? (int32_t)__builtin_ctzll(inside) : -1;
        t.inside_count[at] = (uint8_t)__popcll(inside);
        if constexpr (WITH_DISTANCE) {
            t.distance[at] = best;
            t.nearest[at] = (int32_t)best_id;
        }
    }
    OverlapAcc* acc = static_cast<OverlapAcc*>(a.pairs);
    uint32_t lo[3], hi[3];
    for (uint64_t m = present; m != 0ull; m &= m - 1ull) {        // the samples inside k: the diagonal
        const uint32_t k = uniform((uint32_t)__builtin_ctzll(m));
        const bool mine = ((inside >> k) & 1ull) != 0ull;
        const uint64_t b = __ballot(mine);
        tile_box(b, row.x0, row.y0, lo, hi);
        add_samples(acc + (size_t)k * a.n_instances + k, mine, b, lane, x, y, 0u, lo, hi);
    }
    for_pairs(present, inside, [&](uint32_t i, uint32_t j, bool both, uint64_t b) __attribute__((always_inline)) {
        tile_box(b, row.x0, row.y0, lo, hi);
        add_samples(acc + (size_t)i * a.n_instances + j, both, b, lane, x, y, 0u, lo, hi);
    });
}

// [leaf][distance_only][with_distance]
void (*const kSectionTable[2][2][2])(SectionArgs) = {
    {{k_section_tiles<false, false>, k_section_tiles<false, true>}, {k_section_tiles<true, false>, k_section_tiles<true, true>}},
    {{k_section_leaf<false, false>, k_section_leaf<false, true>}, {k_section_leaf<true, false>, k_section_leaf<true, true>}},
};
HU_BIG_LDS(kSectionTable);

// What both entry points of the section check and fill: cells_args() of a lattice {dims u, dims v, 1} with windows, and the
// plane's frame.
int section_args(const hu_cells_launch* l, const float u[3], const float v[3], SectionArgs& t)
{
    if (!u || !v) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    std::memset(&t, 0, sizeof(t));
    int rc;
    if ((rc = cells_args(kWindows | kStrict | kPlanar, l, t.c))) return rc;
    if ((uint64_t)l->dims[0] * l->dims[1] > (1ull << 28)) return hu_fail(HU_ERR_BAD_ARG, "a section holds at most 2^28 samples");
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(u[i]) || !std::isfinite(v[i]) || !std::isfinite(l->corner[i])) return hu_fail(HU_ERR_BAD_ARG, "the plane's frame must be finite");
        t.u[i] = u[i];
        t.v[i] = v[i];
    }
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_section_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3],
                     int with_distance)
{
    SectionArgs t;
    int rc;
    if ((rc = section_args(launch, u, v, t))) return rc;
    if ((rc = cells_children(t.c, children))) return rc;
    if ((rc = check_child_side(t.c.child_side, 8u, 8192u))) return rc;
    if (std::isnan(t.c.thr) || t.c.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    // WITH_DISTANCE keeps every candidate's w at the children's centres: 4 bytes per instance and lane after the register file
    return cells_launch(kSectionTable[0][launch->distance_only != 0][with_distance != 0], t, t.c, *launch, with_distance ? 4u * launch->n : 0u);
}

int hu_section_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], int with_distance, int32_t* part_ids_dev,
                    uint8_t* inside_count_dev, float* distance_dev, int32_t* nearest_dev, void* acc_dev)
{
    SectionArgs t;
    int rc;
    if ((rc = section_args(launch, u, v, t))) return rc;
    if (!part_ids_dev || !inside_count_dev || !acc_dev || (with_distance && (!distance_dev || !nearest_dev)))
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = acc_dev;
    t.part_ids = part_ids_dev;
    t.inside_count = inside_count_dev;
    t.distance = distance_dev;
    t.nearest = nearest_dev;
    return cells_launch(kSectionTable[1][launch->distance_only != 0][with_distance != 0], t, t.c, *launch, 0u);
}

}  // extern "C"
