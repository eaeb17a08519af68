// codecad_amd/csrc/instance_pairs.hip
//
// The checks between the instances of an assembly: INTERFERENCE (codecad_amd/interference.py), which pairs of instances
// have lattice samples inside both, how many, where; and CLEARANCE (codecad_amd/clearance.py), which pairs come closer
// than a gap, and where.  Every instance has a tape of its own; the kernels reach them through a device table
// (InstanceRec) and evaluate them with the tape interpreter, one instance at a time, the instance index wave-uniform so
// that its records still arrive through scalar loads.
//
// The lattice is cut into cubic CELLS of side 4^k samples; a cell is a 16-byte row {x0 | y0 << 16, z0, mask lo, mask hi}:
// its first sample's indices and the 64-bit mask of the instances that may still matter in it (candidates).
// One WAVEFRONT takes one cell and its 64 lanes take the cell's 4 x 4 x 4 parts, lane = 16 x + 4 y + z
// (instance_cells.hpp).  Clearance is interference's traversal with a threshold t > 0 instead of 0 and a WINDOW per
// instance, an index box the host computes: a sample is NEAR the pair (i, j) when it lies in both instances' windows
// and w_i < t, w_j < t; there v = max(w_i, w_j).
//   k_instance_cells (side > 4): a lane is a child cell; every candidate is evaluated at the child's centre and dropped
//     where its distance proves it has no sample inside (interference) or near (clearance: or where the child misses
//     its window, WINDOWED) the child; children with >= 2 candidates left are compacted into the next list (ballots,
//     one atomic per workgroup: kernels.hpp wg_compact_slots);
//   k_interference_leaf (side 4): a lane is a sample; every candidate is evaluated there, which gives the lane's
//     inside bitmask (w < 0, strictly), and every pair of candidates with a sample inside both adds its count, index
//     sums and index box to the pair's accumulators (one atomic per accumulator per wavefront);
//   k_clearance_leaf (side 4): the same with the near bitmask, every w kept in the wavefront's LDS area, [instance][lane],
//     so that a pair also gives the least order key of v;
//   k_clearance_witness (side 4), launched after the leaf over the same list: evaluates again and, for every pair, its
//     first lane whose v has the pair's final least key gives one u64 atomicMin of x << 32 | y << 16 | z.  Lanes go
//     16 x + 4 y + z, so the wavefront's first such lane is its lexicographically smallest sample.
// All read their parent count from the list's header on the device (the *_indirect pattern of the other level kernels).
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the
// end of this file.
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

template <bool DO, bool WINDOWED>
__global__ void __launch_bounds__(256) k_instance_cells(const Args a)
{
    extern __shared__ float4 lds[];
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    const ChildLane q = child_lane(a, row, lane);
    const uint32_t x = q.x, y = q.y, z = q.z;
    const bool live = q.live;
    // the child's centre; its samples lie within (s - 1) * step * sqrt(3) / 2 of it, a.thr is t (interference: 0) plus
    // more than that (interference.py)
    const Point p = child_centre(a, q);
    const uint32_t* windows = WINDOWED ? constant_uniform(a.windows) : nullptr;
    uint64_t keep = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        bool reach = true;
        if constexpr (WINDOWED) {
            const uint32_t* win = windows + 6u * n;
            reach = reaches(win, q, s);
        }
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        if (reach && !(w >= a.thr)) keep |= 1ull << n;            // (a NaN keeps its candidate)
    }
    // (the count and the child-row store stay spelled out: through a shared function this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && __popcll(keep) >= 2};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
}

// the lanes of `b` (this lane: `both`) added to a pair's count, index sums and index box
template <class Acc>
__device__ __forceinline__ void add_samples(Acc* acc, bool both, uint64_t b, const LeafLane l, const CellRow row)
{
    uint32_t lo[3], hi[3];
    mask_box(b, lo, hi);
    const uint32_t origin[3] = {row.x0, row.y0, row.z0};
    for (int k = 0; k < 3; ++k) {
        lo[k] += origin[k];
        hi[k] += origin[k];
    }
    add_samples(acc, both, b, l.lane, l.x, l.y, l.z, lo, hi);
}

template <bool DO>
__global__ void __launch_bounds__(256) k_interference_leaf(const Args a)
{
    extern __shared__ float4 lds[];
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    uint64_t inside = 0ull, present = 0ull;                       // per lane; wave-uniform
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, l.px, l.py, l.pz, lds);
        const bool in = l.live & (w < 0.0f);
        inside |= in ? 1ull << n : 0ull;
        present |= __ballot(in) ? 1ull << n : 0ull;
    }
    count_evaluations(a, l.live, row.mask);
    for_pairs(present, inside, [&](uint32_t i, uint32_t j, bool both, uint64_t b) __attribute__((always_inline)) {
        add_samples(static_cast<OverlapAcc*>(a.pairs) + (size_t)i * a.n_instances + j, both, b, l, row);
    });
}

// Clearance's finest cell: every candidate evaluated at the lane's sample, w into the wavefront's LDS area (after the
// register file) at wl[n * 64 + lane].  `near` is the lane's near bitmask (in n's window and w < t, strictly: a NaN is
// never near), `present` the instances with a near lane (wave-uniform).
struct NearLeaf {
    float* wl;
    uint64_t near, present;
    __device__ __forceinline__ uint32_t key(uint32_t i, uint32_t j, uint32_t lane) const
    {
        return order_key(fmaxf(wl[i * 64u + lane], wl[j * 64u + lane]));
    }
};
template <bool DO> __device__ __forceinline__ NearLeaf near_leaf(const Args& a, const CellRow& row, const LeafLane& l)
{
    extern __shared__ float4 lds[];
    NearLeaf r;
    r.wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 64u * a.n_instances;
    r.near = r.present = 0ull;
    const uint32_t* windows = constant_uniform(a.windows);
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool in = l.live & (l.x >= win[0]) & (l.x <= win[3]) & (l.y >= win[1]) & (l.y <= win[4]) & (l.z >= win[2]) &
                        (l.z <= win[5]);
        const float w = instance_dist<DO>(a, n, l.px, l.py, l.pz, lds);
        r.wl[n * 64u + l.lane] = w;
        r.near |= (in & (w < a.t)) ? 1ull << n : 0ull;
    }
    count_evaluations(a, l.live, row.mask);
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        r.present |= __ballot((r.near >> n) & 1ull) ? 1ull << n : 0ull;
    }
    return r;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_clearance_leaf(const Args a)
{
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    const NearLeaf c = near_leaf<DO>(a, row, l);
    for_pairs(c.present, c.near, [&](uint32_t i, uint32_t j, bool both, uint64_t b) __attribute__((always_inline)) {
        const uint32_t kmin = __builtin_amdgcn_readlane(wave_min_to_last_lane(both ? c.key(i, j, l.lane) : 0xffffffffu), 63);
        NearAcc* acc = static_cast<NearAcc*>(a.pairs) + (size_t)i * a.n_instances + j;
        add_samples(acc, both, b, l, row);
        if (l.lane == 10u) atomicMin(&acc->key, kmin);            // lane 10: the least key, once per wavefront
    });
}

template <bool DO>
__global__ void __launch_bounds__(256) k_clearance_witness(const Args a)
{
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    const NearLeaf c = near_leaf<DO>(a, row, l);
    for_pairs(c.present, c.near, [&](uint32_t i, uint32_t j, bool both, uint64_t) __attribute__((always_inline)) {
        NearAcc* acc = static_cast<NearAcc*>(a.pairs) + (size_t)i * a.n_instances + j;
        // the leaf launch has finished: the least key is final, and this kernel never writes it (a scalar load)
        const uint32_t kmin = *constant_uniform(&acc->key);
        const uint64_t b = __ballot(both && c.key(i, j, l.lane) == kmin);
        if (b != 0ull && l.lane == (uint32_t)__builtin_ctzll(b))
            atomicMin(&acc->witness, ((unsigned long long)l.x << 32) | ((unsigned long long)l.y << 16) | l.z);
    });
}

void (*const kKernels[])(Args) = {
    k_instance_cells<false, false>, k_instance_cells<true, false>, k_interference_leaf<false>, k_interference_leaf<true>,
    k_instance_cells<false, true>,  k_instance_cells<true, true>,  k_clearance_leaf<false>,    k_clearance_leaf<true>,
    k_clearance_witness<false>,     k_clearance_witness<true>,
};
HU_BIG_LDS(kKernels);

// a level of cells above the finest one, of either check
int cells_level(bool clearance, const hu_cells_launch* l, const hu_cells_children* c)
{
    Args a;
    int rc;
    if ((rc = cells_args(clearance ? kWindows | kStrict : 0u, l, a))) return rc;
    if ((rc = cells_children(a, c))) return rc;
    if ((rc = check_child_side(a.child_side, 4u, 16384u, false))) return rc;   // (released without the power-of-two test)
    if (clearance && (!std::isfinite(a.thr) || a.thr < 0.0f)) return hu_fail(HU_ERR_BAD_ARG, "thr must be finite and not negative");
    const auto kernel = clearance ? (l->distance_only ? k_instance_cells<true, true> : k_instance_cells<false, true>)
                                  : (l->distance_only ? k_instance_cells<true, false> : k_instance_cells<false, false>);
    return cells_launch(kernel, a, a, *l, 0u);
}

// a launch over the finest cells, kernels[distance_only]: interference's leaf (no windows, no t), clearance's leaf or witness
int cells_finest(void (*const (&kernels)[2])(Args), bool clearance, const hu_cells_launch* l, float t, void* pairs_dev)
{
    Args a;
    int rc;
    if ((rc = cells_args(clearance ? kWindows | kStrict : 0u, l, a))) return rc;
    if (!pairs_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (clearance && (!std::isfinite(t) || t < 0.0f)) return hu_fail(HU_ERR_BAD_ARG, "t must be finite and not negative");
    a.child_side = 1u;
    a.t = t;
    a.pairs = pairs_dev;
    return cells_launch(kernels[l->distance_only != 0], a, a, *l, clearance ? 4u * l->n : 0u);
}

}  // namespace

extern "C" {

int hu_interference_cells_indirect(const hu_cells_launch* launch, const hu_cells_children* children)
{
    return cells_level(false, launch, children);
}

int hu_interference_leaf_indirect(const hu_cells_launch* launch, void* pairs_dev)
{
    return cells_finest({k_interference_leaf<false>, k_interference_leaf<true>}, false, launch, 0.0f, pairs_dev);
}

int hu_clearance_cells_indirect(const hu_cells_launch* launch, const hu_cells_children* children)
{
    return cells_level(true, launch, children);
}

int hu_clearance_leaf_indirect(const hu_cells_launch* launch, float t, void* pairs_dev)
{
    return cells_finest({k_clearance_leaf<false>, k_clearance_leaf<true>}, true, launch, t, pairs_dev);
}

int hu_clearance_witness_indirect(const hu_cells_launch* launch, float t, void* pairs_dev)
{
    return cells_finest({k_clearance_witness<false>, k_clearance_witness<true>}, true, launch, t, pairs_dev);
}

}  // extern "C"
