// codecad_amd/csrc/instance_gap.hip
//
// The SEPARATION of every pair of instances of an assembly (codecad_amd/separation.py): per pair i < j the least
// v = max(w_i, w_j) over the lattice samples of interference() where both values are numbers, as the order key of
// instance_pairs.hip (unsigned comparison orders the keys as the values, either zero has the key of +0), and the
// lexicographically smallest sample that attains it.  Bit for bit what evaluating every instance at every sample gives.
//
// The traversal is the one of instance_pairs.hip -- 16-byte rows {x0 | y0 << 16, z0, mask lo, mask hi}, cubic cells of 4^k
// samples, one wavefront per cell, lane = 16 x + 4 y + z -- but no fixed threshold prunes it: a BRANCH AND BOUND.  Per level
// boundary there is one array of keys [n][n], U_0 (all ones: nothing known) .. U_L, and the final one after the leaf.  The
// entry point of level l copies U_l to U_{l+1} on the stream, then its kernel reads U_l only, which no launch writes any
// more, and lowers U_{l+1}: every bound a cell is pruned with is final when it is read, so the rows, the evaluations and the
// results do not depend on the order the wavefronts run in.
//   k_gap_cells (child side s >= 4): a lane is a child cell.  Every candidate of the parent is evaluated at the child's
//     lattice sample q = min(first + s / 2, dims - 1) per axis -- a sample, not the half-integer centre, so v(q) is an upper
//     bound on the pair's least v whatever the fields are -- and waits in the wavefront's LDS area, [instance][lane].  Every
//     sample of the child, clipped to dims, lies within (s / 2) * step * sqrt(3) of q, and a.thr = r is a little more than
//     that (separation.py).  The pair (i, j) is DROPPED in the child iff (v(q) - U_l[i][j]) > r in binary32, strictly: with
//     distances of Lipschitz constant at most 1 every sample of the child then has v > U_l[i][j], which a sample attains.
//     A NaN, in v or in the bound, keeps the pair.  The child keeps the bits of its kept pairs and is listed when it has
//     any (kernels.hpp wg_compact_slots).  Per pair the wavefront's least key of v(q) goes to U_{l+1}[i][j] with one atomic
//     min from one lane, and only when it is below the key read.
//   k_gap_leaf (side 4): a lane is a sample.  Every candidate is evaluated at the samples inside dims; per pair of
//     candidates the wavefront's least key goes to the final array in the same way.
//   k_gap_witness (side 4), launched after the leaf over the same list: evaluates again and, for every pair, its first
//     lane whose v has the pair's final key gives one u64 atomicMin of x << 32 | y << 16 | z (k_clearance_witness's rule).
// After the keys the accumulators hold one word per level: the entry points copy each list's length there, so that the one
// read at the end of the traversal also brings the rows every level listed.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the
// end of this file.
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// the float32 of an order_key() (separation.py decodes it alike); the key of all ones, nothing known yet, is a NaN
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Every candidate of `row` evaluated at this lane's point, into the wavefront's LDS area (after the register file) at
// wl[n * 64 + lane]; live lanes x candidates counted once per wavefront.  The one interpreter call site of a kernel.
struct GapLane {
    float* wl;
    uint32_t lane;
    // v = max(w_i, w_j) of this lane where both are numbers, else a NaN
    __device__ __forceinline__ float v(uint32_t i, uint32_t j) const
    {
        const float wi = wl[i * 64u + lane], wj = wl[j * 64u + lane];
        return ((wi == wi) & (wj == wj)) ? fmaxf(wi, wj) : __uint_as_float(0x7fc00000u);
    }
};
template <bool DO>
__device__ __forceinline__ GapLane gap_lane(const Args& a, const CellRow& row, bool live, float px, float py, float pz)
{
    extern __shared__ float4 lds[];
    GapLane g;
    g.wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 64u * a.n_instances;
    g.lane = threadIdx.x & 63u;
    const uint64_t lives = __ballot(live);
    if (g.lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        g.wl[n * 64u + g.lane] = instance_dist<DO>(a, n, px, py, pz, lds);
    }
    return g;
}

// the wavefront's least key of a pair (this lane: `key`, all ones where it has none) into next[pair], from one lane and only
// when it lowers the key `known` that was read for the pair
__device__ __forceinline__ void lower_key(uint32_t* next, uint32_t pair, uint32_t key, uint32_t known, uint32_t lane)
{
    const uint32_t kmin = (uint32_t)__builtin_amdgcn_readlane((int)wave_min_to_last_lane(key), 63);
    if (kmin < known && lane == 0u) atomicMin(next + pair, kmin);
}

template <bool DO>
__global__ void __launch_bounds__(256) k_gap_cells(const GapArgs g)
{
    extern __shared__ float4 lds[];
    const Args& a = g.c;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    GapLane c;
    {
        // the child's sample q, exactly kernels.hpp sample(): a lattice sample of the child, clipped as the child is
        const ChildLane q = child_lane(a, row, threadIdx.x & 63u);
        const uint32_t h = s >> 1;
        c = gap_lane<DO>(a, row, q.live, sample(a.corner[0], a.step, min(q.x + h, a.dims[0] - 1u)),
                         sample(a.corner[1], a.step, min(q.y + h, a.dims[1] - 1u)), sample(a.corner[2], a.step, min(q.z + h, a.dims[2] - 1u)));
    }
    // the child's indices again, from a lane the compiler takes as new: held across the interpreter they cost it a stack frame
    uint32_t lane = c.lane;
    asm volatile("" : "+v"(lane));
    const ChildLane q = child_lane(a, row, lane);
    const uint32_t x = q.x, y = q.y, z = q.z;
    const bool live = q.live;
    const uint32_t* bound = constant_uniform(g.bound);
    uint64_t keep = 0ull;
    // every pair of candidates (instance_cells.hpp for_pairs, spelled out: the lambda's closure cost this kernel a stack frame)
    for (uint64_t mi = row.mask; mi != 0ull; mi &= mi - 1ull) {  // wave-uniform
        const uint32_t i = uniform((uint32_t)__builtin_ctzll(mi));
        for (uint64_t mj = mi & (mi - 1ull); mj != 0ull; mj &= mj - 1ull) {
            const uint32_t j = uniform((uint32_t)__builtin_ctzll(mj));
            const uint32_t pair = i * a.n_instances + j;
            const uint32_t known = bound[pair];                   // final before this launch: a scalar load
            const float v = c.v(i, j);
            // the subtraction first: exact where the decision is close (Sterbenz); a NaN on either side compares false
            if (live && !((v - key_value(known)) > a.thr)) keep |= (1ull << i) | (1ull << j);
            lower_key(g.next, pair, live && v == v ? order_key(v) : 0xffffffffu, known, lane);
        }
    }
    // after the register file: every candidate's w, [wavefront][instance][lane]; then the compaction's scratch
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset +
                                                    (size_t)blockDim.x * a.n_instances * sizeof(float));
    const bool flag[1] = {keep != 0ull};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
}

template <bool DO>
__global__ void __launch_bounds__(256) k_gap_leaf(const GapArgs g)
{
    const Args& a = g.c;
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    // instance_cells.hpp leaf_lane, spelled out: the shared struct renames this kernel's registers
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = row.x0 + (lane >> 4), y = row.y0 + ((lane >> 2) & 3u), z = row.z0 + (lane & 3u);
    const bool live = (x < a.dims[0]) & (y < a.dims[1]) & (z < a.dims[2]);
    const GapLane c = gap_lane<DO>(a, row, live, sample(a.corner[0], a.step, x), sample(a.corner[1], a.step, y), sample(a.corner[2], a.step, z));
    const uint32_t* bound = constant_uniform(g.bound);
    for_pairs(row.mask, live ? row.mask : 0ull, [&](uint32_t i, uint32_t j, bool both, uint64_t) __attribute__((always_inline)) {
        const uint32_t pair = i * a.n_instances + j;
        const float v = c.v(i, j);
        lower_key(g.next, pair, both && v == v ? order_key(v) : 0xffffffffu, bound[pair], c.lane);
    });
}

template <bool DO>
__global__ void __launch_bounds__(256) k_gap_witness(const GapArgs g)
{
    const Args& a = g.c;
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    const GapLane c = gap_lane<DO>(a, row, l.live, l.px, l.py, l.pz);
    const uint32_t* bound = constant_uniform(g.bound);
    for_pairs(row.mask, l.live ? row.mask : 0ull, [&](uint32_t i, uint32_t j, bool both, uint64_t) __attribute__((always_inline)) {
        const uint32_t pair = i * a.n_instances + j;
        // the leaf launch has finished: the least key is final, and this kernel never writes it (a scalar load)
        const uint32_t least = bound[pair];
        const float v = c.v(i, j);
        const uint64_t b = __ballot(both && v == v && order_key(v) == least);
        // lanes go 16 x + 4 y + z: the wavefront's first such lane is its lexicographically smallest sample
        if (b != 0ull && c.lane == (uint32_t)__builtin_ctzll(b))
            atomicMin(g.witness + pair, ((unsigned long long)l.x << 32) | ((unsigned long long)l.y << 16) | l.z);
    });
}

// [kernel][distance_only]
void (*const kGapTable[3][2])(GapArgs) = {
    {k_gap_cells<false>, k_gap_cells<true>},
    {k_gap_leaf<false>, k_gap_leaf<true>},
    {k_gap_witness<false>, k_gap_witness<true>},
};
HU_BIG_LDS(kGapTable);

// Where the accumulators keep what: n^2 uint64 witnesses, then the key arrays U_0 .. U_L and the final one, n^2 uint32
// each, then L uint32: the rows each level listed.  L, the levels above the finest one, comes from the top side 16 * 4^k.
struct GapLayout {
    unsigned long long* witness;
    uint32_t* keys;
    uint32_t* rows;
    uint32_t levels;
    size_t n2;
    uint32_t* key_array(uint32_t k) const { return keys + k * n2; }
};
int gap_layout(void* acc_dev, uint32_t n, uint32_t top_side, GapLayout& out)
{
    if (!acc_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    uint32_t levels = 0;
    for (uint32_t s = 16u; s <= 65536u && !levels; s *= 4u)
        if (s == top_side) {
            for (uint32_t t = s; t > 4u; t /= 4u) ++levels;
        }
    if (!levels) return hu_fail(HU_ERR_BAD_ARG, "top_side must be 16 * 4^k, at most 65536");
    out.n2 = (size_t)n * n;
    out.witness = static_cast<unsigned long long*>(acc_dev);
    out.keys = reinterpret_cast<uint32_t*>(out.witness + out.n2);
    out.rows = out.keys + (levels + 2u) * out.n2;
    out.levels = levels;
    return HU_OK;
}

// What the three entry points check and fill alike: cells_args() of a strict lattice (the witness packs an index into 16
// bits per axis).
int gap_args(const hu_cells_launch* l, GapArgs& g)
{
    std::memset(&g, 0, sizeof(g));
    return cells_args(kStrict, l, g.c);
}

// a launch over the finest cells: the leaf (level rows and the copy of the keys first) or the witness
int gap_finest(bool witness, const hu_cells_launch* l, uint32_t top_side, void* acc_dev)
{
    GapArgs g;
    GapLayout at;
    int rc;
    if ((rc = gap_args(l, g))) return rc;
    if ((rc = gap_layout(acc_dev, l->n, top_side, at))) return rc;
    g.c.child_side = 1u;
    g.witness = at.witness;
    if (witness) {
        g.bound = at.key_array(at.levels + 1u);
    } else {
        g.bound = at.key_array(at.levels);
        g.next = at.key_array(at.levels + 1u);
        HU_HIP(hipMemcpyAsync(at.rows + (at.levels - 1u), l->n_parents_dev, sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)l->stream));
        HU_HIP(hipMemcpyAsync(g.next, g.bound, at.n2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)l->stream));
    }
    return cells_launch(kGapTable[witness ? 2 : 1][l->distance_only != 0], g, g.c, *l, 4u * l->n);
}

}  // namespace

extern "C" {

int hu_separation_cells(const hu_cells_launch* launch, const hu_cells_children* children, uint32_t top_side, void* acc_dev)
{
    GapArgs g;
    GapLayout at;
    int rc;
    if ((rc = gap_args(launch, g))) return rc;
    if ((rc = cells_children(g.c, children))) return rc;
    if ((rc = gap_layout(acc_dev, launch->n, top_side, at))) return rc;
    if (!std::isfinite(g.c.thr) || g.c.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "r must be finite and not negative");
    // the level of the cells whose children have child_side: 0 for the top side's
    uint32_t level = at.levels;
    for (uint32_t s = top_side / 4u, l = 0; s >= 4u; s /= 4u, ++l)
        if (s == g.c.child_side) level = l;
    if (level == at.levels) return hu_fail(HU_ERR_BAD_ARG, "child_side must be top_side / 4^k, at least 4");
    g.bound = at.key_array(level);
    g.next = at.key_array(level + 1u);
    g.witness = at.witness;
    hipStream_t stream = (hipStream_t)launch->stream;
    if (level)
        HU_HIP(hipMemcpyAsync(at.rows + (level - 1u), launch->n_parents_dev, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    HU_HIP(hipMemcpyAsync(g.next, g.bound, at.n2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    return cells_launch(kGapTable[0][launch->distance_only != 0], g, g.c, *launch, 4u * launch->n);
}

int hu_separation_leaf(const hu_cells_launch* launch, uint32_t top_side, void* acc_dev)
{
    return gap_finest(false, launch, top_side, acc_dev);
}

int hu_separation_witness(const hu_cells_launch* launch, uint32_t top_side, void* acc_dev)
{
    return gap_finest(true, launch, top_side, acc_dev);
}

}  // extern "C"
