// codecad_amd/csrc/instance_cells.hpp -- what a kernel over the instances of an assembly is made of, each piece once:
//   the row    cell_row, the table of the instances' programs (constant_uniform, instance_dist);
//   the lane   leaf_lane (a sample of a finest cell), child_lane (a child cell of a level) with child_centre and reaches (a
//              window), count_evaluations;
//   the pairs  mask_box, for_pairs, add_samples;
//   the wavefront reductions  wave_sum64, wave_or64, wave_min_to_last_lane, and order_key;
//   the host side  cells_args, cells_children, check_child_side, cells_launch.
//
// A CELL is a cube of 4^k lattice samples, a 16-byte row {x0 | y0 << 16, z0, mask lo, mask hi}: its first sample's indices
// and the 64-bit mask of the instances still candidates in it.  One wavefront takes one cell, lane = 16 x + 4 y + z of its
// 4 x 4 x 4 parts.  Every such kernel takes hu_cells::Args (instance_args.hpp).
//
// THE KERNELS' INSTRUCTION STREAMS ARE PINNED (tools/compare_device_code.py between two revisions prints `identical`).  They
// inline the interpreter, and how a value is held across it decides registers and schedule, so a kernel takes a piece from
// here where it compiles to the same code with it, and says in a line where it does not.  Compiled and found different, each
// substitution alone:
//   leaf_lane           k_mass_leaf, k_gap_leaf<true> (k_voxel_leaf and k_mesh_leaf take it, and keep their own `lane`);
//   an evaluation count with the guard `&& lives` (as a template flag, and as a function of its own) in k_instance_cells,
//                       k_mesh_cells<true>, k_section_tiles, the outline tiles; with `&& todo` in k_mass_cells, k_mass_leaf and
//                       k_voxel_leaf; the plain one in k_section_leaf (k_voxel_cells counts lanes x evaluations run, another
//                       product, and the second passes of k_mesh_leaf and the outline leaf add a second ballot: not this form);
//   a child-row store (wg_compact_slots and the uint4 row in one function) in k_instance_cells, k_mesh_cells, k_voxel_cells
//                       and k_section_tiles; the outline tiles alone compiled the same, and one user is no shared form;
//   wave_sum64 and wave_or64 as one ladder over an operator: the kernels that sum.
// k_gap_cells recomputes its child_lane and spells out for_pairs for a stack frame's sake (instance_gap.hip).
#pragma once

#include <cmath>
#include <cstring>

#include "host.hpp"
#include "instance_args.hpp"
#include "kernels.hpp"

namespace hu_cells {

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the row of the cell wavefront `w` of this workgroup takes, or `have` = false past the list's end (wave-uniform)
struct CellRow {
    uint32_t x0, y0, z0;
    uint64_t mask;
    bool have;
};
__device__ __forceinline__ CellRow cell_row(const Args& a)
{
    const uint32_t listed = *a.n_parents_dev, n = listed < a.max_parents ? listed : a.max_parents;   // (an overflowed list holds max_parents)
    const uint32_t p = uniform(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    CellRow r{0u, 0u, 0u, 0ull, p < n};
    if (r.have) {
        const uint4 row = a.parents[p];
        r.x0 = uniform(row.x & 0xffffu);
        r.y0 = uniform(row.x >> 16);
        r.z0 = uniform(row.y);
        r.mask = ((uint64_t)uniform(row.w) << 32) | uniform(row.z);
    }
    return r;
}

// A pointer read from the device table is a plain value to the compiler: it cannot tell that it points to global memory
// this kernel never writes, so the interpreter would fetch the records through it with vector (flat) loads.  Made
// wave-uniform and cast through the constant address space, every load through it is a scalar load, as in the kernels
// that take their program as a kernel argument.
template <class T> __device__ __forceinline__ const T* constant_uniform(const T* p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint64_t u = ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
    return (const T*)(const __attribute__((address_space(4))) T*)u;
}

// distance of instance `n` (wave-uniform) at p: the one interpreter call site of a kernel
template <bool DO>
__device__ __forceinline__ float instance_dist(const Args& a, uint32_t n, float px, float py, float pz, void* lds)
{
    const auto r = a.table[n];
    return sdfk::InterpEval<DO>{constant_uniform(r.prog), constant_uniform(r.extra), uniform(r.n4)}.dist(px, py, pz, lds);
}

// the sample of a finest cell this lane takes, lane = 16 x + 4 y + z; `Row` has x0, y0, z0
struct LeafLane {
    uint32_t lane, x, y, z;
    bool live;
    float px, py, pz;
};
template <class Row> __device__ __forceinline__ LeafLane leaf_lane(const Args& a, const Row& row)
{
    LeafLane l;
    l.lane = threadIdx.x & 63u;
    l.x = row.x0 + (l.lane >> 4);
    l.y = row.y0 + ((l.lane >> 2) & 3u);
    l.z = row.z0 + (l.lane & 3u);
    l.live = (l.x < a.dims[0]) & (l.y < a.dims[1]) & (l.z < a.dims[2]);
    // exactly kernels.hpp sample() (the lattice of oracle.grid_eval)
    l.px = sdfk::sample(a.corner[0], a.step, l.x);
    l.py = sdfk::sample(a.corner[1], a.step, l.y);
    l.pz = sdfk::sample(a.corner[2], a.step, l.z);
    return l;
}

// the child cell of side a.child_side a lane of a level takes: its first sample's indices, and whether the row exists and the
// child has a sample inside dims
struct ChildLane {
    uint32_t x, y, z;
    bool live;
};
template <class Row> __device__ __forceinline__ ChildLane child_lane(const Args& a, const Row& row, uint32_t lane)
{
    const uint32_t s = a.child_side;
    ChildLane q;
    q.x = row.x0 + (lane >> 4) * s;
    q.y = row.y0 + ((lane >> 2) & 3u) * s;
    q.z = row.z0 + (lane & 3u) * s;
    q.live = row.have & (q.x < a.dims[0]) & (q.y < a.dims[1]) & (q.z < a.dims[2]);
    return q;
}
// ... its centre, a half-integer index per axis: the child's samples lie within (s - 1) * step * sqrt(3) / 2 of it
struct Point {
    float x, y, z;
};
__device__ __forceinline__ Point child_centre(const Args& a, const ChildLane& q)
{
    const float h = 0.5f * (float)(a.child_side - 1u);
    return Point{a.corner[0] + a.step * ((float)q.x + h), a.corner[1] + a.step * ((float)q.y + h), a.corner[2] + a.step * ((float)q.z + h)};
}
// ... and whether the index box win = {lo x, lo y, lo z, hi x, hi y, hi z} of an instance (wave-uniform) reaches it
__device__ __forceinline__ bool reaches(const uint32_t* win, const ChildLane& q, uint32_t s)
{
    return (q.x <= win[3]) & (q.x + s - 1u >= win[0]) & (q.y <= win[4]) & (q.y + s - 1u >= win[1]) & (q.z <= win[5]) &
           (q.z + s - 1u >= win[2]);
}

// One evaluation per live lane and instance of `candidates` (wave-uniform), counted once per wavefront: the finest kernels
// of instance_pairs.hip.  Every other kernel's count has a guard of its own (`&& lives`, `&& todo`, `evaluated`) and stays
// spelled out there: with the guard as a parameter, or as a second function, each of them compiled to other code.
__device__ __forceinline__ void count_evaluations(const Args& a, bool live, uint64_t candidates)
{
    const uint64_t lives = __ballot(live);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(candidates)));
}

// min and max of the lane coordinates set in a 64-lane mask (lane = 16 x + 4 y + z), per axis
__device__ __forceinline__ void mask_box(uint64_t m, uint32_t (&lo)[3], uint32_t (&hi)[3])
{
    const uint32_t f16 = (uint32_t)((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffull);   // (y, z) of any x
    uint32_t ys = 0u;
    for (uint32_t yy = 0; yy < 4u; ++yy) ys |= ((f16 >> (4u * yy)) & 0xfu) ? 1u << yy : 0u;
    const uint32_t zs = (f16 | (f16 >> 4) | (f16 >> 8) | (f16 >> 12)) & 0xfu;
    lo[0] = (uint32_t)__builtin_ctzll(m) >> 4;  hi[0] = (63u - (uint32_t)__builtin_clzll(m)) >> 4;
    lo[1] = (uint32_t)__builtin_ctz(ys);        hi[1] = 31u - (uint32_t)__builtin_clz(ys);
    lo[2] = (uint32_t)__builtin_ctz(zs);        hi[2] = 31u - (uint32_t)__builtin_clz(zs);
}

// f(i, j, both, b) for every pair i < j of `present` (wave-uniform) some lane has both of in its bitmask `mine`: `both`
// says whether this lane does, `b` is its ballot
template <class F> __device__ __forceinline__ void for_pairs(uint64_t present, uint64_t mine, F f)
{
    for (uint64_t mi = present; mi != 0ull; mi &= mi - 1ull) {
        const uint32_t i = uniform((uint32_t)__builtin_ctzll(mi));
        for (uint64_t mj = mi & (mi - 1ull); mj != 0ull; mj &= mj - 1ull) {
            const uint32_t j = uniform((uint32_t)__builtin_ctzll(mj));
            const bool both = ((mine >> i) & (mine >> j) & 1ull) != 0ull;
            const uint64_t b = __ballot(both);
            if (b == 0ull) continue;                              // wave-uniform
            f(i, j, both, b);
        }
    }
}

// the lanes of `b` (this lane: `both`, its sample at the indices x, y, z) added to an accumulator's count, index sums and
// index box; lo and hi are the least and the greatest index per axis among the samples of b (wave-uniform)
template <class Acc>
__device__ __forceinline__ void add_samples(Acc* acc, bool both, uint64_t b, uint32_t lane, uint32_t x, uint32_t y, uint32_t z,
                                            const uint32_t (&lo)[3], const uint32_t (&hi)[3])
{
    const uint32_t sx = __builtin_amdgcn_readlane(sdfk::wave_sum_to_last_lane(both ? x : 0u), 63);
    const uint32_t sy = __builtin_amdgcn_readlane(sdfk::wave_sum_to_last_lane(both ? y : 0u), 63);
    const uint32_t sz = __builtin_amdgcn_readlane(sdfk::wave_sum_to_last_lane(both ? z : 0u), 63);
    // lanes 0-3: the u64 sums, 4-6: the minima, 7-9: the maxima -- each accumulator once per wavefront
    const unsigned long long add = lane == 0u ? (unsigned long long)__popcll(b) : lane == 1u ? sx : lane == 2u ? sy : sz;
    const uint32_t k = lane < 7u ? lane - 4u : lane - 7u;
    const uint32_t bound = lane < 7u ? (k == 0u ? lo[0] : k == 1u ? lo[1] : lo[2]) : (k == 0u ? hi[0] : k == 1u ? hi[1] : hi[2]);
    if (lane < 4u) atomicAdd(&acc->sums[lane], add);
    else if (lane < 7u) atomicMin(&acc->lo[k], bound);
    else if (lane < 10u) atomicMax(&acc->hi[k], bound);
}

// Sum, or OR, of a 64-bit value over the 64 lanes of a wavefront, wave-uniform: kernels.hpp wave_sum_to_last_lane on both
// halves, the carry propagated by the 64-bit add of every step (lanes without a source give 0, the identity of both).
template <int CTRL, int ROWS> __device__ __forceinline__ unsigned long long dpp64(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROWS, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
    v += dpp64<0x111, 0xf>(v);   // row_shr:1
    v += dpp64<0x112, 0xf>(v);   // row_shr:2
    v += dpp64<0x114, 0xf>(v);   // row_shr:4
    v += dpp64<0x118, 0xf>(v);   // row_shr:8: lane 15 of a row = its total
    v += dpp64<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v += dpp64<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}
// (a ladder folded over an operator changes the code of the kernels that sum: two spellings)
__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v)
{
    v |= dpp64<0x111, 0xf>(v);   // row_shr:1
    v |= dpp64<0x112, 0xf>(v);   // row_shr:2
    v |= dpp64<0x114, 0xf>(v);   // row_shr:4
    v |= dpp64<0x118, 0xf>(v);   // row_shr:8: lane 15 of a row = its total
    v |= dpp64<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v |= dpp64<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// Minimum over the 64 lanes of a wavefront; it arrives in lane 63.  kernels.hpp wave_sum_to_last_lane with min for +
// (lanes without a source take 0xffffffff, the identity).
__device__ __forceinline__ uint32_t wave_min_to_last_lane(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}

// the key of v in an order that unsigned comparison keeps: -0 and +0 get the one key of +0 (clearance.py and separation.py
// decode it)
__device__ __forceinline__ uint32_t order_key(float v)
{
    const uint32_t b = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ------------------------------------------------------------------------------------------
// host side: the entry points over instance cells
// ------------------------------------------------------------------------------------------

// What every entry point over instance cells checks and fills, from its launch record (hip_util.h).  `want` says what the
// check needs beyond interference's, whose entry points were released without these and keep accepting what they accepted:
//   kWindows  the windows are read: not NULL;
//   kStrict   a z extent within 16 bits (a witness packs an index into 16 bits per axis, the sums count on it) and a finite
//             step >= 0;
//   kPlanar   the lattice lies on a plane, {dims[0], dims[1], 1}, and dims[2] is not read.
enum : uint32_t { kWindows = 1u, kStrict = 2u, kPlanar = 4u };
inline int cells_args(uint32_t want, const hu_cells_launch* l, Args& a)
{
    if (!l || !l->table_dev || ((want & kWindows) && !l->windows_dev) || !l->n_parents_dev || !l->evaluations_dev || (!l->parents_dev && l->max_parents))
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    const uint32_t dims[3] = {l->dims[0], l->dims[1], (want & kPlanar) ? 1u : l->dims[2]};
    if (l->n == 0 || l->n > 64u) return hu_fail(HU_ERR_BAD_ARG, "1..64 instances");
    // Two wordings, each entry point's as it was released.  The checks that read windows (clearance, mesh, section, outlines)
    // were released with the strict test and say `tight` for any bad dimension.  Interference was released with the loose
    // test; mass, voxels and separation added the z bound and the step test after it: loose wording for a zero or an x, y
    // past 65536, tight for z alone.  kWindows stands for "released strict" here, which is what tells the two groups apart.
    const char* const tight = "lattice dims must be in 1..65536";
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0 || dims[0] > 65536u || dims[1] > 65536u)
        return hu_fail(HU_ERR_BAD_ARG, (want & kWindows) ? tight : "lattice dims must be positive, x and y at most 65536");
    if ((want & kStrict) && dims[2] > 65536u) return hu_fail(HU_ERR_BAD_ARG, tight);
    if ((want & kStrict) && (!std::isfinite(l->step) || l->step < 0.0f)) return hu_fail(HU_ERR_BAD_ARG, "step must be finite and not negative");
    std::memset(&a, 0, sizeof(a));
    a.table = static_cast<const InstanceRec*>(l->table_dev);
    a.windows = l->windows_dev;
    a.n_instances = l->n;
    a.parents = static_cast<const uint4*>(l->parents_dev);
    a.n_parents_dev = l->n_parents_dev;
    a.max_parents = l->max_parents;
    for (int i = 0; i < 3; ++i) {
        a.dims[i] = dims[i];
        a.corner[i] = l->corner[i];
    }
    a.step = l->step;
    a.evaluations = reinterpret_cast<unsigned long long*>(l->evaluations_dev);
    return HU_OK;
}

// ... and what those of a level above the finest one add, from its record: the children's list, their side and the threshold
// that drops a candidate.  The bounds of child_side and thr are each check's own: its entry point tests them after this,
// the side with check_child_side().
inline int cells_children(Args& a, const hu_cells_children* c)
{
    if (!c || !c->counter_dev || (!c->children_dev && c->capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    a.child_side = c->child_side;
    a.thr = c->thr;
    a.counter = c->counter_dev;
    a.children = static_cast<uint4*>(c->children_dev);
    a.capacity = c->capacity;
    return HU_OK;
}

inline int check_child_side(uint32_t side, uint32_t least, uint32_t most, bool power_of_two = true)
{
    if (side >= least && side <= most && !(power_of_two && (side & (side - 1u)))) return HU_OK;
    return hu_fail(HU_ERR_BAD_ARG, std::string("child_side must be ") + (power_of_two ? "a power of two in " : "in ") + std::to_string(least) +
                                        ".." + std::to_string(most));
}

// The launch of `kernel` over the cells of `a`, which is `k` or a part of it, on the record's stream: a wavefront per cell,
// in workgroups of four wavefronts while their LDS fits 48 KiB (host.hpp hu_workgroup), as launch_shape() sizes the one-voxel
// interpreter kernels.  A lane's LDS: the record's lane_bytes, the register file of the largest instance, then
// `extra_lane_bytes` (clearance's w area at the finest level, the section's at its tiles: 4 bytes per instance and lane).
template <class K>
int cells_launch(void (*kernel)(K), K& k, Args& a, const hu_cells_launch& l, size_t extra_lane_bytes)
{
    uint32_t block;
    size_t lds;
    int rc;
    // the scalar slots and every area after the register file are read as 4-byte words at lane_bytes * block
    if (l.lane_bytes % 4u) return hu_fail(HU_ERR_BAD_ARG, "lane_bytes must be a multiple of 4");
    if ((rc = hu_workgroup((size_t)l.lane_bytes + extra_lane_bytes, block, lds))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    a.scratch_offset = l.lane_bytes * block;
    const uint64_t blocks = ((uint64_t)a.max_parents + block / 64u - 1) / (block / 64u);
    if (blocks == 0) return HU_OK;
    if (blocks > 0x7fffffffull) return hu_fail(HU_ERR_BAD_ARG, "cell list too long for one launch");
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(block), lds, (hipStream_t)l.stream, k);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // namespace hu_cells
