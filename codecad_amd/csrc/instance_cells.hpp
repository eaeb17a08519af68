// codecad_amd/csrc/instance_cells.hpp -- what a kernel over the instances of an assembly is made of (instance_pairs.hip):
// a wavefront's cell row, the table of the instances' programs, the box of a lane mask and the accumulators of a pair
// (instance_section.hip builds the section of an assembly from the same pieces, over square tiles of a plane).
//
// A CELL is a cube of 4^k lattice samples, a 16-byte row {x0 | y0 << 16, z0, mask lo, mask hi}: its first sample's indices
// and the 64-bit mask of the instances still candidates in it.  One wavefront takes one cell, lane = 16 x + 4 y + z of its
// 4 x 4 x 4 parts.  Every such kernel takes hu_cells::Args (instance_args.hpp).  The end of this file has what the entry
// points of such kernels check, fill and launch alike.
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

// ------------------------------------------------------------------------------------------
// host side: the entry points over instance cells (instance_pairs.hip, instance_section.hip, instance_mass.hip)
// ------------------------------------------------------------------------------------------

// What every entry point over instance cells checks and fills, from its launch record (hip_util.h).  The entry points of
// `clearance` also want the windows, a z extent within 16 bits (the witness packs an index into 16 bits per axis) and a
// finite step >= 0; interference's were released without those checks and keep accepting what they accepted.  `planar`:
// the lattice lies on a plane, {dims[0], dims[1], 1}, and dims[2] is not read.
inline int cells_args(bool clearance, const hu_cells_launch* l, Args& a, bool planar = false)
{
    if (!l || !l->table_dev || (clearance && !l->windows_dev) || !l->n_parents_dev || !l->evaluations_dev || (!l->parents_dev && l->max_parents))
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    const uint32_t dims[3] = {l->dims[0], l->dims[1], planar ? 1u : l->dims[2]};
    if (l->n == 0 || l->n > 64u) return hu_fail(HU_ERR_BAD_ARG, "1..64 instances");
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0 || dims[0] > 65536u || dims[1] > 65536u || (clearance && dims[2] > 65536u))
        return hu_fail(HU_ERR_BAD_ARG, clearance ? "lattice dims must be in 1..65536" : "lattice dims must be positive, x and y at most 65536");
    if (clearance && (!std::isfinite(l->step) || l->step < 0.0f)) return hu_fail(HU_ERR_BAD_ARG, "step must be finite and not negative");
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
// that drops a candidate.  The bounds of child_side and thr are each check's own: its entry point tests them after this.
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

// What a unit's allow_big_lds_* hook (host.hpp) does with its [kernel][distance_only] table: every kernel of it may take
// `bytes` of dynamic LDS.
template <class K, size_t N>
hipError_t allow_big_lds_table(void (*const (&table)[N][2])(K), size_t bytes)
{
    hipError_t e = hipSuccess;
    for (const auto& level : table)
        for (const auto variant : level)
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)variant, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

}  // namespace hu_cells
