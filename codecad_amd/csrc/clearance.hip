// codecad_amd/csrc/clearance.hip
//
// Clearance between the instances of an assembly (codecad_amd/clearance.py): which pairs of instances come closer than
// a gap, and where.  The traversal is interference.hip's with a threshold t > 0 instead of 0: cells of 4^k samples with a
// 64-bit candidate mask (instance_cells.hpp), one wavefront per cell, every instance's tape reached through the device
// table.  A sample is NEAR the pair (i, j) when it lies in both instances' windows (index boxes the host computes) and
// w_i < t, w_j < t; there v = max(w_i, w_j).
//   k_clearance_cells (side > 4): a lane is a child cell; a candidate leaves it when the child misses its window or its
//     distance at the child's centre is >= thr (clearance.py); children with >= 2 candidates left are compacted into
//     the next list (kernels.hpp wg_compact_slots);
//   k_clearance_leaf (side 4): a lane is a sample; every candidate is evaluated there into the wavefront's LDS area,
//     [instance][lane], which gives the lane's near bitmask; every pair with near lanes adds its count, index sums, index
//     box and the least order key of v to its accumulators (one atomic per accumulator per wavefront);
//   k_clearance_witness (side 4), launched after the leaf over the same list: evaluates again and, for every pair, its
//     first lane whose v has the pair's final least key gives one u64 atomicMin of x << 32 | y << 16 | z.  Lanes go
//     16 x + 4 y + z, so the wavefront's first such lane is its lexicographically smallest sample.
// All read their parent count from the list's header on the device.  Built WITHOUT -structurizecfg-skip-uniform-regions
// (hip_util/builder.py FLAGGED_SOURCES).  hip_util.hip validates arguments and calls the launch functions at the end.
#include "launchers.hpp"
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// the key of v in an order that unsigned comparison keeps: -0 and +0 get the one key of +0 (clearance.py decodes it)
__device__ __forceinline__ uint32_t order_key(float v)
{
    const uint32_t b = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
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

template <bool DO>
__global__ void __launch_bounds__(256) k_clearance_cells(const hu_clearance::Args a)
{
    extern __shared__ float4 lds[];
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    const uint32_t x = row.x0 + (lane >> 4) * s, y = row.y0 + ((lane >> 2) & 3u) * s, z = row.z0 + (lane & 3u) * s;
    const bool live = row.have & (x < a.dims[0]) & (y < a.dims[1]) & (z < a.dims[2]);
    // the child's centre; its samples lie within (s - 1) * step * sqrt(3) / 2 of it, a.thr is t plus more than that
    const float h = 0.5f * (float)(s - 1u);
    const float px = a.corner[0] + a.step * ((float)x + h);
    const float py = a.corner[1] + a.step * ((float)y + h);
    const float pz = a.corner[2] + a.step * ((float)z + h);
    const uint32_t* windows = constant_uniform(a.windows);
    uint64_t keep = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool reach = (x <= win[3]) & (x + s - 1u >= win[0]) & (y <= win[4]) & (y + s - 1u >= win[1]) &
                           (z <= win[5]) & (z + s - 1u >= win[2]);
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        if (reach && !(w >= a.thr)) keep |= 1ull << n;            // (a NaN keeps its candidate)
    }
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && __popcll(keep) >= 2};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
}

// the sample of a finest cell this lane takes, and the wavefront's part of the w area (after the register file)
struct LeafLane {
    uint32_t lane, x, y, z;
    bool live;
    float* wl;
};
__device__ __forceinline__ LeafLane leaf_lane(const hu_clearance::Args& a, const CellRow& row)
{
    extern __shared__ float4 lds[];
    LeafLane l;
    l.lane = threadIdx.x & 63u;
    l.x = row.x0 + (l.lane >> 4);
    l.y = row.y0 + ((l.lane >> 2) & 3u);
    l.z = row.z0 + (l.lane & 3u);
    l.live = (l.x < a.dims[0]) & (l.y < a.dims[1]) & (l.z < a.dims[2]);
    l.wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 64u * a.n_instances;
    return l;
}

// every candidate evaluated at the lane's sample, w into the wavefront's LDS area at wl[n * 64 + lane]; returns the
// lane's near bitmask (in n's window and w < t, strictly: a NaN is never near)
template <bool DO>
__device__ __forceinline__ uint64_t near_mask(const hu_clearance::Args& a, const CellRow& row, const LeafLane& l)
{
    extern __shared__ float4 lds[];
    // exactly kernels.hpp sample() (the lattice of oracle.grid_eval)
    const float px = sample(a.corner[0], a.step, l.x), py = sample(a.corner[1], a.step, l.y), pz = sample(a.corner[2], a.step, l.z);
    const uint32_t* windows = constant_uniform(a.windows);
    uint64_t near = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool in = l.live & (l.x >= win[0]) & (l.x <= win[3]) & (l.y >= win[1]) & (l.y <= win[4]) & (l.z >= win[2]) &
                        (l.z <= win[5]);
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        l.wl[n * 64u + l.lane] = w;
        near |= (in & (w < a.t)) ? 1ull << n : 0ull;
    }
    const uint64_t lives = __ballot(l.live);
    if (l.lane == 0u) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    return near;
}

// the instances with a near lane (wave-uniform)
__device__ __forceinline__ uint64_t present_of(uint64_t near, uint64_t mask)
{
    uint64_t present = 0ull;
    for (uint64_t m = mask; m != 0ull; m &= m - 1ull) {
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        present |= __ballot((near >> n) & 1ull) ? 1ull << n : 0ull;
    }
    return present;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_clearance_leaf(const hu_clearance::Args a)
{
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    const uint64_t near = near_mask<DO>(a, row, l);
    const uint64_t present = present_of(near, row.mask);
    const uint32_t lane = l.lane;
    for (uint64_t mi = present; mi != 0ull; mi &= mi - 1ull) {
        const uint32_t i = uniform((uint32_t)__builtin_ctzll(mi));
        for (uint64_t mj = mi & (mi - 1ull); mj != 0ull; mj &= mj - 1ull) {
            const uint32_t j = uniform((uint32_t)__builtin_ctzll(mj));
            const bool both = ((near >> i) & (near >> j) & 1ull) != 0ull;
            const uint64_t b = __ballot(both);
            if (b == 0ull) continue;                              // wave-uniform
            const uint32_t key = both ? order_key(fmaxf(l.wl[i * 64u + lane], l.wl[j * 64u + lane])) : 0xffffffffu;
            const uint32_t kmin = __builtin_amdgcn_readlane(wave_min_to_last_lane(key), 63);
            const uint32_t sx = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? l.x : 0u), 63);
            const uint32_t sy = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? l.y : 0u), 63);
            const uint32_t sz = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? l.z : 0u), 63);
            uint32_t lo[3], hi[3];
            mask_box(b, lo, hi);
            hu_clearance::PairAcc* acc = a.pairs + (size_t)i * a.n_instances + j;
            // lanes 0-3: the u64 sums, 4-6: the minima, 7-9: the maxima, 10: the least key -- each once per wavefront
            const unsigned long long add = lane == 0u ? (unsigned long long)__popcll(b) : lane == 1u ? sx : lane == 2u ? sy : sz;
            const uint32_t k = lane < 7u ? lane - 4u : lane - 7u;
            const uint32_t origin = k == 0u ? row.x0 : k == 1u ? row.y0 : row.z0;
            const uint32_t bound = origin + (lane < 7u ? (k == 0u ? lo[0] : k == 1u ? lo[1] : lo[2]) : (k == 0u ? hi[0] : k == 1u ? hi[1] : hi[2]));
            if (lane < 4u) atomicAdd(&acc->sums[lane], add);
            else if (lane < 7u) atomicMin(&acc->lo[k], bound);
            else if (lane < 10u) atomicMax(&acc->hi[k], bound);
            else if (lane == 10u) atomicMin(&acc->key, kmin);
        }
    }
}

template <bool DO>
__global__ void __launch_bounds__(256) k_clearance_witness(const hu_clearance::Args a)
{
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const LeafLane l = leaf_lane(a, row);
    const uint64_t near = near_mask<DO>(a, row, l);
    const uint64_t present = present_of(near, row.mask);
    for (uint64_t mi = present; mi != 0ull; mi &= mi - 1ull) {
        const uint32_t i = uniform((uint32_t)__builtin_ctzll(mi));
        for (uint64_t mj = mi & (mi - 1ull); mj != 0ull; mj &= mj - 1ull) {
            const uint32_t j = uniform((uint32_t)__builtin_ctzll(mj));
            const bool both = ((near >> i) & (near >> j) & 1ull) != 0ull;
            if (__ballot(both) == 0ull) continue;                 // wave-uniform
            hu_clearance::PairAcc* acc = a.pairs + (size_t)i * a.n_instances + j;
            // the leaf launch has finished: the least key is final, and this kernel never writes it (a scalar load)
            const uint32_t kmin = *constant_uniform(&acc->key);
            const uint64_t b = __ballot(both && order_key(fmaxf(l.wl[i * 64u + l.lane], l.wl[j * 64u + l.lane])) == kmin);
            if (b != 0ull && l.lane == (uint32_t)__builtin_ctzll(b))
                atomicMin(&acc->witness, ((unsigned long long)l.x << 32) | ((unsigned long long)l.y << 16) | l.z);
        }
    }
}

}  // namespace

namespace hu_clearance {

hipError_t allow_big_lds(size_t bytes)
{
    hipError_t e = hipSuccess;
    const void* kernels[] = {(const void*)k_clearance_cells<true>, (const void*)k_clearance_cells<false>,
                             (const void*)k_clearance_leaf<true>, (const void*)k_clearance_leaf<false>,
                             (const void*)k_clearance_witness<true>, (const void*)k_clearance_witness<false>};
    for (const void* k : kernels)
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

hipError_t level(Kernel kernel, bool distance_only, const Args& a, uint32_t blocks, uint32_t block, size_t lds, hipStream_t stream)
{
    if (kernel == kCells) {
        if (distance_only) hipLaunchKernelGGL(k_clearance_cells<true>, dim3(blocks), dim3(block), lds, stream, a);
        else hipLaunchKernelGGL(k_clearance_cells<false>, dim3(blocks), dim3(block), lds, stream, a);
    } else if (kernel == kLeaf) {
        if (distance_only) hipLaunchKernelGGL(k_clearance_leaf<true>, dim3(blocks), dim3(block), lds, stream, a);
        else hipLaunchKernelGGL(k_clearance_leaf<false>, dim3(blocks), dim3(block), lds, stream, a);
    } else {
        if (distance_only) hipLaunchKernelGGL(k_clearance_witness<true>, dim3(blocks), dim3(block), lds, stream, a);
        else hipLaunchKernelGGL(k_clearance_witness<false>, dim3(blocks), dim3(block), lds, stream, a);
    }
    return hipGetLastError();
}

}  // namespace hu_clearance
