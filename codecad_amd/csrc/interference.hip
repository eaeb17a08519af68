// codecad_amd/csrc/interference.hip
//
// Interference between the instances of an assembly (codecad_amd/interference.py): which pairs of instances have
// lattice samples inside both, how many, where.  Every instance has a tape of its own; the kernels reach them through
// a device table (InstanceRec) and evaluate them with the tape interpreter, one instance at a time, the instance
// index wave-uniform so that its records still arrive through scalar loads.
//
// The lattice is cut into cubic CELLS of side 4^k samples; a cell is a 16-byte row {x0 | y0 << 16, z0, mask lo, mask hi}:
// its first sample's indices and the 64-bit mask of the instances that may still have a sample inside it (candidates).
// One WAVEFRONT takes one cell and its 64 lanes take the cell's 4 x 4 x 4 parts, lane = 16 x + 4 y + z:
//   k_interference_cells (side > 4): a lane is a child cell; every candidate is evaluated at the child's centre and
//     dropped where its distance proves it has no sample inside the child; children with >= 2 candidates left are
//     compacted into the next list (ballots, one atomic per workgroup: kernels.hpp wg_compact_slots);
//   k_interference_leaf (side 4): a lane is a sample; every candidate is evaluated there, which gives the lane's
//     inside bitmask (w < 0, strictly), and every pair of candidates with a sample inside both adds its count, index
//     sums and index box to the pair's accumulators (one atomic per accumulator per wavefront).
// Both read their parent count from the list's header on the device (the *_indirect pattern of the other level kernels).
// The cell row, the instance table's scalar-load path and mask_box are shared with clearance.hip (instance_cells.hpp).
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  hip_util.hip validates
// arguments and calls the launch functions at the end of this file.
#include "launchers.hpp"
#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

template <bool DO>
__global__ void __launch_bounds__(256) k_interference_cells(const hu_interference::Args a)
{
    extern __shared__ float4 lds[];
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    const uint32_t s = a.child_side;
    const uint32_t x = row.x0 + (lane >> 4) * s, y = row.y0 + ((lane >> 2) & 3u) * s, z = row.z0 + (lane & 3u) * s;
    const bool live = row.have & (x < a.dims[0]) & (y < a.dims[1]) & (z < a.dims[2]);
    // the child's centre; its samples lie within (s - 1) * step * sqrt(3) / 2 of it, a.thr is more than that (interference.py)
    const float h = 0.5f * (float)(s - 1u);
    const float px = a.corner[0] + a.step * ((float)x + h);
    const float py = a.corner[1] + a.step * ((float)y + h);
    const float pz = a.corner[2] + a.step * ((float)z + h);
    uint64_t keep = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        if (!(w >= a.thr)) keep |= 1ull << n;                     // (a NaN keeps its candidate)
    }
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && __popcll(keep) >= 2};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
}

template <bool DO>
__global__ void __launch_bounds__(256) k_interference_leaf(const hu_interference::Args a)
{
    extern __shared__ float4 lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = cell_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const uint32_t lx = lane >> 4, ly = (lane >> 2) & 3u, lz = lane & 3u;
    const uint32_t x = row.x0 + lx, y = row.y0 + ly, z = row.z0 + lz;
    const bool live = (x < a.dims[0]) & (y < a.dims[1]) & (z < a.dims[2]);
    // exactly kernels.hpp sample() (the lattice of oracle.grid_eval)
    const float px = sample(a.corner[0], a.step, x), py = sample(a.corner[1], a.step, y), pz = sample(a.corner[2], a.step, z);
    uint64_t inside = 0ull, present = 0ull;                       // per lane; wave-uniform
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        const bool in = live & (w < 0.0f);
        inside |= in ? 1ull << n : 0ull;
        present |= __ballot(in) ? 1ull << n : 0ull;
    }
    const uint64_t lives = __ballot(live);
    if (lane == 0u) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    for (uint64_t mi = present; mi != 0ull; mi &= mi - 1ull) {
        const uint32_t i = uniform((uint32_t)__builtin_ctzll(mi));
        for (uint64_t mj = mi & (mi - 1ull); mj != 0ull; mj &= mj - 1ull) {
            const uint32_t j = uniform((uint32_t)__builtin_ctzll(mj));
            const bool both = ((inside >> i) & (inside >> j) & 1ull) != 0ull;
            const uint64_t b = __ballot(both);
            if (b == 0ull) continue;                              // wave-uniform
            const uint32_t sx = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? x : 0u), 63);
            const uint32_t sy = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? y : 0u), 63);
            const uint32_t sz = __builtin_amdgcn_readlane(wave_sum_to_last_lane(both ? z : 0u), 63);
            uint32_t lo[3], hi[3];
            mask_box(b, lo, hi);
            hu_interference::PairAcc* acc = a.pairs + (size_t)i * a.n_instances + j;
            // lanes 0-3: the u64 sums, 4-6: the minima, 7-9: the maxima -- each accumulator once per wavefront
            const unsigned long long add = lane == 0u ? (unsigned long long)__popcll(b) : lane == 1u ? sx : lane == 2u ? sy : sz;
            const uint32_t k = lane < 7u ? lane - 4u : lane - 7u;
            const uint32_t origin = k == 0u ? row.x0 : k == 1u ? row.y0 : row.z0;
            const uint32_t bound = origin + (lane < 7u ? (k == 0u ? lo[0] : k == 1u ? lo[1] : lo[2]) : (k == 0u ? hi[0] : k == 1u ? hi[1] : hi[2]));
            if (lane < 4u) atomicAdd(&acc->sums[lane], add);
            else if (lane < 7u) atomicMin(&acc->lo[k], bound);
            else if (lane < 10u) atomicMax(&acc->hi[k], bound);
        }
    }
}

}  // namespace

namespace hu_interference {

hipError_t allow_big_lds(size_t bytes)
{
    hipError_t e = hipSuccess;
    const void* kernels[] = {(const void*)k_interference_cells<true>, (const void*)k_interference_cells<false>,
                             (const void*)k_interference_leaf<true>, (const void*)k_interference_leaf<false>};
    for (const void* k : kernels)
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

hipError_t level(bool leaf, bool distance_only, const Args& a, uint32_t blocks, uint32_t block, size_t lds, hipStream_t stream)
{
    if (leaf) {
        if (distance_only) hipLaunchKernelGGL(k_interference_leaf<true>, dim3(blocks), dim3(block), lds, stream, a);
        else hipLaunchKernelGGL(k_interference_leaf<false>, dim3(blocks), dim3(block), lds, stream, a);
    } else {
        if (distance_only) hipLaunchKernelGGL(k_interference_cells<true>, dim3(blocks), dim3(block), lds, stream, a);
        else hipLaunchKernelGGL(k_interference_cells<false>, dim3(blocks), dim3(block), lds, stream, a);
    }
    return hipGetLastError();
}

}  // namespace hu_interference
