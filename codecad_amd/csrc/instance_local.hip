// codecad_amd/csrc/instance_local.hip
//
// THE LOCAL THICKNESS of a uint16 field on the part-id volume of an assembly, for codecad_amd/wall_thickness.py: every sample
// takes the greatest value of a ball that contains it,
//     out(p) = max{ in(q) : q in the lattice, |p - q|^2 < in(q) }      for p in S with in(p) > 0,      out(p) = 0 elsewhere,
// where in(q) counts as 0 outside S, outside the lattice and in the padding z in [nz, pitch), whatever is stored there, and is
// at most cap = radius_sq + 1 <= 1025 (the caller's to ensure).  q = p always qualifies, so out >= in on those samples.  With
// in = the capped squared distance to the background (depth_sq of instance_thickness.hip) out is the greatest capped inscribed
// ball over a sample.  This step is not separable: a dense 3D gather with a radius the data decide.  All integers, exact.
//
// k_thick_local<HALO, THREADS>: a workgroup takes one TILE of 8 x 8 x 16 samples (HU_COMPONENTS_TILE_*), lanes along z, a
// wavefront a slab of 4 y x 16 z of one x at a time.
//   1. It reads the tile and a halo of K = isqrt(radius_sq) around it -- the ids and the field, zeros where the field does not
//      count -- and reduces the greatest value M.  While K <= HALO the values go to LDS as they are read.
//   2. No ball reaches further than |p - q|^2 <= M - 1: the search shrinks to r2e = min(radius_sq, M - 1), ke = isqrt(r2e), for the
//      whole workgroup, and no sample can read more than top = min(M, cap).  M == 0: zeros are written and the workgroup leaves.
//      Where K > HALO >= ke the tile is staged now, with a halo of ke: a sheet costs what its thickness costs, not what K costs.
//   3. The gather walks dx = 0, 1, -1, 2, ..., dy likewise within the disc, dz in [-h, h], h = isqrt(r2e - dx^2 - dy^2): one
//      read, one compare and one max per tap, from LDS when staged, else from global memory (two loads and the bounds).  A lane
//      is FINISHED when it holds `top`; before every column of dz a ballot lets the wavefront leave when all its lanes are.
//   4. Per part: lane p of a wavefront gathers the least key L << 48 | x << 32 | y << 16 | z and the samples with L == cap of
//      part p over everything the wavefront computes, and issues one atomicMin and one atomicAdd at the end.
// HALO = 0 is the comparison arm: no LDS, every tap from global memory, the same bytes.  HALO = 4, 10, 16 hold kLdsBytes(HALO)
// of LDS with 256, 512, 1024 threads (4, 8, 16 wavefronts a workgroup, where id_volume.hpp's other kernels have four): the
// wavefronts a compute unit holds stay near 16 to 32 as the tile's footprint grows.
// No kernel has a private array or scratch.  The volume's contract: id_volume.hpp.  The entry point is at the end of this file.
#include "id_volume.hpp"

using namespace hu_cells;

namespace {

constexpr uint32_t kMaxRadius = HU_LOCAL_MAX_RADIUS_SQ;
constexpr uint32_t kTX = HU_COMPONENTS_TILE_X, kTY = HU_COMPONENTS_TILE_Y, kTZ = HU_COMPONENTS_TILE_Z;
constexpr uint32_t kTile = kTX * kTY * kTZ;
constexpr uint32_t kMaxHalo = HU_LOCAL_LDS_K;
constexpr uint32_t window(uint32_t halo) { return (kTX + 2u * halo) * (kTY + 2u * halo) * (kTZ + 2u * halo); }
constexpr uint32_t kLdsBytes(uint32_t halo, uint32_t threads) { return (halo ? window(halo) * 2u : 0u) + threads / 64u * 4u; }
static_assert(kMaxRadius == 1024u && kTile == 1024u && kTZ == 16u && kTY == 8u, "include/hip_util.h");
static_assert(kLdsBytes(kMaxHalo, 1024u) == HU_LOCAL_LDS_BYTES && HU_LOCAL_LDS_BYTES <= 160u * 1024u, "include/hip_util.h");

struct LocalArgs {
    const uint16_t* in;                 // uint16[nx][ny][pitch]
    const uint8_t* ids;                 // uint8[nx][ny][pitch]
    uint16_t* out;
    unsigned long long* keys;           // 64: lowered
    unsigned long long* counts;         // 64: the samples that read the cap
    uint32_t nx, ny, nz, pitch;
    uint32_t of, r2, K;
};

// in(q) as it counts, q any point of Z^3: nothing outside the lattice or in the padding is read
__device__ __forceinline__ uint32_t value_at(const LocalArgs& a, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= (int)a.nx || y >= (int)a.ny || z >= (int)a.nz) return 0u;
    const size_t at = ((size_t)(uint32_t)x * a.ny + (uint32_t)y) * a.pitch + (uint32_t)z;
    return in_set(a.ids[at], a.of) ? (uint32_t)a.in[at] : 0u;
}

// the window of the tile at (x0, y0, z0) with a halo of H, z fastest: its greatest value over this thread's entries; STORE
// writes the entries to `tile` as well
template <bool STORE>
__device__ __forceinline__ uint32_t read_window(const LocalArgs& a, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t H, uint16_t* tile)
{
    const uint32_t wy = kTY + 2u * H, wz = kTZ + 2u * H, total = (kTX + 2u * H) * wy * wz;
    uint32_t m = 0u;
    for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
        const uint32_t r = i / wz, rz = i - r * wz, rx = r / wy, ry = r - rx * wy;
        const uint32_t v = value_at(a, (int)(x0 + rx) - (int)H, (int)(y0 + ry) - (int)H, (int)(z0 + rz) - (int)H);
        if (STORE) tile[i] = (uint16_t)v;
        m = max(m, v);
    }
    return m;
}

// the greatest `m` of the workgroup (wave-uniform); holds a barrier, after which the staged window may be read
__device__ __forceinline__ uint32_t block_max(uint32_t m, uint32_t* slots)
{
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63u) == 0u) slots[threadIdx.x >> 6] = m;
    __syncthreads();
    uint32_t all = 0u;
    for (uint32_t w = 0u; w < (blockDim.x >> 6); ++w) all = max(all, slots[w]);
    return uniform(all);
}

// the greatest v with v * v <= n, from a start not below it (wave-uniform)
__device__ __forceinline__ uint32_t lower_to_root(uint32_t from, uint32_t n)
{
    while (from * from > n) --from;
    return from;
}

// j = 0, 1, 2, 3, 4, ... -> 0, 1, -1, 2, -2, ...: the near offsets first, so that a lane meets `top` early
__device__ __forceinline__ int outward(uint32_t j) { return (j & 1u) ? (int)((j + 1u) >> 1) : -(int)(j >> 1); }

// the gather of one sample a lane: tap(dx, dy, dz) is in(p + d) as it counts, `own` in(p).  r2e, ke, top: wave-uniform.
template <class Tap>
__device__ __forceinline__ uint32_t gather(uint32_t own, uint32_t top, uint32_t r2e, uint32_t ke, Tap tap)
{
    uint32_t best = own;
    bool open = own != 0u && best < top;                               // (a sample that does not count searches nothing)
    uint32_t reach_y = ke;
    for (uint32_t j = 0u; j <= 2u * ke; ++j) {                         // wave-uniform
        const int dx = outward(j);
        const uint32_t left_x = r2e - (uint32_t)(dx * dx);
        reach_y = lower_to_root(reach_y, left_x);
        uint32_t h = reach_y;
        for (uint32_t i = 0u; i <= 2u * reach_y; ++i) {
            const int dy = outward(i);
            const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);
            h = lower_to_root(h, r2e - d2);
            if (__ballot(open) == 0ull) return best;
            for (int dz = -(int)h; dz <= (int)h; ++dz) {
                const uint32_t v = tap(dx, dy, dz);
                if (v > d2 + (uint32_t)(dz * dz)) best = max(best, v);
            }
            open = open && best < top;
        }
    }
    return best;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long k)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(k, off);
        k = other < k ? other : k;
    }
    return k;
}

template <uint32_t HALO, uint32_t THREADS>
__global__ void __launch_bounds__(THREADS) k_thick_local(const LocalArgs a)
{
    __shared__ uint16_t tile[HALO ? window(HALO) : 1u];
    __shared__ uint32_t slots[THREADS / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x0 = blockIdx.z * kTX, y0 = blockIdx.y * kTY, z0 = blockIdx.x * kTZ;
    const uint32_t K = a.K, cap = a.r2 + 1u;
    bool staged = HALO != 0u && K <= HALO;                             // uniform over the workgroup
    uint32_t H = K;
    const uint32_t M = block_max(staged ? read_window<true>(a, x0, y0, z0, K, tile) : read_window<false>(a, x0, y0, z0, K, tile), slots);
    if (M == 0u) {                                                     // nothing counts in reach of the tile
        for (uint32_t s = threadIdx.x; s < kTile; s += THREADS) {
            const uint32_t x = x0 + (s >> 7), y = y0 + ((s >> 4) & 7u), z = z0 + (s & 15u);
            if (x < a.nx && y < a.ny && z < a.nz) a.out[((size_t)x * a.ny + y) * a.pitch + z] = (uint16_t)0u;
        }
        return;
    }
    const uint32_t r2e = min(a.r2, M - 1u), ke = lower_to_root(K, r2e), top = min(M, cap);
    if (HALO != 0u && !staged && ke <= HALO) {                         // a wide K over a thin tile: the halo that matters fits
        read_window<true>(a, x0, y0, z0, ke, tile);
        __syncthreads();
        staged = true, H = ke;
    }
    const uint32_t wy = kTY + 2u * H, wz = kTZ + 2u * H;
    unsigned long long least = ~0ull, capped = 0ull;
    for (uint32_t s = threadIdx.x; s < kTile; s += THREADS) {           // a wavefront: 4 y x 16 z of one x
        const uint32_t lx = s >> 7, ly = (s >> 4) & 7u, lz = s & 15u;
        const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
        const bool inside = x < a.nx && y < a.ny && z < a.nz;
        const size_t at = ((size_t)x * a.ny + y) * a.pitch + z;
        uint32_t own, L;
        if (HALO != 0u && staged) {
            const uint16_t* centre = tile + ((lx + H) * wy + ly + H) * wz + lz + H;
            own = *centre;                                             // (0 outside the lattice)
            L = gather(own, top, r2e, ke, [&](int dx, int dy, int dz) -> uint32_t { return centre[(dx * (int)wy + dy) * (int)wz + dz]; });
        } else {
            own = value_at(a, (int)x, (int)y, (int)z);
            L = gather(own, top, r2e, ke, [&](int dx, int dy, int dz) -> uint32_t { return value_at(a, (int)x + dx, (int)y + dy, (int)z + dz); });
        }
        if (own == 0u) L = 0u;
        if (inside) a.out[at] = (uint16_t)L;
        const uint32_t id = L != 0u ? a.ids[at] : kEmpty;              // (L != 0: inside, and in S)
        const bool counted = id < 64u;
        const unsigned long long key = (unsigned long long)L << 48 | (unsigned long long)x << 32 | (unsigned long long)y << 16 | z;
        for (uint64_t todo = __ballot(counted); todo != 0ull;) {       // wave-uniform: every part present
            const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)__builtin_ctzll(todo));
            const bool mine = counted && id == p;
            todo &= ~__ballot(mine);
            const unsigned long long k = wave_min(mine ? key : ~0ull);
            const unsigned long long c = (unsigned long long)__popcll(__ballot(mine && L == cap));
            if (lane == p) least = k < least ? k : least, capped += c;
        }
    }
    if (least != ~0ull) atomicMin(&a.keys[lane], least);
    if (capped != 0ull) atomicAdd(&a.counts[lane], capped);
}

bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0u; }

}  // namespace

extern "C" {

int hu_thickness_local(const void* depth_dev, const void* ids_dev, void* out_dev, uint64_t* keys_dev, uint64_t* counts_dev,
                       const uint32_t dims[3], uint32_t pitch, uint32_t of, uint32_t radius_sq, int lds, void* stream)
{
    LocalArgs a{};
    if (!depth_dev || !ids_dev || !out_dev || !keys_dev || !counts_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    int rc;
    if ((rc = lattice_of(dims, pitch, a)) || (rc = check_of(of, "HU_THICKNESS_SOLID"))) return rc;
    if (radius_sq > kMaxRadius) return hu_fail(HU_ERR_BAD_ARG, "radius_sq must be at most 1024");
    if (misaligned(depth_dev, 2u) || misaligned(out_dev, 2u)) return hu_fail(HU_ERR_BAD_ARG, "distance volumes must be aligned to 2 bytes");
    if (misaligned(keys_dev, 8u) || misaligned(counts_dev, 8u)) return hu_fail(HU_ERR_BAD_ARG, "the keys and the counts must be aligned to 8 bytes");
    if (depth_dev == out_dev) return hu_fail(HU_ERR_BAD_ARG, "in and out must not overlap");
    a.in = static_cast<const uint16_t*>(depth_dev);
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.out = static_cast<uint16_t*>(out_dev);
    a.keys = reinterpret_cast<unsigned long long*>(keys_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    a.of = of, a.r2 = radius_sq;
    while ((a.K + 1u) * (a.K + 1u) <= radius_sq) ++a.K;
    // tiles: at most 4096 x 8192 x 8192
    const dim3 grid((a.nz + kTZ - 1u) / kTZ, (a.ny + kTY - 1u) / kTY, (a.nx + kTX - 1u) / kTX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!lds) hipLaunchKernelGGL((k_thick_local<0u, 256u>), grid, dim3(256), 0, s, a);
    else if (a.K <= 4u) hipLaunchKernelGGL((k_thick_local<4u, 256u>), grid, dim3(256), 0, s, a);
    else if (a.K <= 10u) hipLaunchKernelGGL((k_thick_local<10u, 512u>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((k_thick_local<kMaxHalo, 1024u>), grid, dim3(1024), 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
