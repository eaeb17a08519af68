// codecad_amd/csrc/instance_thickness.hip
//
// The CAPPED SQUARED EUCLIDEAN DISTANCE TRANSFORM of a predicate on the part-id volume of an assembly, twice, for the thin
// walls of codecad_amd/thin_walls.py: transform 1 gives every sample of S its squared distance to the background, capped at
// R2 + 1 (depth_sq; the CORE E is where it reaches the cap); transform 2 gives every sample its squared distance to E, capped
// at C2 + 1, and a sample of S that reaches that cap is THIN.  All integers, exact.
//
// A transform is three PASSES, along z, then y, then x, each a capped min-plus stencil along its axis,
//     out(i) = min(cap, min over |k| <= K of in(i + k) + k * k),            K = isqrt(cap - 1) <= 255,
// over uint16[nx][ny][pitch] volumes of the pitch of the id volume.  A tap outside the lattice reads `outside`: 0 in
// transform 1 (everything outside the lattice is background), the cap in transform 2 (no core out there).  Values are at most
// 65535 and k * k at most 65025: the sum is taken in 32 bits and then capped, nothing wraps.  A lane stops tapping once
// k * k >= best (no further tap can lower it) and the wavefront leaves the loop when every lane has stopped.
//
// LANES LIE ALONG z IN EVERY PASS, so every global access of a wavefront is a run of consecutive uint16 (or id bytes):
//   k_thick_z: a wavefront takes 64 consecutive z of one (x, y) column.  It reads the ids (transform 1: in S ? cap : 0) or
//     depth_sq (transform 2: > R2 ? 0 : cap, so the core is never stored) and never a byte of the padding z in [nz, pitch):
//     z outside [0, nz) is `outside`.  LDS: the wavefront's 64 + 2 K inputs, 4 x 576 uint16 a workgroup.
//   k_thick_axis: along y a COLUMN is one z of one x (pitch columns, nx slabs), along x one (y, z) (ny * pitch columns, one
//     slab), z = column % pitch, and the columns z >= nz are neither read nor written.  A workgroup of four wavefronts takes
//     64 columns x `tile` positions along the axis; wavefront w computes the positions w, w + 4, ...  LDS: the tile's rows
//     with their halo, (tile + 2 K) x 64 uint16, at most kRows = 256 rows = 32 KiB (the host picks tile = 256 - 2 K while
//     K <= 96 and the global path above).  LDS == false reads every tap from global memory: the comparison arm, the same bytes.
//     FINISH == 1 (x pass of transform 1) also counts the core per part, FINISH == 2 (x pass of transform 2) reads the ids,
//     writes thin_ids (the id where thin, else 255; pitch as the ids) instead of distances and counts the thin samples per
//     part: lane p of a wavefront gathers the count of part p over the wavefront's rows and adds it once at the end -- one
//     atomic per accumulator and wavefront.
// No kernel has a private array or scratch.  The volume's contract: id_volume.hpp.  The entry points are at the end of this file.
#include "id_volume.hpp"

using namespace hu_cells;

namespace {

constexpr uint32_t kMaxK = HU_THICKNESS_MAX_K;
constexpr uint32_t kRows = HU_THICKNESS_LDS_ROWS;       // rows of 64 uint16 of k_thick_axis' LDS
constexpr uint32_t kSegment = 64u + 2u * kMaxK + 2u;    // k_thick_z: a wavefront's inputs, 576
static_assert(kMaxK == 255u && kRows == 256u, "include/hip_util.h");

struct ThickArgs {
    const uint8_t* ids;                 // uint8[nx][ny][pitch] (z pass of transform 1; FINISH != 0)
    const uint16_t* in;                 // uint16[nx][ny][pitch]
    uint16_t* out;
    uint8_t* thin;                      // FINISH == 2
    unsigned long long* counts;         // FINISH != 0: 64 accumulators
    uint32_t nx, ny, nz, pitch;
    uint32_t K, cap, outside;
    uint32_t r2;                        // z pass of transform 2: the core is in > r2
    uint32_t of;
    uint32_t n, tile;                   // k_thick_axis: positions along the axis, and those of a workgroup
    uint32_t columns, column_blocks;    // ... columns of a slab, and ceil(columns / 64)
    uint64_t stride, slab;              // ... elements between two positions, and between two slabs
};

// the stencil at one sample: tap(d) is in(i + d), d in [-K, K].  Wave-uniform trip count; best <= cap throughout.
template <class Tap> __device__ __forceinline__ uint32_t stencil(uint32_t K, uint32_t cap, bool active, Tap tap)
{
    uint32_t best = active ? min(cap, tap(0)) : 0u;
    for (uint32_t k = 1u; k <= K; ++k) {
        const uint32_t kk = k * k;
        const bool go = kk < best;                                   // (an inactive lane has best = 0: it never goes)
        if (__ballot(go) == 0ull) break;
        if (go) best = min(best, min(tap(-(int)k), tap((int)k)) + kk);
    }
    return best;
}

template <bool T2, bool LDS>
__global__ void __launch_bounds__(256) k_thick_z(const ThickArgs a)
{
    __shared__ uint16_t staged[LDS ? 4u * kSegment : 1u];
    const uint32_t lane = threadIdx.x & 63u, w = uniform(threadIdx.x >> 6);
    const uint32_t segments = (a.nz + 63u) >> 6;
    const uint64_t units = (uint64_t)a.nx * a.ny * segments;
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + w;
    const bool have = unit < units;                                   // wave-uniform; no return before the barrier
    const uint64_t column = have ? unit / segments : 0ull;
    const uint32_t z0 = have ? ((uint32_t)(unit - column * segments)) << 6 : 0u;
    const size_t base = (size_t)column * a.pitch;
    const uint32_t K = a.K, cap = a.cap;
    // in(z) of this column, z any integer: nothing outside [0, nz) is read
    auto input = [&](int z) -> uint32_t {
        if (z < 0 || z >= (int)a.nz) return a.outside;
        if (T2) return a.in[base + (uint32_t)z] > a.r2 ? 0u : cap;
        return in_set(a.ids[base + (uint32_t)z], a.of) ? cap : 0u;
    };
    if (LDS) {
        uint16_t* mine = staged + w * kSegment;
        if (have)
            for (uint32_t j = lane; j < 64u + 2u * K; j += 64u) mine[j] = (uint16_t)input((int)(z0 + j) - (int)K);
        __syncthreads();
    }
    const uint32_t z = z0 + lane;
    const bool active = have && z < a.nz;
    const uint32_t best = LDS ? stencil(K, cap, active, [&](int d) -> uint32_t { return staged[w * kSegment + K + lane + d]; })
                              : stencil(K, cap, active, [&](int d) -> uint32_t { return input((int)z + d); });
    if (active) a.out[base + z] = (uint16_t)best;
}

template <int FINISH, bool LDS>
__global__ void __launch_bounds__(256) k_thick_axis(const ThickArgs a)
{
    __shared__ uint16_t rows[LDS ? kRows * 64u : 1u];
    const uint32_t lane = threadIdx.x & 63u, w = uniform(threadIdx.x >> 6);
    const uint32_t slab = blockIdx.x / a.column_blocks, c = (blockIdx.x - slab * a.column_blocks) * 64u + lane;
    const uint32_t z = c % a.pitch;
    const bool active = c < a.columns && z < a.nz;                    // (the padding is neither read nor written)
    const uint32_t first = blockIdx.y * a.tile;                       // < n
    const uint32_t count = min(a.tile, a.n - first);
    const size_t base = (size_t)slab * a.slab + c;
    const uint32_t K = a.K, cap = a.cap;
    auto input = [&](int i) -> uint32_t {                             // in(position i) of this column
        return (i < 0 || i >= (int)a.n) ? a.outside : (uint32_t)a.in[base + (size_t)(uint32_t)i * a.stride];
    };
    if (LDS) {                                                        // count + 2 K <= tile + 2 K <= kRows
        for (uint32_t r = w; r < count + 2u * K; r += 4u) rows[r * 64u + lane] = active ? (uint16_t)input((int)(first + r) - (int)K) : (uint16_t)0u;
        __syncthreads();
    }
    unsigned long long mine = 0ull;
    for (uint32_t r = w; r < count; r += 4u) {                        // wave-uniform
        const uint32_t i = first + r;
        const uint32_t best = LDS ? stencil(K, cap, active, [&](int d) -> uint32_t { return rows[(uint32_t)((int)(r + K) + d) * 64u + lane]; })
                                  : stencil(K, cap, active, [&](int d) -> uint32_t { return input((int)i + d); });
        const size_t at = base + (size_t)i * a.stride;
        if (FINISH == 0) {
            if (active) a.out[at] = (uint16_t)best;
        } else {
            const uint32_t id = active ? a.ids[at] : kEmpty;
            // 1: best is depth_sq, the core is where it reaches the cap R2 + 1 >= 1 (outside S it is 0)
            // 2: best is the capped distance to the core: a sample of S that reaches the cap C2 + 1 is thin
            // (an empty sample reaches the cap only on inputs no transform makes; it is nobody's, not part 63's)
            const bool counted = active && best == cap && (FINISH == 1 ? id != kEmpty : in_set(id, a.of));
            if (FINISH == 1) {
                if (active) a.out[at] = (uint16_t)best;
            } else {
                if (active) a.thin[at] = (uint8_t)(counted ? id : kEmpty);
            }
            gather_counts(counted, id, lane, mine);
        }
    }
    if (FINISH != 0 && mine != 0ull) atomicAdd(&a.counts[lane], mine);
}

int thick_args(const uint32_t dims[3], uint32_t pitch, uint32_t K, uint32_t cap, uint32_t of, ThickArgs& a)
{
    a = ThickArgs{};
    if (!dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (int rc = lattice_of(dims, pitch, a)) return rc;
    if (cap > 65535u) return hu_fail(HU_ERR_BAD_ARG, "cap must be at most 65535");
    if (K > kMaxK) return hu_fail(HU_ERR_BAD_ARG, "K must be at most 255");
    if (int rc = check_of(of, "HU_THICKNESS_SOLID")) return rc;
    a.K = K, a.cap = cap, a.of = of;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_thickness_pass_z(const void* ids_dev, const void* depth_dev, void* out_dev, const uint32_t dims[3], uint32_t pitch,
                        uint32_t of, uint32_t radius_sq, uint32_t K, uint32_t cap, int lds, void* stream)
{
    ThickArgs a;
    int rc;
    if ((rc = thick_args(dims, pitch, K, cap, of, a))) return rc;
    if (!out_dev || (!ids_dev && !depth_dev)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(out_dev) % 2u || reinterpret_cast<uintptr_t>(depth_dev) % 2u)
        return hu_fail(HU_ERR_BAD_ARG, "distance volumes must be aligned to 2 bytes");
    const bool second = depth_dev != nullptr;                        // transform 2 reads depth_sq, transform 1 the ids
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.in = static_cast<const uint16_t*>(depth_dev);
    a.out = static_cast<uint16_t*>(out_dev);
    a.r2 = radius_sq;
    a.outside = second ? cap : 0u;
    const uint64_t units = (uint64_t)a.nx * a.ny * ((a.nz + 63u) / 64u), blocks = (units + 3u) / 4u;
    if (blocks > 0x7fffffffull) return hu_fail(HU_ERR_BAD_ARG, "lattice too large for one launch");
    const dim3 grid((uint32_t)blocks), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (second && lds) hipLaunchKernelGGL((k_thick_z<true, true>), grid, block, 0, s, a);
    else if (second) hipLaunchKernelGGL((k_thick_z<true, false>), grid, block, 0, s, a);
    else if (lds) hipLaunchKernelGGL((k_thick_z<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_thick_z<false, false>), grid, block, 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_thickness_pass_axis(const void* in_dev, void* out_dev, const void* ids_dev, void* thin_dev, uint64_t* counts_dev,
                           const uint32_t dims[3], uint32_t pitch, int axis, uint32_t of, uint32_t K, uint32_t cap,
                           uint32_t outside, int finish, uint32_t tile, int lds, void* stream)
{
    ThickArgs a;
    int rc;
    if ((rc = thick_args(dims, pitch, K, cap, of, a))) return rc;
    if (axis != 0 && axis != 1) return hu_fail(HU_ERR_BAD_ARG, "axis must be 0 (x) or 1 (y)");
    if (finish < 0 || finish > 2) return hu_fail(HU_ERR_BAD_ARG, "finish must be 0, 1 or 2");
    if (!in_dev || (finish != 2 && !out_dev) || (finish != 0 && (!ids_dev || !counts_dev)) || (finish == 2 && !thin_dev))
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(in_dev) % 2u || reinterpret_cast<uintptr_t>(out_dev) % 2u ||
        reinterpret_cast<uintptr_t>(counts_dev) % 8u)
        return hu_fail(HU_ERR_BAD_ARG, "distance volumes must be aligned to 2 bytes, the counts to 8");
    if (outside > cap) return hu_fail(HU_ERR_BAD_ARG, "outside must be at most cap");
    if (tile == 0u || tile > 65536u) return hu_fail(HU_ERR_BAD_ARG, "tile must be in 1..65536");
    if (lds && tile + 2u * K > kRows) return hu_fail(HU_ERR_BAD_ARG, "tile + 2 K must be at most HU_THICKNESS_LDS_ROWS with lds");
    a.in = static_cast<const uint16_t*>(in_dev);
    a.out = static_cast<uint16_t*>(out_dev);
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.thin = static_cast<uint8_t*>(thin_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    a.outside = outside;
    a.tile = tile;
    uint64_t slabs;
    if (axis == 1) {
        a.n = a.ny, a.stride = pitch, a.columns = pitch, a.slab = (uint64_t)a.ny * pitch, slabs = a.nx;
    } else {
        const uint64_t columns = (uint64_t)a.ny * pitch;
        if (columns > 0xffffffc0ull) return hu_fail(HU_ERR_BAD_ARG, "lattice too large for one launch");
        a.n = a.nx, a.stride = columns, a.columns = (uint32_t)columns, a.slab = 0u, slabs = 1u;
    }
    a.column_blocks = (a.columns + 63u) / 64u;
    const uint64_t gx = slabs * a.column_blocks, gy = (a.n + tile - 1u) / tile;
    if (gx > 0x7fffffffull || gy > 65535u) return hu_fail(HU_ERR_BAD_ARG, "lattice too large for one launch");
    const dim3 grid((uint32_t)gx, (uint32_t)gy), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (finish == 0 && lds) hipLaunchKernelGGL((k_thick_axis<0, true>), grid, block, 0, s, a);
    else if (finish == 0) hipLaunchKernelGGL((k_thick_axis<0, false>), grid, block, 0, s, a);
    else if (finish == 1 && lds) hipLaunchKernelGGL((k_thick_axis<1, true>), grid, block, 0, s, a);
    else if (finish == 1) hipLaunchKernelGGL((k_thick_axis<1, false>), grid, block, 0, s, a);
    else if (lds) hipLaunchKernelGGL((k_thick_axis<2, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_thick_axis<2, false>), grid, block, 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
