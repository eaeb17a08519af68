// codecad_amd/csrc/instance_geodesic.hip
//
// SHORTEST PATHS INSIDE A SET of the part-id volume of an assembly (codecad_amd/flow_length.py): the geodesic distance in
// 6-steps from a seed set, by a min-plus relaxation that is repeated until it changes nothing.
// S is a set of samples of the lattice given by a predicate on the id (in_geo below: in_set of id_volume.hpp, and this unit's own
// code kVoid for the samples inside no part); a STEP joins two 6-neighbours that are both in S; nothing outside the lattice is in
// S.  dist is uint32[nx][ny][pitch] beside the ids: d(p), the least number of steps from a seed to p, kNone on a sample of S no
// seed reaches.  ENTRIES OUTSIDE S ARE NEITHER READ AS DATA NOR WRITTEN by the sweeps (the seed writes kNone there once), and no
// byte of the padding z in [nz, pitch) of either volume is read or written.  All integers, exact, and independent of the order
// in which anything ran: values only ever fall, and the fixed point of d(p) = min(d(p), d(q) + 1) over the steps (p, q) with the
// seeds at 0 is the distance.  At most 2^31 entries: an entry's buffer index q = (x * ny + y) * pitch + z is 32-bit, here and in
// the keys.
//
// THE KERNELS, one argument record (GeoArgs):
//   1 k_geo_seed writes EVERY in-lattice entry of dist: 0 on a seed in S, kNone elsewhere.  The seeds are the samples of S at the
//     lattice's border (kBorder), in one layer of an axis (kLayer), or none (kList), and then k_geo_seed_list, a lane a listed
//     sample, stores 0 on those in S: the same stream, so after the fill.
//   2 k_geo_sweep_lines / k_geo_sweep_columns, one SWEEP a launch: along every line of the axis a forward walk and then a
//     backward walk of the whole line.  The carry c is kNone at the start and after a sample outside S; on a sample of S
//     v = min(dist, c + 1 saturating at kNone), stored where it is lower than dist, and then c = v.  Lines of one axis share no
//     entry, so a launch is race-free and its bytes are those of the plain walk whatever the schedule.  *word becomes nonzero
//     when any entry was lowered: at most one store per wavefront.
//     lines (axis 0 or 1): a wavefront owns 64 consecutive z of one line (line_unit of id_volume.hpp), the carry is a register
//     per lane, rows are coalesced 256 bytes; kBatch layers of ids and then of dist are in flight -- the loads do not depend on
//     the carry, only the chain of minima does.
//     columns (axis 2): a wavefront owns a column, one word of 64 samples at a time; inside a word a walk is a SEGMENTED MIN-PLUS
//     SCAN across the lanes in six steps: the ballot of S says where the lane's run starts, step s takes the value s lanes back
//     plus s where that lane is in the run, and the carry from the word before reaches the lanes of the run that starts the word.
//     First up the words, then down them (the same scan with the lanes mirrored).
//   3 k_geo_stats: per part (the id; slot 64 under kVoid) the reached samples, the unreached ones of S, the sum of d, and the key
//     (d + 1) << 32 | (0xffffffff - q) raised by a 64-bit atomic maximum: the greatest finite d and the first sample that has
//     it.  Gathered per wavefront as gather_counts does: lane p keeps part p's, one atomic per accumulator, wavefront and part.
// No kernel has a private array, scratch or LDS (the batches are unrolled: registers).  Entry points: at the end.
#include "id_volume.hpp"

using namespace hu_cells;

namespace {

constexpr uint32_t kNone = HU_GEODESIC_NONE;            // d of a sample no seed reaches, and of every sample outside S
constexpr uint32_t kVoid = HU_GEODESIC_EMPTY;           // of: S is id == 255 (in_set keeps its own two codes)
constexpr uint32_t kBorder = HU_GEODESIC_BORDER, kLayer = HU_GEODESIC_LAYER, kList = HU_GEODESIC_LIST;
constexpr uint32_t kBatch = 4u;                         // layers a lane of the walks along x and y has in flight
static_assert(kVoid != kSolid && kVoid > 63u && HU_GEODESIC_SOLID == kSolid && HU_GEODESIC_SLOTS == 65, "include/hip_util.h");

struct GeoArgs {
    const uint8_t* ids;                 // uint8[nx][ny][pitch]
    uint32_t* dist;                     // uint32[nx][ny][pitch]
    uint32_t* word;                     // the sweeps: *changed
    const uint32_t* samples;            // k_geo_seed_list: uint32[n_samples][3]
    unsigned long long* keys;           // k_geo_stats: 65
    unsigned long long* counts;         // k_geo_stats: 3 x 65
    uint32_t nx, ny, nz, pitch;
    uint32_t axis, of;
    uint32_t mode, layer, n_samples;    // the seeds
    uint32_t na;                        // dims[axis]
    uint32_t segments;                  // ceil(nz / 64)
};

__device__ __forceinline__ bool in_geo(uint32_t id, uint32_t of) { return of == kVoid ? id == kEmpty : in_set(id, of); }

// c + s, saturating at kNone (kNone itself stays: no carry)
__device__ __forceinline__ uint32_t step_on(uint32_t c, uint32_t s) { return c > kNone - s ? kNone : c + s; }

// ---- stage 1: the seeds -------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_geo_seed(const GeoArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny * a.segments) {
        const ColumnUnit u = column_unit(a, unit);
        const uint32_t z = u.z0 + lane;
        if (z >= a.nz) continue;                                              // (the padding: nothing)
        bool seed = false;
        if (a.mode == kBorder)
            seed = u.x == 0u || u.x == a.nx - 1u || u.y == 0u || u.y == a.ny - 1u || z == 0u || z == a.nz - 1u;
        else if (a.mode == kLayer)
            seed = (a.axis == 0u ? u.x : a.axis == 1u ? u.y : z) == a.layer;
        const size_t q = u.base + z;
        if (seed) seed = in_geo(a.ids[q], a.of);                              // (ids are read where a seed may be)
        a.dist[q] = seed ? 0u : kNone;
    }
}

__global__ void __launch_bounds__(256) k_geo_seed_list(const GeoArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_samples) return;
    const uint32_t x = a.samples[3u * i], y = a.samples[3u * i + 1u], z = a.samples[3u * i + 2u];
    if (x >= a.nx || y >= a.ny || z >= a.nz) return;                          // (the host has refused it: nothing is touched)
    const size_t q = ((size_t)x * a.ny + y) * a.pitch + z;
    if (in_geo(a.ids[q], a.of)) a.dist[q] = 0u;
}

// ---- stage 2: the sweeps ------------------------------------------------------------------------------------------------

// one walk of a lane's line: layer h of the walk is index h (UP) or na - 1 - h of the axis -> an entry was lowered
template <bool UP>
__device__ __forceinline__ bool walk_line(const GeoArgs& a, bool active, uint32_t base, uint32_t stride)
{
    bool any = false;
    uint32_t c = kNone;                                                       // d of the sample before, kNone where it is not in S
    for (uint32_t t0 = 0u; t0 < a.na; t0 += kBatch) {                         // wave-uniform
        bool in[kBatch];                                                      // (unrolled: registers)
        uint32_t d[kBatch];
#pragma unroll
        for (uint32_t k = 0u; k < kBatch; ++k) {
            const uint32_t h = t0 + k, q = base + (UP ? h : a.na - 1u - h) * stride;
            in[k] = active && h < a.na && in_geo(a.ids[q], a.of);
        }
#pragma unroll
        for (uint32_t k = 0u; k < kBatch; ++k) {
            const uint32_t h = t0 + k, q = base + (UP ? h : a.na - 1u - h) * stride;
            d[k] = in[k] ? a.dist[q] : kNone;                                 // (outside S: not read)
        }
#pragma unroll
        for (uint32_t k = 0u; k < kBatch; ++k) {
            const uint32_t h = t0 + k, q = base + (UP ? h : a.na - 1u - h) * stride;
            const uint32_t v = min(d[k], step_on(c, 1u));
            if (in[k] && v < d[k]) {
                a.dist[q] = v;
                any = true;
            }
            c = in[k] ? v : kNone;
        }
    }
    return any;
}

__global__ void __launch_bounds__(256) k_geo_sweep_lines(const GeoArgs a)
{
    // a line along x is one y, along y one x; 64 consecutive z of it, one such unit a wavefront
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6);
    if (unit >= line_units(a)) return;
    const auto u = line_unit<uint32_t>(a, unit, threadIdx.x & 63u);         // (at most 2^31 entries: 32-bit indices)
    const bool active = u.z < a.nz;
    bool any = walk_line<true>(a, active, u.base, u.stride);
    any |= walk_line<false>(a, active, u.base, u.stride);                     // (a lane reads back its own stores: program order)
    if (__ballot(any) != 0ull && (threadIdx.x & 63u) == 0u) *a.word = 1u;
}

// one walk of a word: position `pos` of the lane in the direction of the walk (0 first), `e` the ballot of S in that order,
// `c` the carry into the word (wave-uniform) -> the lane's value
template <bool UP>
__device__ __forceinline__ uint32_t scan_word(uint32_t d, uint32_t lane, uint32_t pos, uint64_t e, uint32_t c)
{
    const uint64_t gaps = ~e & ((1ull << pos) - 1ull);                        // the samples outside S before this lane
    const uint32_t start = gaps != 0ull ? 64u - (uint32_t)__builtin_clzll(gaps) : 0u;         // where the lane's run starts
    uint32_t v = d;
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint32_t t = (uint32_t)__shfl((int)v, (int)((UP ? lane - s : lane + s) & 63u));   // (every lane takes part)
        if (pos >= start + s) v = min(v, step_on(t, s));                      // the lane s before is in the run
    }
    if (start == 0u) v = min(v, step_on(c, pos + 1u));                        // the run starts the word: the carry reaches it
    return v;
}

template <bool UP>
__device__ __forceinline__ bool walk_column(const GeoArgs& a, uint32_t base, uint32_t lane)
{
    bool any = false;
    const uint32_t pos = UP ? lane : 63u - lane;
    uint32_t c = kNone;                                                       // wave-uniform: d of the last sample of the word before
    for (uint32_t k = 0u; k < a.segments; ++k) {                              // wave-uniform
        const uint32_t z = ((UP ? k : a.segments - 1u - k) << 6) + lane, q = base + z;
        const bool in = z < a.nz && in_geo(a.ids[q], a.of);
        const uint32_t d = in ? a.dist[q] : kNone;                            // (outside S and in the padding: not read)
        uint64_t e = __ballot(in);
        if (!UP) e = __builtin_bitreverse64(e);
        const uint32_t v = scan_word<UP>(d, lane, pos, e, c);
        if (in && v < d) {
            a.dist[q] = v;
            any = true;
        }
        // what leaves the word: its last sample's value, kNone where that is not in S
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)v, UP ? 63 : 0);
        c = (e >> 63) != 0ull ? last : kNone;
    }
    return any;
}

__global__ void __launch_bounds__(256) k_geo_sweep_columns(const GeoArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    bool any = false;
    HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny) {                                  // a unit is a whole (x, y) column
        const uint32_t base = (uint32_t)unit * a.pitch;                       // (at most 2^31 entries)
        any |= walk_column<true>(a, base, lane);
        any |= walk_column<false>(a, base, lane);
    }
    if (__ballot(any) != 0ull && lane == 0u) *a.word = 1u;
}

// ---- stage 3: the counts, the sums and the farthest samples ---------------------------------------------------------------

// the greatest v over the 64 lanes, wave-uniform (instance_cells.hpp wave_min_to_last_lane with max; the identity is 0)
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ void __launch_bounds__(256) k_geo_stats(const GeoArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long reached = 0ull, unreached = 0ull, sum = 0ull, best = 0ull;      // lane p: those of id p (p & 63 under kVoid)
    HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny * a.segments) {
        const ColumnUnit u = column_unit(a, unit);
        const uint32_t z = u.z0 + lane, q0 = (uint32_t)u.base + u.z0;         // (at most 2^31 entries)
        const uint32_t id = z < a.nz ? a.ids[u.base + z] : kEmpty;
        const bool in = z < a.nz && in_geo(id, a.of);
        const uint32_t d = in ? a.dist[u.base + z] : kNone;
        const bool got = in && d != kNone;
        gather_counts(in && !got, id, lane, unreached);
        for (uint64_t todo = __ballot(got); todo != 0ull;) {                  // wave-uniform: every id with a reached sample
            const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)__builtin_ctzll(todo));
            const bool mine = got && id == p;
            const uint64_t b = __ballot(mine);
            todo &= ~b;
            const unsigned long long total = wave_sum64(mine ? (unsigned long long)d : 0ull);
            const uint32_t far = wave_max(mine ? d + 1u : 0u);                // (d <= 0xfffffffe: d + 1 does not wrap)
            // the lanes of a unit lie in ascending q: the first lane that has the greatest d is the first sample
            const uint32_t first = (uint32_t)__builtin_ctzll(__ballot(mine && d + 1u == far));
            const unsigned long long key = (unsigned long long)far << 32 | (0xffffffffu - (q0 + first));
            if (lane == (p & 63u)) {
                reached += (unsigned long long)__popcll(b);
                sum += total;
                best = key > best ? key : best;
            }
        }
    }
    // under kVoid every counted id is 255: lane 63 holds slot 64
    const uint32_t slot = a.of == kVoid ? 64u : lane;
    if (reached != 0ull) atomicAdd(&a.counts[slot], reached);
    if (unreached != 0ull) atomicAdd(&a.counts[65u + slot], unreached);
    if (sum != 0ull) atomicAdd(&a.counts[130u + slot], sum);
    if (best != 0ull) atomicMax(&a.keys[slot], best);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

// The one fill and check of what every entry point takes.
int geo_args(const void* ids_dev, const void* dist_dev, const uint32_t dims[3], uint32_t pitch, uint32_t of, GeoArgs& a)
{
    a = GeoArgs{};
    if (!ids_dev || !dist_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    int rc;
    if ((rc = lattice_of(dims, pitch, a)) || (rc = lattice_axis(2, a))) return rc;
    if ((uint64_t)a.nx * a.ny * a.pitch > (1ull << 31))                       // (each factor is at most 65536: no overflow below 2^48)
        return hu_fail(HU_ERR_BAD_ARG, "a distance volume holds at most 2^31 entries");
    if (of != kVoid && (rc = check_of(of, "HU_GEODESIC_SOLID or HU_GEODESIC_EMPTY"))) return rc;
    if (reinterpret_cast<uintptr_t>(dist_dev) % 4u) return hu_fail(HU_ERR_BAD_ARG, "the distances must be aligned to 4 bytes");
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.dist = static_cast<uint32_t*>(const_cast<void*>(dist_dev));
    a.of = of;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_geodesic_seed(const void* ids_dev, void* dist_dev, const uint32_t dims[3], uint32_t pitch, uint32_t of, int mode, int axis,
                     uint32_t layer, const uint32_t* samples_dev, uint32_t n_samples, void* stream)
{
    GeoArgs a;
    int rc;
    if ((rc = geo_args(ids_dev, dist_dev, dims, pitch, of, a))) return rc;
    if (mode != (int)kBorder && mode != (int)kLayer && mode != (int)kList)
        return hu_fail(HU_ERR_BAD_ARG, "mode must be HU_GEODESIC_BORDER, HU_GEODESIC_LAYER or HU_GEODESIC_LIST");
    a.mode = (uint32_t)mode;
    if (a.mode == kLayer) {
        if ((rc = lattice_axis(axis, a))) return rc;
        if (layer >= a.na) return hu_fail(HU_ERR_BAD_ARG, "layer must be below dims[axis]");
        a.axis = (uint32_t)axis, a.layer = layer;
    }
    if (a.mode == kList) {
        if (!samples_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
        if (reinterpret_cast<uintptr_t>(samples_dev) % 4u) return hu_fail(HU_ERR_BAD_ARG, "the samples must be aligned to 4 bytes");
        if (n_samples == 0u || n_samples > HU_GEODESIC_MAX_SAMPLES)
            return hu_fail(HU_ERR_BAD_ARG, "n_samples must be in 1.." + std::to_string(HU_GEODESIC_MAX_SAMPLES));
        a.samples = samples_dev, a.n_samples = n_samples;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_geo_seed, dim3(walking_blocks((uint64_t)a.nx * a.ny * a.segments, 4u)), dim3(256), 0, s, a);
    HU_HIP(hipGetLastError());
    if (a.mode == kList) {
        hipLaunchKernelGGL(k_geo_seed_list, dim3((a.n_samples + 255u) / 256u), dim3(256), 0, s, a);
        HU_HIP(hipGetLastError());
    }
    return HU_OK;
}

int hu_geodesic_sweep(const void* ids_dev, void* dist_dev, uint32_t* word_dev, const uint32_t dims[3], uint32_t pitch, int axis,
                      uint32_t of, void* stream)
{
    GeoArgs a;
    int rc;
    if ((rc = geo_args(ids_dev, dist_dev, dims, pitch, of, a)) || (rc = lattice_axis(axis, a))) return rc;
    if (!word_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(word_dev) % 4u) return hu_fail(HU_ERR_BAD_ARG, "the changed word must be aligned to 4 bytes");
    a.axis = (uint32_t)axis, a.word = word_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.axis == 2u)
        hipLaunchKernelGGL(k_geo_sweep_columns, dim3(walking_blocks((uint64_t)a.nx * a.ny, 1u)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_geo_sweep_lines, dim3((uint32_t)((line_units(a) + 3u) / 4u)), dim3(256), 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_geodesic_stats(const void* ids_dev, const void* dist_dev, uint64_t* keys_dev, uint64_t* counts_dev, const uint32_t dims[3],
                      uint32_t pitch, uint32_t of, void* stream)
{
    GeoArgs a;
    int rc;
    if ((rc = geo_args(ids_dev, dist_dev, dims, pitch, of, a))) return rc;
    if (!keys_dev || !counts_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(keys_dev) % 8u) return hu_fail(HU_ERR_BAD_ARG, "the keys must be aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 8u) return hu_fail(HU_ERR_BAD_ARG, "the counts must be aligned to 8 bytes");
    a.keys = reinterpret_cast<unsigned long long*>(keys_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    hipLaunchKernelGGL(k_geo_stats, dim3(walking_blocks((uint64_t)a.nx * a.ny * a.segments, 4u)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
