// codecad_amd/csrc/instance_drain.hip
//
// WHAT AN ASSEMBLY HOLDS WHEN DRAINED ALONG A LATTICE AXIS, on the part-id volume of an assembly, for codecad_amd/drainage.py.
// Up is s * e, e the unit index vector of `axis` and s = +1 (`up`) or -1; BELOW p is p - s e, the LAYER of p is h(p) = p[axis]
// (s > 0) or n_axis - 1 - p[axis]; the LATERAL axes are the other two.  E is the samples of the lattice with id == 255, S those
// with id != 255.  All integers, exact, and independent of the order in which anything ran.
//   X (escapes): the least subset of E that holds every p of E in layer 0 or with a lateral index of 0 or n - 1, and every p of E
//     whose sample below or one of whose lateral neighbours is in X.
//   T = E \ X (trapped); the FLOOR of a trapped sample is the nearest sample of S below it on its line.
// Nothing outside the lattice is in S, and no byte of the padding z in [nz, pitch) is read or written as data.
//
// MONOTONE REACHABILITY: connected within a layer, handed on from layer to layer in one direction only.
//   1 k_drain_local / k_drain_merge_*: the union-find of instance_components.hip BY CONSTRUCTION: they wrap the one labelling
//     body of label_kernels.hpp (instance_components.hip states THE INVARIANT, id_volume.hpp has find and unite) with the predicate id == 255
//     and edges = lateral(): the two lateral axes only, so every layer is labelled at once and no edge crosses layers.
//     k_drain_local<true>: a tile of 8 x 8 x 16 samples in LDS (4 KiB of labels, 256 B of column masks), then k_drain_merge_faces,
//     a lane per pair across the tile faces of the two lateral axes.  k_drain_local<false> writes label = own index and
//     k_drain_merge_all, a lane per sample, unites its two forward lateral neighbours: the comparison arm, the same bytes.
//     hu_components_flatten then makes every entry the index of its root: it needs only the invariant.
//   2 k_drain_seed: BIT 31 OF A ROOT'S ENTRY IS THE ESCAPE FLAG (at most 2^31 entries: the bit is free, the device of kSlot).
//     A sample of E in layer 0 or at a lateral border flags its root.  A flag that reads set issues no atomic, and a wavefront
//     issues one atomic per distinct root of a unit.  Units without a border sample load nothing.
//   3 k_drain_rise, one PASS a launch: every p of E whose sample below is in E under a flagged root flags its own root, and
//     *changed is set when a flag was newly set (the value atomicOr returns decides).  A pass walks every line of the axis from
//     layer 0 upwards and carries "the sample below escapes", so a straight shaft rises through all its layers in one pass.
//     <false> (axis 0 or 1): a wavefront owns 64 consecutive z of one line (line_unit of id_volume.hpp), the carry is a register per lane, kBatch entries and
//     then their roots' entries are in flight.  <true> (axis 2): the line is the wavefront itself; it takes the ballots of E and of
//     the flags it read (bit-reversed for s < 0, so that a higher bit is always ABOVE), floods the flag bits upwards through the
//     runs of E by the carry of one addition and hands the top bit on into the next word.  Along one line every sample lies in
//     another layer and so under another root: a word is read once.
//     Flags are only ever set and X is the least fixed point: the same bytes whatever ran when.  A pass does at least what one
//     synchronous step over all (sample, below) pairs does, so n_axis + 1 passes are the most.
//   4 k_drain_floor: the same lines, walked the same way, carrying the id of the last sample of S seen from below; a sample of E
//     whose root is unflagged writes that id.  EVERY IN-LATTICE BYTE OF trapped IS WRITTEN (255 elsewhere): no memset.  Along z the
//     nearest set bit of S below a lane comes from the ballot and its id by a cross-lane read; the carry from the word below is
//     the last id, 255 while there was none.  Lane p gathers the count of floor p over everything its wavefront walks and adds
//     it once at the end.
// THE ENTRY 0x7fffffff.  A volume of exactly 2^31 entries has one whose flagged value reads like NONE.  It is the sample
// (nx - 1, ny - 1, nz - 1): a lateral border on every axis, as is every sample of its line, so it always escapes and nobody waits
// for its carry; k_drain_floor takes E from the ids, where NONE | flag reads as flagged.
// No kernel has a private array or scratch (the batches are unrolled: registers).  Entry points: at the end.
#include <algorithm>

#include "id_volume.hpp"            // stages 2 to 4: the units, their walk, gather_counts; kFlag, live, escapes, raise
#include "label_kernels.hpp"        // stage 1

using namespace hu_cells;

namespace {

constexpr uint32_t kBatch = 4u;             // layers a lane of the walks along x and y has in flight

struct DrainArgs {
    const uint8_t* ids;                 // uint8[nx][ny][pitch]
    uint32_t* labels;                   // uint32[nx][ny][pitch]
    uint8_t* trapped;
    uint32_t* changed;
    unsigned long long* counts;         // 64 accumulators: the trapped samples per floor
    uint32_t nx, ny, nz, pitch;
    uint32_t total;                     // nx * ny * pitch <= 2^31
    uint32_t axis, up;
    uint32_t na;                        // dims[axis]
    uint32_t segments;                  // ceil(nz / 64)
};

// ---- stage 1: the layers' components ----------------------------------------------------------------------------------

// the edges of the two lateral axes: the forward neighbour along the axis lies in another layer
__device__ __forceinline__ uint32_t lateral(const DrainArgs& k) { return 7u & ~(1u << k.axis); }

template <bool LOCAL>
__global__ void __launch_bounds__(256) k_drain_local(const DrainArgs k)
{
    label_tile<LOCAL>(k, k.ids, [](uint32_t id) { return id == kEmpty; }, lateral(k));
}

// blockIdx.y = 0, 1: the lateral axes in ascending order
__global__ void __launch_bounds__(256) k_drain_merge_faces(const DrainArgs k)
{
    label_merge_faces(k, blockIdx.y == 0u ? (k.axis == 0u ? 1u : 0u) : (k.axis == 2u ? 1u : 2u));
}

__global__ void __launch_bounds__(256) k_drain_merge_all(const DrainArgs k) { label_merge_all(k, lateral(k)); }

// ---- stages 2 and 3: the flags ----------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_drain_seed(const DrainArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny * a.segments) {
        const ColumnUnit u = column_unit(a, unit);
        const uint32_t z = u.z0 + lane;
        const bool xb = u.x == 0u || u.x == a.nx - 1u, yb = u.y == 0u || u.y == a.ny - 1u, zb = z == 0u || z == a.nz - 1u;
        const bool first = a.axis == 0u ? u.x == (a.up ? 0u : a.nx - 1u) : a.axis == 1u ? u.y == (a.up ? 0u : a.ny - 1u)
                                                                                       : z == (a.up ? 0u : a.nz - 1u);
        const bool side = a.axis == 0u ? (yb || zb) : a.axis == 1u ? (xb || zb) : (xb || yb);
        const bool seed = z < a.nz && (first || side);
        if (__ballot(seed) == 0ull) continue;                                 // wave-uniform: nothing of the unit is read
        const uint32_t q = (uint32_t)u.base + z;                              // (at most 2^31 entries)
        const uint32_t l = seed ? a.labels[q] : kNone;
        const bool want = l != kNone && !escapes(a.labels, l, q);             // (kNone has the flag's bit: tested first)
        if (a.axis == 2u) raise<true>(a.labels, lane, want, l);               // the lanes of a unit lie in 64 layers
        else raise<false>(a.labels, lane, want, l);
    }
}

template <bool ALONG_Z>
__global__ void __launch_bounds__(256) k_drain_rise(const DrainArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    bool any = false;
    if (!ALONG_Z) {
        // a line along x is one y, along y one x; 64 consecutive z of it, one such unit a wavefront
        const uint64_t unit = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6);
        if (unit >= line_units(a)) return;
        const auto u = line_unit<uint32_t>(a, unit, lane);                  // (at most 2^31 entries: 32-bit indices)
        const bool active = u.z < a.nz;
        const uint32_t stride = u.stride, base = u.base;
        bool below = false;                                                   // the sample below is in E and escapes
        for (uint32_t t0 = 0u; t0 < a.na; t0 += kBatch) {                     // wave-uniform: from layer 0 up
            uint32_t entry[kBatch], root[kBatch];                             // (unrolled: registers)
#pragma unroll
            for (uint32_t k = 0u; k < kBatch; ++k) {
                const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride;
                entry[k] = active && h < a.na ? a.labels[q] : kNone;
            }
#pragma unroll
            for (uint32_t k = 0u; k < kBatch; ++k) {                          // the roots' entries, live: own entries tell themselves
                const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride, l = entry[k];
                root[k] = (l & kFlag) == 0u && l != q ? live(a.labels + l) : l;
            }
#pragma unroll
            for (uint32_t k = 0u; k < kBatch; ++k) {
                const uint32_t l = entry[k];
                const bool in = l != kNone, flagged = in && (root[k] & kFlag) != 0u;
                const bool want = in && below && !flagged;
                if (__ballot(want) != 0ull) any |= raise<false>(a.labels, lane, want, l);     // wave-uniform
                below = flagged || want;
            }
        }
    } else HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny) {                           // a unit is a whole (x, y) column
        const uint32_t base = (uint32_t)unit * a.pitch;
        const uint32_t v = a.up ? lane : 63u - lane;                          // the lane's position in the word: a higher one is above
        uint64_t carry = 0ull;                                                // wave-uniform: bit 0, the sample below the word escapes
        const uint32_t zf = ((a.up ? 0u : a.segments - 1u) << 6) + lane;
        uint32_t next = zf < a.nz ? a.labels[base + zf] : kNone;
        for (uint32_t k = 0u; k < a.segments; ++k) {                          // wave-uniform: from the lowest word up
            const uint32_t z = ((a.up ? k : a.segments - 1u - k) << 6) + lane, l = next;
            if (k + 1u < a.segments) {                                        // (the next word is on its way)
                const uint32_t zn = a.up ? z + 64u : z - 64u;
                next = zn < a.nz ? a.labels[base + zn] : kNone;
            }
            const bool in = l != kNone;                                       // (z >= nz: kNone)
            const bool flagged = in && escapes(a.labels, l, base + z);
            uint64_t e = __ballot(in), f = __ballot(flagged);
            if (!a.up) e = __builtin_bitreverse64(e), f = __builtin_bitreverse64(f);
            // the flags flood upwards through the runs of E: a carry enters a run at its lowest source, clears every bit of the
            // run from there on but those of further sources, and leaves it above its top
            const uint64_t source = f | (carry & e);
            const uint64_t out = (((e + source) ^ e) & e) | source;
            const bool want = (((out & ~f) >> v) & 1ull) != 0ull;             // in E, unflagged: l is the root's index
            any |= raise<true>(a.labels, lane, want, l);
            carry = out >> 63;
        }
    }
    if (any) *a.changed = 1u;
}

// ---- stage 4: the floors ------------------------------------------------------------------------------------------------

template <bool ALONG_Z>
__global__ void __launch_bounds__(256) k_drain_floor(const DrainArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0ull;
    if (!ALONG_Z) {
        const uint64_t unit = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6);
        if (unit < line_units(a)) {
            const auto u = line_unit<uint32_t>(a, unit, lane);                  // (at most 2^31 entries: 32-bit indices)
            const bool active = u.z < a.nz;
            const uint32_t stride = u.stride, base = u.base;
            uint32_t floor = kEmpty;                                          // the id of the last sample of S below
            for (uint32_t t0 = 0u; t0 < a.na; t0 += kBatch) {                 // wave-uniform: from layer 0 up
                uint32_t id[kBatch], entry[kBatch], root[kBatch];             // (unrolled: registers)
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride;
                    const bool here = active && h < a.na;
                    id[k] = here ? a.ids[q] : 0u;                             // (0: neither read further nor written)
                    entry[k] = here ? a.labels[q] : kNone;
                }
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride, l = entry[k];
                    root[k] = id[k] == kEmpty && (l & kFlag) == 0u && l != q ? a.labels[l] : l;
                }
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride;
                    const bool here = active && h < a.na;
                    if (here && id[k] != kEmpty) floor = id[k];
                    const bool held = here && id[k] == kEmpty && (root[k] & kFlag) == 0u && floor != kEmpty;
                    if (here) a.trapped[q] = (uint8_t)(held ? floor : kEmpty);
                    gather_counts(held, floor, lane, mine);
                }
            }
        }
    } else HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny) {                           // a unit is a whole (x, y) column
        const uint32_t base = (uint32_t)unit * a.pitch;
        const uint32_t v = a.up ? lane : 63u - lane;                          // the lane's position in the word: a higher one is above
        uint32_t carry = kEmpty;                                              // wave-uniform: the id of the last sample of S below the word
        for (uint32_t k = 0u; k < a.segments; ++k) {                          // wave-uniform: from the lowest word up
            const uint32_t z = ((a.up ? k : a.segments - 1u - k) << 6) + lane, q = base + z;
            const bool active = z < a.nz;
            const uint32_t id = active ? a.ids[q] : kEmpty;
            const bool empty = active && id == kEmpty;
            const uint32_t l = empty ? a.labels[q] : kNone;
            const bool open = empty && ((l & kFlag) != 0u || (l != q && (a.labels[l] & kFlag) != 0u));
            uint64_t set = __ballot(id != kEmpty);
            if (!a.up) set = __builtin_bitreverse64(set);
            const uint64_t under = set & ((1ull << v) - 1ull);                // the samples of S below this lane in the word
            const uint32_t j = under != 0ull ? 63u - (uint32_t)__builtin_clzll(under) : v;         // the nearest of them
            const uint32_t fetched = (uint32_t)__shfl((int)id, (int)(a.up ? j : 63u - j));         // (every lane takes part)
            const uint32_t floor = under != 0ull ? fetched : carry;
            const bool held = empty && !open && floor != kEmpty;
            if (active) a.trapped[q] = (uint8_t)(held ? floor : kEmpty);
            gather_counts(held, floor, lane, mine);
            if (set != 0ull) {                                                // the highest sample of S of the word is what leaves it
                const uint32_t top = 63u - (uint32_t)__builtin_clzll(set);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)(a.up ? top : 63u - top));
            }
        }
    }
    if (mine != 0ull) atomicAdd(&a.counts[lane], mine);
}

int drain_args(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, DrainArgs& a)
{
    a = DrainArgs{};
    if (!labels_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    int rc;
    if ((rc = lattice_of(dims, pitch, a)) || (rc = lattice_axis(axis, a)) ||
        (rc = labels_of(labels_dev, "the labels must be aligned to 4 bytes", a)))
        return rc;
    a.axis = (uint32_t)axis, a.up = up != 0;
    return HU_OK;
}

// a wavefront a unit of 64 z of a line along x or y
inline uint32_t line_blocks(const DrainArgs& a) { return (uint32_t)((line_units(a) + 3u) / 4u); }

}  // namespace

extern "C" {

int hu_drain_layers(const void* ids_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int local, void* stream)
{
    DrainArgs a;
    int rc;
    if ((rc = drain_args(labels_dev, dims, pitch, axis, 1, a))) return rc;
    if (!ids_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(ids_dev) % 16u) return hu_fail(HU_ERR_BAD_ARG, "the volume must be aligned to 16 bytes");
    a.ids = static_cast<const uint8_t*>(ids_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (local) {
        hipLaunchKernelGGL(k_drain_local<true>, tile_grid(a), dim3(256), 0, s, a);
        HU_HIP(hipGetLastError());
        const uint64_t most = std::max(face_pairs(a, axis == 0 ? 1u : 0u), face_pairs(a, axis == 2 ? 1u : 2u));
        if (most == 0u) return HU_OK;                              // one tile across both lateral axes: nothing to merge
        hipLaunchKernelGGL(k_drain_merge_faces, dim3(blocks_of(most), 2), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(k_drain_local<false>, tile_grid(a), dim3(256), 0, s, a);
        HU_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_drain_merge_all, dim3(blocks_of(a.total)), dim3(256), 0, s, a);
    }
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_drain_seed(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, void* stream)
{
    DrainArgs a;
    int rc;
    if ((rc = drain_args(labels_dev, dims, pitch, axis, up, a))) return rc;
    hipLaunchKernelGGL(k_drain_seed, dim3(walking_blocks((uint64_t)a.nx * a.ny * a.segments, 4u)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_drain_rise(void* labels_dev, uint32_t* changed_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, void* stream)
{
    DrainArgs a;
    int rc;
    if ((rc = drain_args(labels_dev, dims, pitch, axis, up, a))) return rc;
    if (!changed_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(changed_dev) % 4u) return hu_fail(HU_ERR_BAD_ARG, "the changed word must be aligned to 4 bytes");
    a.changed = changed_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (axis == 2)
        hipLaunchKernelGGL((k_drain_rise<true>), dim3(walking_blocks((uint64_t)a.nx * a.ny, 1u)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_drain_rise<false>), dim3(line_blocks(a)), dim3(256), 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_drain_floor(const void* ids_dev, const void* labels_dev, void* trapped_dev, uint64_t* counts_dev, const uint32_t dims[3],
                   uint32_t pitch, int axis, int up, void* stream)
{
    DrainArgs a;
    int rc;
    if ((rc = drain_args(const_cast<void*>(labels_dev), dims, pitch, axis, up, a))) return rc;
    if (!ids_dev || !trapped_dev || !counts_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 8u) return hu_fail(HU_ERR_BAD_ARG, "the counts must be aligned to 8 bytes");
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.trapped = static_cast<uint8_t*>(trapped_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (axis == 2)
        hipLaunchKernelGGL((k_drain_floor<true>), dim3(walking_blocks((uint64_t)a.nx * a.ny, 1u)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_drain_floor<false>), dim3(line_blocks(a)), dim3(256), 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
