// codecad_amd/csrc/instance_ground.hip
//
// WHAT A PRINT STARTS IN MID-AIR, on the part-id volume of an assembly, for codecad_amd/islands.py: the second caller of the
// monotone reachability of instance_drain.hip -- connected within a layer, handed on from layer to layer in one direction only.
// The build direction is s * e, e the unit index vector of `axis` and s = +1 (`up`) or -1; BELOW p is p - s e, the LAYER of p is
// h(p) = p[axis] (s > 0) or n_axis - 1 - p[axis]; the LATERAL axes are the other two.  S is the samples of the lattice with
// id != 255 (`of` = HU_OVERHANG_SOLID) or id == of; h0 is the least layer that holds a sample of S, the plate lies right under
// it.  All integers, exact, and independent of the order in which anything ran.
//   G (grounded): the least subset of S that holds every p of S in layer h0 and every p of S whose sample below or one of
//     whose in-lattice lateral neighbours is in G.  Nothing is handed downwards; the lattice's sides and top ground nothing.
//   F = S \ G (floating);  A (starts) = {p in F : p - s e not in S};  J (joins) = {p in F : p + s e in G}.
// Nothing outside the lattice is in S, and no byte of the padding z in [nz, pitch) is read or written as data.
//
//   1 k_ground_local / k_ground_merge_*: the one labelling body of label_kernels.hpp with the predicate in_set(id, of) and the
//     edges of the two lateral axes: every layer of S is labelled at once, as k_drain_local and k_drain_merge_* label those of
//     the empty samples.  <true>: tiles of 8 x 8 x 16 samples in LDS, then a lane per pair across the tile faces of the two
//     lateral axes; <false> and k_ground_merge_all: the comparison arm, the same bytes.  hu_components_flatten follows.
//   2 k_ground_seed: BIT 31 OF A ROOT'S ENTRY (kFlag of id_volume.hpp) SAYS THAT ITS LAYER COMPONENT IS GROUNDED.  The depth
//     word that hu_overhang_first_layer raised to n_axis - h0 is read here, on the device.  The units are those of layer h0
//     alone: along x and y the 64 z of every line that crosses it, along z the one word of every column that holds it, where
//     the one lane in layer h0 issues the atomic.  A flag that reads set issues no atomic, and a wavefront issues one atomic
//     per distinct root.  There are no lateral seeds, and an empty S (the word reads 0) seeds nothing.
//   3 hu_drain_rise of instance_drain.hip, as it is: it needs only labels and flags.  G is the least fixed point and flags are
//     only ever set: the same bytes whatever ran when, in at most n_axis + 1 passes.
//   4 k_ground_mark: every line of the axis from layer 0 up, once.  Per sample: is it in S (the ids), is its root flagged
//     (plain loads: the flags are final), is the sample below in S (a carry), is the sample above in G -- which lies on the far
//     side of the walk.  <false> (axis 0 or 1): a wavefront owns 64 consecutive z of one line (line_unit of id_volume.hpp),
//     kBatch layers in flight; a lane keeps the id of its last sample where that floats and writes that sample's join byte one
//     step later, when it knows whether the next one is grounded; the top layer's join bytes are 255.  <true> (axis 2): the
//     line is the wavefront; it takes the ballots of S and of G (bit-reversed for s < 0, so that a higher bit is always ABOVE),
//     F = S & ~G, A = F & ~(S << 1 | the top bit of the word below), J = F & (G >> 1 | the lowest G bit of the NEXT word << 63):
//     a word is written when the ballots of the next one are known, the last with a zero.
//     EVERY IN-LATTICE BYTE OF floating, start AND join IS WRITTEN EXACTLY ONCE (255 where nothing is): no memset.  Lane p
//     gathers the counts of id p over everything its wavefront walks and adds them once at the end: counts[0][p] += F,
//     counts[1][p] += A, counts[2][p] += J.
// THE ENTRY 0x7fffffff.  A volume of exactly 2^31 entries has one whose flagged value reads like NONE, the sample
// (nx - 1, ny - 1, nz - 1).  It is the greatest index, so it is a root only when it is alone in its layer component.  Upwards
// it lies in the top layer of every axis: nothing is above it, and k_ground_mark takes S from the ids, where NONE | flag
// reads as flagged.  Downwards it lies in layer 0 and hu_drain_rise, which takes the set from the labels, would not hand its
// ground on: hu_ground_seed refuses exactly 2^31 entries with up == 0.
// No kernel has a private array or scratch (the batches are unrolled: registers); LDS only in k_ground_local.  Entry points: at
// the end.
#include <algorithm>

#include "id_volume.hpp"            // stages 2 and 4: the units, their walk, gather_counts, kFlag, escapes, raise
#include "label_kernels.hpp"        // stage 1

using namespace hu_cells;

namespace {

constexpr uint32_t kBatch = 4u;             // layers a lane of the walk along x and y has in flight

struct GroundArgs {
    const uint8_t* ids;                 // uint8[nx][ny][pitch]
    uint32_t* labels;                   // uint32[nx][ny][pitch]
    uint8_t* floating;
    uint8_t* start;
    uint8_t* join;
    const uint32_t* word;               // the depth word of hu_overhang_first_layer: n_axis - h0, 0 while S is empty
    unsigned long long* counts;         // 3 x 64 accumulators: F, A and J per part
    uint32_t nx, ny, nz, pitch;
    uint32_t total;                     // nx * ny * pitch <= 2^31
    uint32_t axis, up, of;
    uint32_t na;                        // dims[axis]
    uint32_t segments;                  // ceil(nz / 64)
};

// ---- stage 1: the layers' components of S -------------------------------------------------------------------------------

// the edges of the two lateral axes: the forward neighbour along the axis lies in another layer
__device__ __forceinline__ uint32_t lateral(const GroundArgs& k) { return 7u & ~(1u << k.axis); }

template <bool LOCAL>
__global__ void __launch_bounds__(256) k_ground_local(const GroundArgs k)
{
    const uint32_t of = k.of;
    label_tile<LOCAL>(k, k.ids, [of](uint32_t id) { return in_set(id, of); }, lateral(k));
}

// blockIdx.y = 0, 1: the lateral axes in ascending order
__global__ void __launch_bounds__(256) k_ground_merge_faces(const GroundArgs k)
{
    label_merge_faces(k, blockIdx.y == 0u ? (k.axis == 0u ? 1u : 0u) : (k.axis == 2u ? 1u : 2u));
}

__global__ void __launch_bounds__(256) k_ground_merge_all(const GroundArgs k) { label_merge_all(k, lateral(k)); }

// ---- stage 2: the seeds ---------------------------------------------------------------------------------------------------

// the units of ONE layer: along x and y the line_units (64 z of a line each), along z the columns
__host__ __device__ __forceinline__ uint64_t layer_units(const GroundArgs& a)
{
    return a.axis == 2u ? (uint64_t)a.nx * a.ny : line_units(a);
}

__global__ void __launch_bounds__(256) k_ground_seed(const GroundArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t depth = uniform(*a.word);
    if (depth == 0u || depth > a.na) return;                                  // S is empty: nothing is grounded
    const uint32_t h0 = a.na - depth;
    const uint32_t at = a.up ? h0 : a.na - 1u - h0;                           // the index of layer h0 along the axis
    HU_FOR_UNITS(unit, layer_units(a)) {
        uint32_t q;                                                           // (at most 2^31 entries)
        bool seed;
        if (a.axis == 2u) {
            const uint32_t z = (at & ~63u) + lane;                            // the word of the column that holds layer h0
            q = (uint32_t)unit * a.pitch + z;
            seed = z == at;                                                   // (at < nz)
        } else {
            const auto u = line_unit<uint32_t>(a, unit, lane);
            q = u.base + at * u.stride;
            seed = u.z < a.nz;
        }
        const uint32_t l = seed ? a.labels[q] : kNone;
        const bool want = l != kNone && !escapes(a.labels, l, q);             // (kNone has the flag's bit: tested first)
        if (a.axis == 2u) raise<true>(a.labels, lane, want, l);               // one lane
        else raise<false>(a.labels, lane, want, l);                           // the lanes of a unit lie in one layer
    }
}

// ---- stage 4: floating, starts and joins -------------------------------------------------------------------------------

template <bool ALONG_Z>
__global__ void __launch_bounds__(256) k_ground_mark(const GroundArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long floated = 0ull, started = 0ull, joined = 0ull;
    if (!ALONG_Z) {
        // a line along x is one y, along y one x; 64 consecutive z of it, one such unit a wavefront
        const uint64_t unit = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6);
        if (unit < line_units(a)) {
            const auto u = line_unit<uint32_t>(a, unit, lane);                  // (at most 2^31 entries: 32-bit indices)
            const bool active = u.z < a.nz;
            const uint32_t stride = u.stride, base = u.base;
            bool below = false;                                               // the sample below is in S
            uint32_t held = kEmpty;                                           // the id of the sample below where it floats: its join byte is due
            for (uint32_t t0 = 0u; t0 < a.na; t0 += kBatch) {                 // wave-uniform: from layer 0 up
                uint32_t id[kBatch], entry[kBatch], root[kBatch];             // (unrolled: registers)
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride;
                    const bool here = active && h < a.na;
                    id[k] = here ? a.ids[q] : kEmpty;
                    entry[k] = here ? a.labels[q] : kNone;
                }
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride, l = entry[k];
                    const bool in = h < a.na && active && in_set(id[k], a.of);
                    root[k] = in && (l & kFlag) == 0u && l != q ? a.labels[l] : l;
                }
#pragma unroll
                for (uint32_t k = 0u; k < kBatch; ++k) {
                    const uint32_t h = t0 + k, q = base + (a.up ? h : a.na - 1u - h) * stride;
                    const bool here = active && h < a.na;
                    const bool in = here && in_set(id[k], a.of);
                    const bool grounded = in && (root[k] & kFlag) != 0u;
                    const bool floats = in && !grounded;
                    const bool starts = floats && !below;
                    const bool joins = grounded && held != kEmpty;            // ... of the sample below
                    if (here) {
                        a.floating[q] = (uint8_t)(floats ? id[k] : kEmpty);
                        a.start[q] = (uint8_t)(starts ? id[k] : kEmpty);
                        if (h > 0u) a.join[a.up ? q - stride : q + stride] = (uint8_t)(joins ? held : kEmpty);
                        if (h == a.na - 1u) a.join[q] = (uint8_t)kEmpty;      // nothing above the top layer is grounded
                    }
                    gather_counts(floats, id[k], lane, floated);
                    gather_counts(starts, id[k], lane, started);
                    gather_counts(joins, held, lane, joined);
                    below = in;
                    held = floats ? id[k] : kEmpty;
                }
            }
        }
    } else HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny) {                           // a unit is a whole (x, y) column
        const uint32_t base = (uint32_t)unit * a.pitch;
        const uint32_t v = a.up ? lane : 63u - lane;                          // the lane's position in the word: a higher one is above
        // the word below, whose bytes are due: this lane's id and index, and the word's F, A and G (wave-uniform)
        uint32_t due_id = kEmpty, due_q = 0u;
        bool due_active = false;
        uint64_t due_f = 0ull, due_a = 0ull, due_g = 0ull;
        uint64_t carry = 0ull;                                                // bit 0: the top sample of the word below is in S
        for (uint32_t k = 0u; k <= a.segments; ++k) {                         // wave-uniform: from the lowest word up, and one step more
            uint32_t id = kEmpty, q = 0u;
            bool active = false;
            uint64_t s = 0ull, g = 0ull;
            if (k < a.segments) {
                const uint32_t z = ((a.up ? k : a.segments - 1u - k) << 6) + lane;
                active = z < a.nz, q = base + z;
                id = active ? a.ids[q] : kEmpty;
                const bool in = active && in_set(id, a.of);
                const uint32_t l = in ? a.labels[q] : kNone;
                const bool grounded = in && ((l & kFlag) != 0u || (l != q && (a.labels[l] & kFlag) != 0u));
                s = __ballot(in), g = __ballot(grounded);
                if (!a.up) s = __builtin_bitreverse64(s), g = __builtin_bitreverse64(g);
            }
            if (k > 0u) {                                                     // the word below: what is above its top sample is known now
                const uint64_t j = due_f & ((due_g >> 1) | (g << 63));
                const bool floats = ((due_f >> v) & 1ull) != 0ull, starts = ((due_a >> v) & 1ull) != 0ull, joins = ((j >> v) & 1ull) != 0ull;
                if (due_active) {
                    a.floating[due_q] = (uint8_t)(floats ? due_id : kEmpty);
                    a.start[due_q] = (uint8_t)(starts ? due_id : kEmpty);
                    a.join[due_q] = (uint8_t)(joins ? due_id : kEmpty);
                }
                gather_counts(floats, due_id, lane, floated);
                gather_counts(starts, due_id, lane, started);
                gather_counts(joins, due_id, lane, joined);
            }
            due_id = id, due_q = q, due_active = active;
            due_f = s & ~g, due_a = due_f & ~((s << 1) | carry), due_g = g;
            carry = s >> 63;
        }
    }
    if (floated != 0ull) atomicAdd(&a.counts[lane], floated);
    if (started != 0ull) atomicAdd(&a.counts[64u + lane], started);
    if (joined != 0ull) atomicAdd(&a.counts[128u + lane], joined);
}

int ground_args(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, GroundArgs& a)
{
    a = GroundArgs{};
    if (!labels_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    int rc;
    if ((rc = lattice_of(dims, pitch, a)) || (rc = lattice_axis(axis, a)) ||
        (rc = labels_of(labels_dev, "the labels must be aligned to 4 bytes", a)))
        return rc;
    a.axis = (uint32_t)axis, a.up = up != 0;
    return HU_OK;
}

int ground_ids(const void* ids_dev, uint32_t of, GroundArgs& a)
{
    if (!ids_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(ids_dev) % 16u) return hu_fail(HU_ERR_BAD_ARG, "the volume must be aligned to 16 bytes");
    int rc;
    if ((rc = check_of(of, "HU_OVERHANG_SOLID"))) return rc;
    a.ids = static_cast<const uint8_t*>(ids_dev), a.of = of;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_ground_layers(const void* ids_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, uint32_t of, int local,
                     void* stream)
{
    GroundArgs a;
    int rc;
    if ((rc = ground_args(labels_dev, dims, pitch, axis, 1, a)) || (rc = ground_ids(ids_dev, of, a))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (local) {
        hipLaunchKernelGGL(k_ground_local<true>, tile_grid(a), dim3(256), 0, s, a);
        HU_HIP(hipGetLastError());
        const uint64_t most = std::max(face_pairs(a, axis == 0 ? 1u : 0u), face_pairs(a, axis == 2 ? 1u : 2u));
        if (most == 0u) return HU_OK;                              // one tile across both lateral axes: nothing to merge
        hipLaunchKernelGGL(k_ground_merge_faces, dim3(blocks_of(most), 2), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(k_ground_local<false>, tile_grid(a), dim3(256), 0, s, a);
        HU_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ground_merge_all, dim3(blocks_of(a.total)), dim3(256), 0, s, a);
    }
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_ground_seed(void* labels_dev, const uint32_t* word_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, void* stream)
{
    GroundArgs a;
    int rc;
    if ((rc = ground_args(labels_dev, dims, pitch, axis, up, a))) return rc;
    if (!word_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(word_dev) % 4u) return hu_fail(HU_ERR_BAD_ARG, "the depth word must be aligned to 4 bytes");
    if (a.total == 0x80000000u && !a.up)
        return hu_fail(HU_ERR_BAD_ARG, "a volume of exactly 2^31 entries is grounded with up != 0 only: downwards the flag of its last entry would be lost");
    a.word = word_dev;
    hipLaunchKernelGGL(k_ground_seed, dim3(walking_blocks(layer_units(a), 1u)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_ground_mark(const void* ids_dev, const void* labels_dev, void* floating_dev, void* start_dev, void* join_dev, uint64_t* counts_dev,
                   const uint32_t dims[3], uint32_t pitch, int axis, int up, uint32_t of, void* stream)
{
    GroundArgs a;
    int rc;
    if ((rc = ground_args(const_cast<void*>(labels_dev), dims, pitch, axis, up, a)) || (rc = ground_ids(ids_dev, of, a))) return rc;
    if (!floating_dev || !start_dev || !join_dev || !counts_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 8u) return hu_fail(HU_ERR_BAD_ARG, "the counts must be aligned to 8 bytes");
    a.floating = static_cast<uint8_t*>(floating_dev);
    a.start = static_cast<uint8_t*>(start_dev);
    a.join = static_cast<uint8_t*>(join_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (axis == 2)
        hipLaunchKernelGGL((k_ground_mark<true>), dim3(walking_blocks((uint64_t)a.nx * a.ny, 1u)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_ground_mark<false>), dim3((uint32_t)((line_units(a) + 3u) / 4u)), dim3(256), 0, s, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
