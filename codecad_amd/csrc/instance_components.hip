// codecad_amd/csrc/instance_components.hip
//
// The CONNECTED COMPONENTS of a predicate on the part-id volume of an assembly (codecad_amd/assembly_components.py): S is
// the samples with id == 255 (empty space) or id != 255 (solid) of the uint8[nx][ny][pitch] part-id volume (id_volume.hpp
// has its contract), two samples of S are connected when they differ by one step along one axis, and the label of a
// sample is the smallest linear index (x * ny + y) * nz + z of its component, NONE = 0xffffffff outside S.  The padding
// z in [nz, pitch) is neither in S nor anybody's neighbour: no kernel reads a byte of it as a sample.
//
// ROWS.  labels is uint32[nx][ny][pitch].  Until the last kernel a label is an index INTO THAT BUFFER,
//     q = (x * ny + y) * pitch + z,
// so that a label is also the address of its parent.  q grows with the linear index (both order x, then y, then z), so the
// smallest q of a component belongs to its smallest linear index; k_comp_finish converts.  The entry points refuse a buffer
// of more than 2^31 entries: bit 31 of an entry is free, and stage 4 keeps a root's slot under it.
//
// THE INVARIANT.  From k_comp_local on, every entry of a sample of S holds label[q] <= q, the index of a sample of its own
// component, and no kernel ever RAISES an entry (plain stores write a root found by descending, atomicMin only lowers).
// Every loop over global memory (find, unite) follows labels that strictly decrease, so it ends after at most q steps
// whatever other wavefronts do; there is no lock, no flag and no wait for anybody's progress.
//
// Stages 1 and 2 are THE ONE LABELLING BODY of label_kernels.hpp, which describes it, wrapped with the predicate of `solid`
// and every edge (edges = 7, a constant); instance_reach.hip wraps the same body for its layers.
//   1 k_comp_local<true>: label_tile, a tile of 8 x 8 x 16 samples labelled in LDS (4 KiB of labels, 256 B of column
//     masks), every sample united with its three forward neighbours inside the tile; NONE outside S and in the padding.
//     k_comp_local<false> (the comparison arm) writes label = own index.
//   2 k_comp_merge_faces: label_merge_faces, a lane per pair of samples across a tile face, three ranges of one launch
//     (blockIdx.y is the axis); k_comp_merge_all (the comparison arm): label_merge_all, a lane per sample.
//   3 k_comp_flatten: every sample of S replaces its label by its root.
//   4 k_comp_roots: a root (label == own index) takes a slot from *counter (one atomic per wavefront) and keeps
//     0x80000000 | slot in its own entry -- no third volume.  k_comp_stats: a unit is 64 consecutive z of one (x, y)
//     column; a lane finds its slot in its root's entry, the wavefront walks the unit's distinct slots (readlane / ballot),
//     reduces count, z sum, z range, the owners' mask and the flags per slot, gathers them in registers over 64 consecutive
//     units while the slot stays the same, and lane 0 issues one atomic per accumulator word when it changes and at the
//     end.  Slots >= capacity are counted and not touched: the host regrows the table and runs k_comp_stats again.
//   5 k_comp_finish: an entry becomes the LINEAR index of its root.
// No kernel has a private array or scratch.  find and unite: id_volume.hpp; kNone, the tiles, blocks_of: label_kernels.hpp.  The entry points are at the end of this file.
#include <algorithm>

#include "id_volume.hpp"            // stages 3 to 5: find, the volume's contract
#include "label_kernels.hpp"        // stages 1 and 2

using namespace sdfk;
using namespace hu_cells;

namespace {

constexpr uint32_t kSlot = 0x80000000u;     // stage 4: the entry of a root holds kSlot | slot

// the accumulators of a component (72 bytes; the host's dtype is assembly_components._ROW).  A zeroed row is an empty one:
// the low corner of the box is kept COMPLEMENTED, so that it grows by atomicMax from 0 like everything else.
struct CompRow {
    unsigned long long count, sums[3], parts;
    uint32_t not_lo[3], hi[3];
    uint32_t label, flags;                  // flags bit 0: touches the border of the lattice
};
static_assert(sizeof(CompRow) == HU_COMPONENTS_ROW_BYTES, "the row of include/hip_util.h");

struct CompArgs {
    const uint8_t* volume;
    uint32_t* labels;
    uint32_t nx, ny, nz, pitch;
    uint32_t total;                          // nx * ny * pitch <= 2^31
    uint32_t solid;                          // S: id != 255 (else id == 255)
    uint32_t* counter;
    CompRow* table;
    uint32_t capacity;
};

__device__ __forceinline__ bool in_flagged_set(uint32_t id, uint32_t solid) { return (id != kEmpty) == (solid != 0u); }

template <bool LOCAL>
__global__ void __launch_bounds__(256) k_comp_local(const CompArgs k)
{
    label_tile<LOCAL>(k, k.volume, [solid = k.solid](uint32_t id) { return in_flagged_set(id, solid); }, 7u);
}

// blockIdx.y = the axis
__global__ void __launch_bounds__(256) k_comp_merge_faces(const CompArgs k) { label_merge_faces(k, blockIdx.y); }

__global__ void __launch_bounds__(256) k_comp_merge_all(const CompArgs k) { label_merge_all(k, 7u); }

__global__ void __launch_bounds__(256) k_comp_flatten(const CompArgs k)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= k.total) return;
    const uint32_t l = k.labels[q];
    if (l == kNone || l == q) return;
    const uint32_t r = find(k.labels, l);                          // uses THE INVARIANT; r <= l: the store lowers the entry
    if (r != l) k.labels[q] = r;
}

__global__ void __launch_bounds__(256) k_comp_roots(const CompArgs k)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const bool root = q < k.total && k.labels[q] == q;            // (kNone is no index: total <= 2^31)
    const uint64_t roots = __ballot(root);
    if (roots == 0ull) return;                                     // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(k.counter, (uint32_t)__popcll(roots));
    base = uniform(base);
    if (root) k.labels[q] = kSlot | (base + (uint32_t)__popcll(roots & ((1ull << lane) - 1ull)));
}

// the owner bit of the sample at byte offset `at`, or 0 for an empty one
__device__ __forceinline__ unsigned long long owner_bit(const uint8_t* volume, size_t at)
{
    const uint32_t id = volume[at];
    return id == kEmpty ? 0ull : 1ull << (id & 63u);
}

// what a wavefront has gathered for the component it is in, wave-uniform, between two flushes
struct Run {
    uint32_t slot;                           // kNone: nothing gathered
    unsigned long long count, sx, sy, sz, parts;
    uint32_t lox, loy, loz, hix, hiy, hiz, border, label;   // label: the root's linear index once it was met, else kNone
};
// one atomic per accumulator word, run and component
__device__ __forceinline__ void flush(const CompArgs& k, const Run& r, uint32_t lane)
{
    if (r.slot == kNone || lane != 0u) return;
    CompRow* row = k.table + r.slot;
    atomicAdd(&row->count, r.count);
    atomicAdd(&row->sums[0], r.sx);
    atomicAdd(&row->sums[1], r.sy);
    atomicAdd(&row->sums[2], r.sz);
    if (r.parts) atomicOr(&row->parts, r.parts);
    atomicMax(&row->not_lo[0], ~r.lox);
    atomicMax(&row->not_lo[1], ~r.loy);
    atomicMax(&row->not_lo[2], ~r.loz);
    atomicMax(&row->hi[0], r.hix);
    atomicMax(&row->hi[1], r.hiy);
    atomicMax(&row->hi[2], r.hiz);
    if (r.border) atomicOr(&row->flags, 1u);
    if (r.label != kNone) row->label = r.label;
}

// A UNIT is 64 consecutive z of one column: x and y are wave-uniform, so the x and y sums are count * x and count * y, the z
// range comes from the ballot, and only the z sum and the owners' mask need a reduction across the lanes.  A wavefront walks
// kStatsUnits consecutive units (along z, then y, then x) and keeps gathering in registers while the component stays the
// same: the outside, one component of millions of samples, costs an atomic per word every 64 units and not every unit.  It
// indexes in 32 bits (at most 2^31 entries) and its units are consecutive: not column_unit and HU_FOR_UNITS.
constexpr uint32_t kStatsUnits = 64u;
__global__ void __launch_bounds__(256) k_comp_stats(const CompArgs k)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t segments = (k.nz + 63u) >> 6;
    const uint64_t units = (uint64_t)k.nx * k.ny * segments;
    const uint64_t first = ((uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6)) * kStatsUnits;
    const uint64_t last = first + kStatsUnits < units ? first + kStatsUnits : units;
    Run run{kNone, 0ull, 0ull, 0ull, 0ull, 0ull, 0u, 0u, 0u, 0u, 0u, 0u, 0u, kNone};
    for (uint64_t unit = first; unit < last; ++unit) {              // wave-uniform; this kernel has no barrier
        const uint32_t column = (uint32_t)(unit / segments), z0 = ((uint32_t)(unit - (uint64_t)column * segments)) << 6;
        const uint32_t x = column / k.ny, y = column - x * k.ny, z = z0 + lane;
        const uint32_t q = column * k.pitch + z;
        const uint32_t l = z < k.nz ? k.labels[q] : kNone;         // (z < nz <= pitch: inside the row)
        const bool in = l != kNone;
        uint32_t slot = 0u;
        unsigned long long owners = 0ull;
        if (in) {
            slot = ((l & kSlot) ? l : k.labels[l]) & ~kSlot;       // a root's entry holds its slot, anybody else's its root
            if (k.solid) {
                owners = owner_bit(k.volume, q);
            } else {                                               // the parts that bound the void: in-lattice neighbours only
                const size_t sy = k.pitch, sx = (size_t)k.ny * k.pitch;
                if (z > 0u) owners |= owner_bit(k.volume, (size_t)q - 1u);
                if (z + 1u < k.nz) owners |= owner_bit(k.volume, (size_t)q + 1u);
                if (y > 0u) owners |= owner_bit(k.volume, (size_t)q - sy);
                if (y + 1u < k.ny) owners |= owner_bit(k.volume, (size_t)q + sy);
                if (x > 0u) owners |= owner_bit(k.volume, (size_t)q - sx);
                if (x + 1u < k.nx) owners |= owner_bit(k.volume, (size_t)q + sx);
            }
        }
        const bool side = x == 0u || x == k.nx - 1u || y == 0u || y == k.ny - 1u;   // wave-uniform
        for (uint64_t todo = __ballot(in); todo != 0ull;) {        // wave-uniform: one turn per distinct slot, at most 32
            const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)slot, (int)__builtin_ctzll(todo));
            const bool mine = in && slot == s;
            const uint64_t b = __ballot(mine);
            todo &= ~b;
            if (s >= k.capacity) continue;                         // counted by k_comp_roots; the host regrows the table
            const uint32_t zsum = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_last_lane(mine ? z : 0u), 63);
            const unsigned long long parts = wave_or64(mine ? owners : 0ull);
            const uint64_t root = __ballot(mine && (l & kSlot) != 0u);
            if (s != run.slot) {                                   // another component: what was gathered goes to its row
                flush(k, run, lane);
                run = Run{s, 0ull, 0ull, 0ull, 0ull, 0ull, kNone, kNone, kNone, 0u, 0u, 0u, 0u, kNone};
            }
            const unsigned long long n = (unsigned long long)__popcll(b);
            const uint32_t lo = z0 + (uint32_t)__builtin_ctzll(b), hi = z0 + 63u - (uint32_t)__builtin_clzll(b);
            run.count += n;
            run.sx += n * x;
            run.sy += n * y;
            run.sz += zsum;
            run.parts |= parts;
            run.lox = min(run.lox, x), run.loy = min(run.loy, y), run.loz = min(run.loz, lo);
            run.hix = max(run.hix, x), run.hiy = max(run.hiy, y), run.hiz = max(run.hiz, hi);
            run.border |= (side || lo == 0u || hi == k.nz - 1u) ? 1u : 0u;
            if (root) run.label = (x * k.ny + y) * k.nz + z0 + (uint32_t)__builtin_ctzll(root);   // the LINEAR index
        }
    }
    flush(k, run, lane);
}

__global__ void __launch_bounds__(256) k_comp_finish(const CompArgs k)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= k.total) return;
    const uint32_t l = k.labels[q];
    if (l == kNone) return;
    const uint32_t r = (l & kSlot) ? q : l;
    k.labels[q] = r - (r / k.pitch) * (k.pitch - k.nz);           // (x * ny + y) * nz + z of the root
}

int comp_args(const void* volume_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, CompArgs& k)
{
    k = CompArgs{};
    if (!labels_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    const char* misaligned = "the volume must be aligned to 16 bytes, the labels to 4";
    int rc;
    if ((rc = lattice_of(dims, pitch, k)) || (rc = labels_of(labels_dev, misaligned, k))) return rc;
    if (reinterpret_cast<uintptr_t>(volume_dev) % 16u) return hu_fail(HU_ERR_BAD_ARG, misaligned);
    k.volume = static_cast<const uint8_t*>(volume_dev);
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_components_local(const void* volume_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int solid, int local,
                        void* stream)
{
    CompArgs k;
    int rc;
    if ((rc = comp_args(volume_dev, labels_dev, dims, pitch, k))) return rc;
    if (!volume_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    k.solid = solid ? 1u : 0u;
    if (local)
        hipLaunchKernelGGL(k_comp_local<true>, tile_grid(k), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    else
        hipLaunchKernelGGL(k_comp_local<false>, tile_grid(k), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_components_merge(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int local, void* stream)
{
    CompArgs k;
    int rc;
    if ((rc = comp_args(nullptr, labels_dev, dims, pitch, k))) return rc;
    if (local) {
        const uint64_t most = std::max(face_pairs(k, 0u), std::max(face_pairs(k, 1u), face_pairs(k, 2u)));
        if (most == 0u) return HU_OK;                              // one tile: nothing to merge
        hipLaunchKernelGGL(k_comp_merge_faces, dim3(blocks_of(most), 3), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    } else {
        hipLaunchKernelGGL(k_comp_merge_all, dim3(blocks_of(k.total)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    }
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_components_flatten(void* labels_dev, const uint32_t dims[3], uint32_t pitch, void* stream)
{
    CompArgs k;
    int rc;
    if ((rc = comp_args(nullptr, labels_dev, dims, pitch, k))) return rc;
    hipLaunchKernelGGL(k_comp_flatten, dim3(blocks_of(k.total)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_components_stats(const void* volume_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int solid, int assign_slots,
                        uint32_t* counter_dev, void* table_dev, uint32_t capacity, void* stream)
{
    CompArgs k;
    int rc;
    if ((rc = comp_args(volume_dev, labels_dev, dims, pitch, k))) return rc;
    if (!volume_dev || !counter_dev || !table_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(counter_dev) % 4u || reinterpret_cast<uintptr_t>(table_dev) % 8u)
        return hu_fail(HU_ERR_BAD_ARG, "the counter must be aligned to 4 bytes, the table to 8");
    if (capacity == 0u || capacity > 0x7fffffffu) return hu_fail(HU_ERR_BAD_ARG, "capacity must be in 1..2^31 - 1");
    k.solid = solid ? 1u : 0u;
    k.counter = counter_dev;
    k.table = static_cast<CompRow*>(table_dev);
    k.capacity = capacity;
    if (assign_slots) {
        hipLaunchKernelGGL(k_comp_roots, dim3(blocks_of(k.total)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
        HU_HIP(hipGetLastError());
    }
    const uint64_t waves = ((uint64_t)k.nx * k.ny * ((k.nz + 63u) / 64u) + kStatsUnits - 1u) / kStatsUnits;
    hipLaunchKernelGGL(k_comp_stats, dim3((uint32_t)((waves + 3u) / 4u)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_components_finish(void* labels_dev, const uint32_t dims[3], uint32_t pitch, void* stream)
{
    CompArgs k;
    int rc;
    if ((rc = comp_args(nullptr, labels_dev, dims, pitch, k))) return rc;
    hipLaunchKernelGGL(k_comp_finish, dim3(blocks_of(k.total)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
