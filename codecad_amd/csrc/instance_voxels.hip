// codecad_amd/csrc/instance_voxels.hip
//
// The PART-ID VOLUME of an assembly (codecad_amd/assembly_voxels.py): for every lattice sample the lowest visible index k
// with w_k(p) < 0 (strictly, w_k the tape of instance k alone as in instance_pairs.hip), or EMPTY = 255 -- the owner rule of
// instance_section.hip's part_ids and of instance_mass.hip's O_k -- as uint8[nx][ny][pitch], pitch = nz rounded up to a
// multiple of 16, and per instance the number of samples it owns: bit for bit what evaluating every instance at every
// sample gives.  The host prefills the volume with EMPTY; the kernels write where a part owns a sample (and whole z runs
// of the finest cells).
//
// The traversal is the one of instance_pairs.hip -- cubic cells of 4^k samples, one wavefront per cell, lane = 16 x + 4 y + z
// -- over the default 16-byte row with one more bit,
//     {x0 | y0 << 16, z0 | capped << 31, cand lo, cand hi},
// capped: the HIGHEST bit of cand is FULL in this cell, every sample of the cell inside that instance.  Candidates above a
// full one are never listed: they cannot own a sample of the cell.
//   k_voxel_cells (child side s >= 4): a lane is a child cell, its centre and a.thr those of k_mass_cells.  The candidates
//     are evaluated in ASCENDING index, the capped top bit is inherited without evaluation: w >= thr drops a candidate,
//     w < -thr makes it full, anything else, a NaN included, keeps a boundary candidate; a lane keeps nothing above its
//     lowest full one, and the wavefront stops evaluating once every live lane has a full one (a ballot: wave-uniform).  A
//     child with no candidate is dropped (the prefill stands).  A child whose LOWEST candidate is full is RETIRED, whatever
//     lies above it: w(c) < -thr puts every sample of the child inside k (the premise of instance_mass.hip), and every
//     lower index was dropped by w >= thr or by its window, so it is inside nowhere in the child -- k owns every sample.
//     Any other child is listed (kernels.hpp wg_compact_slots), capped when its highest remaining bit is full.  After the
//     compaction's barriers the wavefront adds the retired lanes' sample counts, one atomic per instance, and walks their
//     ballot: all 64 lanes fill each retired child's extent (clipped to dims in x and y, to the pitch in z) with its index
//     -- side 4: a dword per z run, four children at a time, sixteen lanes each; side >= 16: 16-byte stores, lanes along z
//     first, then y, then x.  Without k.retire nothing ever becomes full: the same kernels, every cell descends.
//   k_voxel_leaf (side 4): a lane is a sample.  Every candidate but a capped top bit is evaluated; id = the lowest inside,
//     else the capped bit, else EMPTY; a lane with z >= nz gives EMPTY.  The four lanes of a z run combine their bytes
//     (quad-permute DPP) and the lane with dz = 0 stores one aligned dword where x and y are in range.  Counts: per
//     instance the ballot of its owners, one atomic per present instance and wavefront.
// Evaluations are counted as the other kernels count them, live lanes x candidates the wavefront evaluated.  The
// accumulators are n + 1 uint64: the samples each instance owns, then the bytes the retired children filled.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the end of
// this file.  What the kernels that walk the volume afterwards rely on: id_volume.hpp.
#include <algorithm>

#include "id_volume.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// what the kernels take beside Args.  There a row's word 1 is z0 | capped << 31, and pairs n_instances + 1 uint64.
struct VoxelArgs {
    Args c;
    uint8_t* volume;                 // [dims x][dims y][pitch], prefilled with kEmpty
    uint32_t pitch;                  // bytes of a z run: dims z rounded up to a multiple of 16
    uint32_t retire;                 // cells: a child whose lowest candidate is provably full is filled and leaves the lists
};
constexpr uint32_t kNone = 64u;      // a lane without a full candidate

struct VoxelRow {
    uint32_t x0, y0, z0;
    uint64_t cand;
    bool capped, have;
};
__device__ __forceinline__ VoxelRow voxel_row(const Args& a)
{
    const CellRow r = cell_row(a);
    return VoxelRow{r.x0, r.y0, r.z0 & 0x7fffffffu, r.mask, (r.z0 >> 31) != 0u, r.have};
}

// the byte offset of sample (x, y, z): 64 bits (65536^2 runs of up to 65536 bytes)
__device__ __forceinline__ size_t voxel_offset(const VoxelArgs& k, uint32_t x, uint32_t y, uint32_t z)
{
    return ((size_t)x * k.c.dims[1] + y) * k.pitch + z;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_voxel_cells(const VoxelArgs k)
{
    extern __shared__ float4 lds[];
    const Args& a = k.c;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const VoxelRow row = voxel_row(a);
    const uint32_t s = a.child_side;
    const ChildLane q = child_lane(a, row, lane);
    const uint32_t x = q.x, y = q.y, z = q.z;
    const bool live = q.live;
    const Point p = child_centre(a, q);
    const float below = k.retire ? -a.thr : -__builtin_inff();   // wave-uniform: nothing is below -inf
    const uint32_t top = row.cand ? 63u - (uint32_t)__builtin_clzll(row.cand) : 0u;
    const uint64_t todo = row.capped ? row.cand & ~(1ull << top) : row.cand;
    uint64_t keep = 0ull;
    uint32_t owner = kNone;                                      // this lane's lowest full candidate: the highest bit of keep
    uint32_t evaluated = 0u;                                     // wave-uniform
    for (uint64_t m = todo; m != 0ull; m &= m - 1ull) {          // wave-uniform, ascending; the one interpreter call site
        if (__ballot(live && owner == kNone) == 0ull) break;     // every live lane has a full candidate below this one
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        ++evaluated;
        const bool open = owner == kNone;                        // (nothing above a full candidate is kept)
        keep |= (open && !(w >= a.thr)) ? 1ull << n : 0ull;      // (a NaN keeps its candidate)
        owner = (open && w < below) ? n : owner;
    }
    if (row.capped && owner == kNone) {                          // the parent's full top candidate is full in every child
        keep |= 1ull << top;
        owner = top;
    }
    // (the store stays spelled out: through a shared function this kernel compiles to other code; the count is its own product)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && evaluated) atomicAdd(a.evaluations, (unsigned long long)__popcll(lives) * evaluated);
    const bool capped = owner != kNone;
    const bool retired = live && capped && (keep & (keep - 1ull)) == 0ull;   // the lowest candidate is the full one
    const bool flag[1] = {live && keep != 0ull && !retired};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), z | (capped ? 0x80000000u : 0u), (uint32_t)keep, (uint32_t)(keep >> 32));
    const uint64_t retiring = __ballot(retired);
    if (retiring == 0ull) return;                                // wave-uniform, after the barriers

    // the samples the retired lanes' owners gain (z clipped to dims) and the bytes their fills write (z clipped to the pitch)
    const uint32_t nx = a.dims[0], ny = a.dims[1], nz = a.dims[2], pitch = k.pitch;
    {
        const uint32_t ex = min(s, nx - min(x, nx - 1u)), ey = min(s, ny - min(y, ny - 1u));
        const unsigned long long area = (unsigned long long)ex * ey;
        const unsigned long long samples = area * min(s, nz - min(z, nz - 1u)), bytes = area * min(s, pitch - min(z, pitch - 1u));
        unsigned long long* counts = static_cast<unsigned long long*>(a.pairs);
        for (uint64_t m = row.cand; m != 0ull; m &= m - 1ull) {  // wave-uniform
            const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
            const bool own = retired && owner == n;
            if (__ballot(own) == 0ull) continue;
            const unsigned long long sum = wave_sum64(own ? samples : 0ull);
            if (lane == 0u) atomicAdd(&counts[n], sum);
        }
        const unsigned long long filled = wave_sum64(retired ? bytes : 0ull);
        if (lane == 0u) atomicAdd(&counts[a.n_instances], filled);
    }

    if (s == 4u) {
        // a z run of a child is one dword (z0 and the pitch are multiples of 4): four retired children a step, sixteen
        // lanes each, lane = 16 q + 4 dx + dy
        const uint32_t q = lane >> 4, dx = (lane >> 2) & 3u, dy = lane & 3u;
        for (uint64_t m = retiring; m != 0ull;) {                // wave-uniform
            uint32_t child = kNone, id = 0u;                     // the retired lane this lane's sixteen fill, and its owner
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const bool more = m != 0ull;
                const uint32_t r = more ? (uint32_t)__builtin_ctzll(m) : 0u;
                const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)owner, (int)r);
                child = (q == i && more) ? r : child;
                id = q == i ? o : id;
                m &= m - 1ull;
            }
            const uint32_t cx = row.x0 + (child >> 4) * 4u + dx, cy = row.y0 + ((child >> 2) & 3u) * 4u + dy;
            const uint32_t cz = row.z0 + (child & 3u) * 4u;
            if (child != kNone && cx < nx && cy < ny)
                *reinterpret_cast<uint32_t*>(k.volume + voxel_offset(k, cx, cy, cz)) = id * 0x01010101u;
        }
        return;
    }
    // s >= 16: z0 and the pitch are multiples of 16, so a z run of a child is whole aligned 16-byte chunks, s / 16 of them
    // before clipping; slot i of a child = (dx * s + dy) * (s / 16) + chunk, lanes along z first
    const uint32_t log_s = 31u - (uint32_t)__builtin_clz(s), log_c = log_s - 4u;
    for (uint64_t m = retiring; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t r = (uint32_t)__builtin_ctzll(m);
        const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)owner, (int)r) * 0x01010101u;
        const uint32_t cx = row.x0 + (r >> 4) * s, cy = row.y0 + ((r >> 2) & 3u) * s, cz = row.z0 + (r & 3u) * s;
        const uint32_t ex = min(s, nx - cx), ey = min(s, ny - cy), ez = min(s, pitch - cz);   // (a retired child is live)
        const uint64_t slots = (uint64_t)ex << (log_s + log_c);
        for (uint64_t i = lane; i < slots; i += 64u) {
            const uint32_t chunk = (uint32_t)i & ((1u << log_c) - 1u), dy = (uint32_t)(i >> log_c) & (s - 1u);
            const uint32_t dx = (uint32_t)(i >> (log_c + log_s));
            if (dy < ey && (chunk << 4) < ez)
                *reinterpret_cast<uint4*>(k.volume + voxel_offset(k, cx + dx, cy + dy, cz + (chunk << 4))) = make_uint4(id, id, id, id);
        }
    }
}

template <bool DO>
__global__ void __launch_bounds__(256) k_voxel_leaf(const VoxelArgs k)
{
    extern __shared__ float4 lds[];
    const Args& a = k.c;
    const VoxelRow row = voxel_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t dz = lane & 3u;
    const LeafLane l = leaf_lane(a, row);
    const uint32_t x = l.x, y = l.y;
    const bool live = l.live;
    const uint32_t top = row.cand ? 63u - (uint32_t)__builtin_clzll(row.cand) : 0u;
    const uint64_t todo = row.capped ? row.cand & ~(1ull << top) : row.cand;
    uint32_t id = kEmpty;
    for (uint64_t m = todo; m != 0ull; m &= m - 1ull) {           // wave-uniform, ascending; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, l.px, l.py, l.pz, lds);
        id = (id == kEmpty && live && w < 0.0f) ? n : id;         // the lowest inside
    }
    // (the count stays spelled out: with its guard through a shared function this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && todo) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(todo)));
    if (row.capped) id = (id == kEmpty && live) ? top : id;       // every sample of the cell is inside the capped candidate
    unsigned long long* counts = static_cast<unsigned long long*>(a.pairs);
    for (uint64_t m = row.cand; m != 0ull; m &= m - 1ull) {       // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint64_t owners = __ballot(id == n);
        if (owners != 0ull && lane == 0u) atomicAdd(&counts[n], (unsigned long long)__popcll(owners));
    }
    // the four lanes of a z run are a quad: byte dz of the run's dword, gathered by two quad permutes
    uint32_t word = id << (8u * dz);
    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0xb1, 0xf, 0xf, false);   // quad_perm:[1,0,3,2]
    word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x4e, 0xf, 0xf, false);   // quad_perm:[2,3,0,1]
    if (dz == 0u && x < a.dims[0] && y < a.dims[1])
        *reinterpret_cast<uint32_t*>(k.volume + voxel_offset(k, x, y, row.z0)) = word;
}

// [leaf][distance_only]
void (*const kVoxelTable[2][2])(VoxelArgs) = {
    {k_voxel_cells<false>, k_voxel_cells<true>},
    {k_voxel_leaf<false>, k_voxel_leaf<true>},
};
HU_BIG_LDS(kVoxelTable);

// What both entry points of the part-id volume check and fill: cells_args() of a strict lattice (every index within
// 16 bits), and a volume whose z runs are `pitch` bytes: a multiple of 16 that holds dims z.
int voxel_args(const hu_cells_launch* l, void* volume_dev, uint32_t pitch, void* acc_dev, VoxelArgs& k)
{
    int rc;
    k = VoxelArgs{};
    if ((rc = cells_args(kStrict, l, k.c))) return rc;
    if (!volume_dev || !acc_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if ((rc = check_pitch(l->dims, pitch))) return rc;
    if (reinterpret_cast<uintptr_t>(volume_dev) % 16u) return hu_fail(HU_ERR_BAD_ARG, "the volume must be aligned to 16 bytes");
    k.volume = static_cast<uint8_t*>(volume_dev);
    k.pitch = pitch;
    k.c.pairs = acc_dev;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_assembly_voxels_cells(const hu_cells_launch* launch, const hu_cells_children* children, int retire, void* volume_dev,
                             uint32_t pitch, void* acc_dev)
{
    VoxelArgs k;
    int rc;
    if ((rc = voxel_args(launch, volume_dev, pitch, acc_dev, k))) return rc;
    if ((rc = cells_children(k.c, children))) return rc;
    if ((rc = check_child_side(k.c.child_side, 4u, 16384u))) return rc;
    if (!std::isfinite(k.c.thr) || k.c.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "thr must be finite and not negative");
    k.retire = retire ? 1u : 0u;
    return cells_launch(kVoxelTable[0][launch->distance_only != 0], k, k.c, *launch, 0u);
}

int hu_assembly_voxels_leaf(const hu_cells_launch* launch, void* volume_dev, uint32_t pitch, void* acc_dev)
{
    VoxelArgs k;
    int rc;
    if ((rc = voxel_args(launch, volume_dev, pitch, acc_dev, k))) return rc;
    k.c.child_side = 1u;
    return cells_launch(kVoxelTable[1][launch->distance_only != 0], k, k.c, *launch, 0u);
}

}  // extern "C"
