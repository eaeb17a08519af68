// codecad_amd/csrc/instance_mass.hip
//
// The MASS PROPERTIES of an assembly (codecad_amd/assembly_mass.py): per visible instance k the ten index sums
//     n, x, y, z, xx, yy, zz, xy, xz, yz
// over V_k, the lattice samples inside k (w_k(p) < 0, strictly, w_k the tape of instance k alone as in instance_pairs.hip),
// and over O_k, the samples inside k and inside no instance of lower index (the owner rule of instance_section.hip's
// part_ids), and the index box of V_k: bit for bit what evaluating every instance at every sample gives.
//
// The traversal is the one of instance_pairs.hip -- cubic cells of 4^k samples, one wavefront per cell, lane = 16 x + 4 y + z
// -- with one more thing a cell knows per instance: that it is FULL, every one of its samples inside.  A row has 32 bytes,
//     {x0 | y0 << 16, z0, cand lo, cand hi, full lo, full hi, 0, 0},    full a subset of cand.
//   k_mass_cells (child side s > 1): a lane is a child cell.  The parent's full candidates are inherited without evaluation;
//     every other candidate is evaluated at the child's centre (the centre formula of k_instance_cells).  The child's samples
//     lie within (s - 1) * step * sqrt(3) / 2 of it and a.thr is more than that (assembly_mass.py), so with |w| no more than
//     the distance to the surface ON BOTH SIDES of it, w >= thr proves that no sample of the child is inside (the candidate
//     is dropped) and w < -thr that all are (the candidate is full); anything else, a NaN included, leaves a boundary
//     candidate.  A child without candidates is dropped; a child whose candidates are all full is RETIRED: each of them gets
//     the closed-form sums over the child's extents, clipped to dims, added to its V sums and box, the lowest of them to
//     its O sums (what is no candidate has no sample inside the child, so the lowest full index owns every sample).  Any
//     other child goes on with both masks (kernels.hpp wg_compact_slots).  Retiring lanes are summed across the wavefront
//     first (wave_sum64): an accumulator word gets at most one atomic per wavefront and instance.  Without kMassRetire in
//     a.flags no candidate ever becomes full: the same kernels, every cell descends to the finest level.
//   k_mass_leaf (side 4): a lane is a sample.  Full candidates are inside without evaluation, the others are evaluated.  Per
//     instance the ballot of the lanes inside it (V) and of those with no lower bit set (O).  The lanes reduce their
//     CELL-LOCAL coordinates 0..3, whose sums and products fit 8 and 10 bits and share three registers; the global sums are
//     rebuilt in uint64 from the cell's origin, wave-uniformly (64 x 65535^2 does not fit 32 bits).
// Evaluations are counted as the other kernels count them, live lanes x candidates evaluated; inherited ones do not count.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry points are at the end of
// this file.
#include <algorithm>

#include "instance_cells.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// the 32-byte row of the cell wavefront `w` of this workgroup takes, or `have` = false past the list's end (wave-uniform)
struct MassRow {
    uint32_t x0, y0, z0;
    uint64_t cand, full;
    bool have;
};
__device__ __forceinline__ MassRow mass_row(const Args& a)
{
    const uint32_t listed = *a.n_parents_dev, n = listed < a.max_parents ? listed : a.max_parents;   // (an overflowed list holds max_parents)
    const uint32_t p = uniform(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    MassRow r{0u, 0u, 0u, 0ull, 0ull, p < n};
    if (r.have) {
        const uint4 head = a.parents[2u * (size_t)p], tail = a.parents[2u * (size_t)p + 1u];
        r.x0 = uniform(head.x & 0xffffu);
        r.y0 = uniform(head.x >> 16);
        r.z0 = uniform(head.y);
        r.cand = ((uint64_t)uniform(head.w) << 32) | uniform(head.z);
        r.full = ((uint64_t)uniform(tail.y) << 32) | uniform(tail.x);
    }
    return r;
}

// ten wave-uniform sums added to an accumulator's ten words by one lane: one atomic per word and wavefront
__device__ __forceinline__ void add_sums(unsigned long long* words, const unsigned long long (&sums)[10], uint32_t lane)
{
    if (lane == 0u)
        for (int i = 0; i < 10; ++i) atomicAdd(&words[i], sums[i]);
}
__device__ __forceinline__ void add_box(MassAcc* acc, const uint32_t (&lo)[3], const uint32_t (&hi)[3], uint32_t lane)
{
    if (lane == 0u)
        for (int k = 0; k < 3; ++k) {
            atomicMin(&acc->lo[k], lo[k]);
            atomicMax(&acc->hi[k], hi[k]);
        }
}

// sum of i and of i^2 over the e indices from x on: e x + e (e - 1) / 2 and e x^2 + x e (e - 1) + (e - 1) e (2 e - 1) / 6
__device__ __forceinline__ void series(uint32_t x, uint32_t e, unsigned long long& first, unsigned long long& second)
{
    const unsigned long long X = x, E = e, pairs = E * (E - 1ull);     // (e >= 1)
    first = E * X + pairs / 2ull;
    second = E * X * X + X * pairs + pairs * (2ull * E - 1ull) / 6ull;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_mass_cells(const Args a)
{
    extern __shared__ float4 lds[];
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const MassRow row = mass_row(a);
    const uint32_t s = a.child_side;
    const ChildLane q = child_lane(a, row, lane);
    const uint32_t x = q.x, y = q.y, z = q.z;
    const bool live = q.live;
    const Point p = child_centre(a, q);
    const float below = (a.flags & kMassRetire) ? -a.thr : -__builtin_inff();   // wave-uniform: nothing is below -inf
    const uint64_t todo = row.cand & ~row.full;
    uint64_t keep = row.full, full = row.full;                   // a full parent's children are full
    for (uint64_t m = todo; m != 0ull; m &= m - 1ull) {          // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        if (!(w >= a.thr)) keep |= 1ull << n;                     // (a NaN keeps its candidate)
        if (w < below) full |= 1ull << n;
    }
    full &= keep;
    // (the count stays spelled out: with its guard through a shared function this kernel compiles to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives && todo) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(todo)));
    const bool retired = live && keep != 0ull && keep == full;
    const bool flag[1] = {live && keep != full};
    uint32_t slot[1];
    wg_compact_slots<1>(flag, a.counter, scratch, slot);         // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity) {
        a.children[2u * (size_t)slot[0]] = make_uint4(x | (y << 16), z, (uint32_t)keep, (uint32_t)(keep >> 32));
        a.children[2u * (size_t)slot[0] + 1u] = make_uint4((uint32_t)full, (uint32_t)(full >> 32), 0u, 0u);
    }
    if (__ballot(retired) == 0ull) return;                        // wave-uniform, after the barriers

    // the closed-form sums of this lane's child over its extents clipped to dims
    const uint32_t ex = min(s, a.dims[0] - min(x, a.dims[0] - 1u)), ey = min(s, a.dims[1] - min(y, a.dims[1] - 1u)),
                   ez = min(s, a.dims[2] - min(z, a.dims[2] - 1u));
    unsigned long long x1, x2, y1, y2, z1, z2;
    series(x, ex, x1, x2);
    series(y, ey, y1, y2);
    series(z, ez, z1, z2);
    const unsigned long long EX = ex, EY = ey, EZ = ez;
    const unsigned long long mine[10] = {EX * EY * EZ, x1 * EY * EZ, EX * y1 * EZ, EX * EY * z1, x2 * EY * EZ, EX * y2 * EZ,
                                         EX * EY * z2, x1 * y1 * EZ, x1 * EY * z1, EX * y1 * z1};
    MassAcc* accs = static_cast<MassAcc*>(a.pairs);
    const uint32_t origin[3] = {row.x0, row.y0, row.z0};
    for (uint64_t m = row.cand; m != 0ull; m &= m - 1ull) {      // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const bool in = retired && ((full >> n) & 1ull) != 0ull;
        const uint64_t bv = __ballot(in);
        if (bv == 0ull) continue;
        const bool own = in && (full & ((1ull << n) - 1ull)) == 0ull;
        const uint64_t bo = __ballot(own);
        unsigned long long sums[10];
        for (int i = 0; i < 10; ++i) sums[i] = wave_sum64(in ? mine[i] : 0ull);
        uint32_t lo[3], hi[3];
        mask_box(bv, lo, hi);
        for (int k = 0; k < 3; ++k) {
            lo[k] = origin[k] + lo[k] * s;
            hi[k] = min(origin[k] + hi[k] * s + (s - 1u), a.dims[k] - 1u);
        }
        add_sums(accs[n].v, sums, lane);
        add_box(accs + n, lo, hi, lane);
        if (bo == 0ull) continue;
        if (bo != bv)
            for (int i = 0; i < 10; ++i) sums[i] = wave_sum64(own ? mine[i] : 0ull);
        add_sums(accs[n].o, sums, lane);
    }
}

// the ten sums of the samples of the ballot `b` (this lane: `in`) of the cell at `origin`, from the lanes' packed cell-local
// coordinates: p1 = dx | dy << 8 | dz << 16, p2 = dx^2 | dy^2 << 10 | dz^2 << 20, p3 = dx dy | dx dz << 10 | dy dz << 20
__device__ __forceinline__ void leaf_sums(bool in, uint64_t b, uint32_t p1, uint32_t p2, uint32_t p3, const uint32_t (&origin)[3],
                                          unsigned long long (&sums)[10])
{
    const uint32_t s1 = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_last_lane(in ? p1 : 0u), 63);
    const uint32_t s2 = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_last_lane(in ? p2 : 0u), 63);
    const uint32_t s3 = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum_to_last_lane(in ? p3 : 0u), 63);
    const unsigned long long n = (unsigned long long)__popcll(b), X = origin[0], Y = origin[1], Z = origin[2];
    const unsigned long long dx = s1 & 0xffu, dy = (s1 >> 8) & 0xffu, dz = (s1 >> 16) & 0xffu;
    const unsigned long long dxx = s2 & 0x3ffu, dyy = (s2 >> 10) & 0x3ffu, dzz = (s2 >> 20) & 0x3ffu;
    const unsigned long long dxy = s3 & 0x3ffu, dxz = (s3 >> 10) & 0x3ffu, dyz = (s3 >> 20) & 0x3ffu;
    sums[0] = n;
    sums[1] = n * X + dx;
    sums[2] = n * Y + dy;
    sums[3] = n * Z + dz;
    sums[4] = n * X * X + 2ull * X * dx + dxx;
    sums[5] = n * Y * Y + 2ull * Y * dy + dyy;
    sums[6] = n * Z * Z + 2ull * Z * dz + dzz;
    sums[7] = n * X * Y + X * dy + Y * dx + dxy;
    sums[8] = n * X * Z + X * dz + Z * dx + dxz;
    sums[9] = n * Y * Z + Y * dz + Z * dy + dyz;
}

template <bool DO>
__global__ void __launch_bounds__(256) k_mass_leaf(const Args a)
{
    extern __shared__ float4 lds[];
    const MassRow row = mass_row(a);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    // (the lane and the count stay spelled out: with instance_cells.hpp leaf_lane or a shared count this kernel compiles to other code)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t dx = lane >> 4, dy = (lane >> 2) & 3u, dz = lane & 3u;
    const uint32_t x = row.x0 + dx, y = row.y0 + dy, z = row.z0 + dz;
    const bool live = (x < a.dims[0]) & (y < a.dims[1]) & (z < a.dims[2]);
    // exactly kernels.hpp sample() (the lattice of oracle.grid_eval)
    const float px = sample(a.corner[0], a.step, x), py = sample(a.corner[1], a.step, y), pz = sample(a.corner[2], a.step, z);
    const uint64_t todo = row.cand & ~row.full;
    uint64_t inside = live ? row.full : 0ull, present = row.full;  // per lane; wave-uniform (a row's first sample is live)
    for (uint64_t m = todo; m != 0ull; m &= m - 1ull) {           // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const float w = instance_dist<DO>(a, n, px, py, pz, lds);
        const bool in = live & (w < 0.0f);
        inside |= in ? 1ull << n : 0ull;
        present |= __ballot(in) ? 1ull << n : 0ull;
    }
    const uint64_t lives = __ballot(live);
    if (lane == 0u && todo) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(todo)));
    const uint32_t p1 = dx | (dy << 8) | (dz << 16);
    const uint32_t p2 = (dx * dx) | ((dy * dy) << 10) | ((dz * dz) << 20);
    const uint32_t p3 = (dx * dy) | ((dx * dz) << 10) | ((dy * dz) << 20);
    MassAcc* accs = static_cast<MassAcc*>(a.pairs);
    const uint32_t origin[3] = {row.x0, row.y0, row.z0};
    for (uint64_t m = present; m != 0ull; m &= m - 1ull) {        // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const bool in = ((inside >> n) & 1ull) != 0ull;
        const uint64_t bv = __ballot(in);
        if (bv == 0ull) continue;                                 // (a full candidate has every live lane)
        const bool own = in && (inside & ((1ull << n) - 1ull)) == 0ull;
        const uint64_t bo = __ballot(own);
        unsigned long long sums[10];
        leaf_sums(in, bv, p1, p2, p3, origin, sums);
        uint32_t lo[3], hi[3];
        mask_box(bv, lo, hi);
        for (int k = 0; k < 3; ++k) {
            lo[k] += origin[k];
            hi[k] += origin[k];
        }
        add_sums(accs[n].v, sums, lane);
        add_box(accs + n, lo, hi, lane);
        if (bo == 0ull) continue;
        if (bo != bv) leaf_sums(own, bo, p1, p2, p3, origin, sums);
        add_sums(accs[n].o, sums, lane);
    }
}

// [leaf][distance_only]
void (*const kMassTable[2][2])(Args) = {
    {k_mass_cells<false>, k_mass_cells<true>},
    {k_mass_leaf<false>, k_mass_leaf<true>},
};
HU_BIG_LDS(kMassTable);

// What both entry points of the assembly's mass properties check and fill: cells_args() of a strict lattice (every index
// within 16 bits), and what the sums need beyond it: a lattice whose second-moment sums fit 64 bits.
int mass_args(const hu_cells_launch* l, void* acc_dev, Args& a)
{
    int rc;
    if ((rc = cells_args(kStrict, l, a))) return rc;
    if (!acc_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    const uint32_t* dims = l->dims;
    const uint64_t longest = std::max(dims[0], std::max(dims[1], dims[2])) - 1u;
    const unsigned __int128 bound = (unsigned __int128)dims[0] * dims[1] * dims[2] * longest * longest;
    if (bound >> 64) return hu_fail(HU_ERR_BAD_ARG, "the lattice's second-moment index sums would not fit 64 bits");
    a.pairs = acc_dev;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_assembly_mass_cells(const hu_cells_launch* launch, const hu_cells_children* children, int retire, void* acc_dev)
{
    Args a;
    int rc;
    if ((rc = mass_args(launch, acc_dev, a))) return rc;
    if ((rc = cells_children(a, children))) return rc;
    if ((rc = check_child_side(a.child_side, 4u, 16384u))) return rc;
    if (!std::isfinite(a.thr) || a.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "thr must be finite and not negative");
    if (a.max_parents > 0x7fffffffu || a.capacity > 0x7fffffffu) return hu_fail(HU_ERR_BAD_ARG, "a list of 32-byte rows holds fewer than 2^31");
    a.flags = retire ? kMassRetire : 0u;
    return cells_launch(kMassTable[0][launch->distance_only != 0], a, a, *launch, 0u);
}

int hu_assembly_mass_leaf(const hu_cells_launch* launch, void* acc_dev)
{
    Args a;
    int rc;
    if ((rc = mass_args(launch, acc_dev, a))) return rc;
    if (a.max_parents > 0x7fffffffu) return hu_fail(HU_ERR_BAD_ARG, "a list of 32-byte rows holds fewer than 2^31");
    a.child_side = 1u;
    return cells_launch(kMassTable[1][launch->distance_only != 0], a, a, *launch, 0u);
}

}  // extern "C"
