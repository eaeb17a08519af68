// codecad_amd/csrc/instance_contacts.hip
//
// WHICH PARTS TOUCH, OVER HOW MANY FACES AND WHERE, on the part-id volume of an assembly, for codecad_amd/contacts.py.  The
// FACE of axis a at sample p lies between p and p + e_a and counts for a pair only when both samples are in the lattice.  For an
// ordered pair i != j of parts
//   C_a[i][j] = { p : ids[p] = i, ids[p + e_a] = j }                         (j lies right above i),
// and a ROW of the table holds, per (a, i, j): |C|, the sums of p per axis, the lowest and highest p per axis and the
// lexicographically first p as the KEY x << 32 | y << 16 | z.  The lows and the key are stored COMPLEMENTED, so that a table of
// zeros is the empty table and every update is an atomicAdd or an atomicMax (the trick of CompRow, instance_components.hip).
//   EXPOSED [a][0][i]: the p with ids[p] = i and p + e_a empty or outside the lattice; [a][1][i]: the same with p - e_a.
//   INTERFACE SAMPLE: ids[p] = i != 255 and some in-lattice 6-neighbour q with ids[q] not in {i, 255}.
// All integers, exact, independent of the order anything ran in.  Nothing outside the lattice is inside any part, and no byte
// of the padding z in [nz, pitch) is read or written.
//
// k_contact_faces: LANES LIE ALONG z; a UNIT is 64 consecutive z of one (x, y) column (id_volume.hpp), walked a grid apart.  A
// lane holds its own id and the ids of its six neighbours: the x and y neighbours are the same 64 bytes of the four adjacent
// columns (255 beyond the lattice, a wave-uniform test), the z neighbours come by cross-lane reads, and lane 0 and lane 63 fetch
// the one byte across the word edge where that byte lies inside nz.  Per axis a lane whose upper neighbour is another part holds
// the PAIR CODE i << 6 | j.  The wavefront loops over the distinct codes present (wave-uniform, as gather_counts does over ids)
// and forms a code's count, sums, box and key from its ballot alone: popcount, ctz, clz and the sum of the set lane positions.
// THE ATOMICS ARE BOUNDED BY WHAT CHANGES, NOT BY WHAT IS THERE: per axis the wavefront keeps the code it met last with its
// partial row in wave-uniform registers and writes it out -- eleven atomics in three instructions, a lane each -- only when
// another code arrives or its walk ends.  An interface normal to an axis, which gives every unit on it the same code, so costs a
// wavefront one row update, not one a unit.  The exposed and interface counts are gathered per lane-as-part and added once at
// the end.  No private array, no LDS, no scratch.  The entry point is at the end of this file.
#include "id_volume.hpp"

using namespace hu_cells;

namespace {

constexpr uint32_t kParts = HU_CONTACT_MAX_PARTS;       // the table is ContactRow[3][kParts][kParts]
constexpr uint32_t kNoCode = ~0u;                       // no pair: a code is at most 63 << 6 | 63
static_assert(kParts == 64u, "include/hip_util.h; a lane per part, six bits per part of a pair code");

struct ContactRow {                                     // include/hip_util.h: 64 bytes
    unsigned long long count;
    unsigned long long sums[3];
    unsigned long long not_key;                         // ~(x << 32 | y << 16 | z) of the lexicographically first p
    uint32_t not_lo[3];                                 // ~(the lowest p per axis)
    uint32_t hi[3];
};
static_assert(sizeof(ContactRow) == 64, "include/hip_util.h");

struct ContactArgs {
    const uint8_t* ids;                 // uint8[nx][ny][pitch]
    uint8_t* contact;                   // the same shape, or NULL
    ContactRow* rows;                   // [3][kParts][kParts]
    unsigned long long* counts;         // [7][64]: exposed [a][0], [a][1] per axis a, then the interface samples
    uint32_t nx, ny, nz, pitch;
    uint32_t n;
    uint32_t na;                        // (lattice_axis: nz)
    uint32_t segments;                  // ceil(nz / 64)
};

// the id at `at`; anything that is no part of the table counts as empty
__device__ __forceinline__ uint32_t id_at(const uint8_t* at, uint32_t n)
{
    const uint32_t id = *at;
    return id < n ? id : kEmpty;
}

// the sum of the positions of the set bits of `b`: bit k of a position weighs 2^k
__device__ __forceinline__ uint32_t position_sum(uint64_t b)
{
    return (uint32_t)__popcll(b & 0xaaaaaaaaaaaaaaaaull) + ((uint32_t)__popcll(b & 0xccccccccccccccccull) << 1)
         + ((uint32_t)__popcll(b & 0xf0f0f0f0f0f0f0f0ull) << 2) + ((uint32_t)__popcll(b & 0xff00ff00ff00ff00ull) << 3)
         + ((uint32_t)__popcll(b & 0xffff0000ffff0000ull) << 4) + ((uint32_t)__popcll(b & 0xffffffff00000000ull) << 5);
}

// what a wavefront has met of one pair on one axis and not written out yet (every field wave-uniform)
struct Pending {
    uint32_t code;                      // i << 6 | j, or kNoCode
    unsigned long long count, sx, sy, sz, key;
    uint32_t lox, loy, loz, hix, hiy, hiz;
};

__device__ __forceinline__ void flush(const ContactArgs& a, uint32_t axis, uint32_t lane, const Pending& p)
{
    if (p.code == kNoCode) return;                                    // wave-uniform
    ContactRow* row = a.rows + ((size_t)axis * kParts * kParts + p.code);         // [axis][i][j]: i * 64 + j is the code
    unsigned long long* wide = &row->count;                           // count, sums[3], not_key
    uint32_t* narrow = row->not_lo;                                   // not_lo[3], hi[3]
    if (lane < 4u)
        atomicAdd(wide + lane, lane == 0u ? p.count : lane == 1u ? p.sx : lane == 2u ? p.sy : p.sz);
    else if (lane == 4u)
        atomicMax(wide + 4, ~p.key);
    else if (lane < 11u)
        atomicMax(narrow + (lane - 5u), lane == 5u ? ~p.lox : lane == 6u ? ~p.loy : lane == 7u ? ~p.loz
                                      : lane == 8u ? p.hix : lane == 9u ? p.hiy : p.hiz);
}

// the lanes with `has` hold `code`, the pair of their sample and the one above it on `axis`; they are samples z0 + lane of column (x, y)
__device__ __forceinline__ void meet(const ContactArgs& a, uint32_t axis, uint32_t lane, Pending& p, bool has, uint32_t code,
                                     uint32_t x, uint32_t y, uint32_t z0)
{
    for (uint64_t todo = __ballot(has); todo != 0ull;) {              // wave-uniform: the distinct codes present
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)__builtin_ctzll(todo));
        const uint64_t b = __ballot(has && code == c);
        todo &= ~b;
        const uint32_t k = (uint32_t)__popcll(b);
        const uint32_t zlo = z0 + (uint32_t)__builtin_ctzll(b), zhi = z0 + 63u - (uint32_t)__builtin_clzll(b);
        const unsigned long long key = ((unsigned long long)x << 32) | ((unsigned long long)y << 16) | zlo;
        if (c != p.code) {                                            // another code arrives: the last one is written out
            flush(a, axis, lane, p);
            p.code = c, p.count = 0ull, p.sx = p.sy = p.sz = 0ull, p.key = key;
            p.lox = x, p.loy = y, p.loz = zlo, p.hix = x, p.hiy = y, p.hiz = zhi;
        }
        p.count += k, p.sx += (unsigned long long)x * k, p.sy += (unsigned long long)y * k;
        p.sz += (unsigned long long)z0 * k + position_sum(b);
        p.key = key < p.key ? key : p.key;
        p.lox = min(p.lox, x), p.loy = min(p.loy, y), p.loz = min(p.loz, zlo);
        p.hix = max(p.hix, x), p.hiy = max(p.hiy, y), p.hiz = max(p.hiz, zhi);
    }
}

__device__ __forceinline__ uint32_t pair_code(uint32_t id, uint32_t above)
{
    return id != kEmpty && above != kEmpty && above != id ? id << 6 | above : kNoCode;
}

__global__ void __launch_bounds__(256) k_contact_faces(const ContactArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    Pending px{kNoCode}, py{kNoCode}, pz{kNoCode};
    unsigned long long ex0 = 0ull, ex1 = 0ull, ey0 = 0ull, ey1 = 0ull, ez0 = 0ull, ez1 = 0ull, met = 0ull;   // of part `lane`
    const size_t plane = (size_t)a.ny * a.pitch;
    HU_FOR_UNITS(unit, (uint64_t)a.nx * a.ny * a.segments) {
        const ColumnUnit u = column_unit(a, unit);
        const uint32_t z = u.z0 + lane;
        const bool active = z < a.nz;
        const uint8_t* at = a.ids + u.base + z;
        const uint32_t id = active ? id_at(at, a.n) : kEmpty;
        // the neighbours: 255 beyond the lattice (wave-uniform tests on x and y)
        const uint32_t xm = active && u.x > 0u ? id_at(at - plane, a.n) : kEmpty;
        const uint32_t xp = active && u.x + 1u < a.nx ? id_at(at + plane, a.n) : kEmpty;
        const uint32_t ym = active && u.y > 0u ? id_at(at - a.pitch, a.n) : kEmpty;
        const uint32_t yp = active && u.y + 1u < a.ny ? id_at(at + a.pitch, a.n) : kEmpty;
        const uint32_t from_below = (uint32_t)__shfl_up((int)id, 1), from_above = (uint32_t)__shfl_down((int)id, 1);   // (every lane takes part)
        uint32_t zm = from_below, zp = from_above;                    // (a lane past nz holds 255)
        if (lane == 0u) zm = u.z0 > 0u ? id_at(at - 1, a.n) : kEmpty;                // z0 - 1 < nz
        if (lane == 63u) zp = u.z0 + 64u < a.nz ? id_at(at + 1, a.n) : kEmpty;       // z0 + 64 < nz: the byte is data
        const bool solid = id != kEmpty;
        meet(a, 0u, lane, px, pair_code(id, xp) != kNoCode, pair_code(id, xp), u.x, u.y, u.z0);
        meet(a, 1u, lane, py, pair_code(id, yp) != kNoCode, pair_code(id, yp), u.x, u.y, u.z0);
        meet(a, 2u, lane, pz, pair_code(id, zp) != kNoCode, pair_code(id, zp), u.x, u.y, u.z0);
        gather_counts(solid && xp == kEmpty, id, lane, ex0);
        gather_counts(solid && xm == kEmpty, id, lane, ex1);
        gather_counts(solid && yp == kEmpty, id, lane, ey0);
        gather_counts(solid && ym == kEmpty, id, lane, ey1);
        gather_counts(solid && zp == kEmpty, id, lane, ez0);
        gather_counts(solid && zm == kEmpty, id, lane, ez1);
        const auto other = [id](uint32_t q) { return q != kEmpty && q != id; };
        const bool meets = solid && (other(xm) || other(xp) || other(ym) || other(yp) || other(zm) || other(zp));
        gather_counts(meets, id, lane, met);
        if (a.contact && active) a.contact[u.base + z] = (uint8_t)(meets ? id : kEmpty);
    }
    flush(a, 0u, lane, px), flush(a, 1u, lane, py), flush(a, 2u, lane, pz);
    if (ex0 != 0ull) atomicAdd(&a.counts[lane], ex0);
    if (ex1 != 0ull) atomicAdd(&a.counts[64u + lane], ex1);
    if (ey0 != 0ull) atomicAdd(&a.counts[128u + lane], ey0);
    if (ey1 != 0ull) atomicAdd(&a.counts[192u + lane], ey1);
    if (ez0 != 0ull) atomicAdd(&a.counts[256u + lane], ez0);
    if (ez1 != 0ull) atomicAdd(&a.counts[320u + lane], ez1);
    if (met != 0ull) atomicAdd(&a.counts[384u + lane], met);
}

}  // namespace

extern "C" {

int hu_contact_faces(const void* ids_dev, void* contact_ids_dev, void* rows_dev, uint64_t* counts_dev, const uint32_t dims[3],
                     uint32_t pitch, uint32_t n, void* stream)
{
    if (!ids_dev || !rows_dev || !counts_dev || !dims) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (reinterpret_cast<uintptr_t>(rows_dev) % 8u || reinterpret_cast<uintptr_t>(counts_dev) % 8u)
        return hu_fail(HU_ERR_BAD_ARG, "the rows and the counts must be aligned to 8 bytes");
    ContactArgs a{};
    if (int rc = lattice_of(dims, pitch, a)) return rc;
    if (int rc = lattice_axis(2, a)) return rc;
    if (n == 0u || n > kParts) return hu_fail(HU_ERR_BAD_ARG, "n must be in 1..64");
    a.ids = static_cast<const uint8_t*>(ids_dev);
    a.contact = static_cast<uint8_t*>(contact_ids_dev);
    a.rows = static_cast<ContactRow*>(rows_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    a.n = n;
    // four units a wavefront at the least; the bounded grid bounds the row updates of an interface that every unit meets
    const uint64_t units = (uint64_t)a.nx * a.ny * a.segments;
    hipLaunchKernelGGL(k_contact_faces, dim3(walking_blocks(units, 4u)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}

}  // extern "C"
