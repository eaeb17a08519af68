// codecad_amd/csrc/id_volume.hpp -- the PART-ID VOLUME of an assembly and what the kernels that walk it share.
//
// THE CONTRACT.  instance_voxels.hip fills a uint8[nx][ny][pitch] volume on the device, x slowest: the byte of sample (x, y, z) is
// the index of the part that owns it, 255 (kEmpty) where it is inside no part.  pitch is nz rounded up to a multiple of 16; the
// PADDING z in [nz, pitch) is never read as data.  Every dimension is at most 65536, so the volume may hold 2^48 bytes: BYTE
// OFFSETS ARE 64-BIT.  Nothing outside the lattice is inside any part.  A kernel takes the lattice in its argument struct as
// uint32 nx, ny, nz, pitch and, where it walks units, segments and na, under these names: the structs keep their own layout (the
// order of a kernel's arguments decides how its scalar loads pair up).  Lanes lie along z; workgroups are four wavefronts
// (but for instance_local.hip's kernels over wide windows, which take 8 and 16 to keep a compute unit's wavefronts up).
#pragma once

#include "instance_cells.hpp"

namespace hu_cells {

constexpr uint32_t kEmpty = 255u;                       // the id of a sample inside no part
constexpr uint32_t kSolid = HU_THICKNESS_SOLID;         // of: S is id != 255; any other of (<= 63): S is id == of
static_assert(kSolid == kEmpty && HU_OVERHANG_SOLID == kSolid, "include/hip_util.h");

__device__ __forceinline__ bool in_set(uint32_t id, uint32_t of) { return of == kSolid ? id != kEmpty : id == of; }

// lane p's `mine` += the lanes that count and whose id is p, for every id present (wave-uniform loop)
__device__ __forceinline__ void gather_counts(bool counted, uint32_t id, uint32_t lane, unsigned long long& mine)
{
    for (uint64_t todo = __ballot(counted); todo != 0ull;) {
        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)__builtin_ctzll(todo));
        const uint64_t b = __ballot(counted && id == p);
        todo &= ~b;
        if (lane == (p & 63u)) mine += (unsigned long long)__popcll(b);
    }
}

// unit `unit` of nx * ny * segments: 64 consecutive z, from z0 on, of column (x, y), whose bytes start at `base` (wave-uniform)
struct ColumnUnit {
    uint32_t x, y, z0;
    size_t base;
};
template <class A> __device__ __forceinline__ ColumnUnit column_unit(const A& a, uint64_t unit)
{
    const uint64_t column = unit / a.segments;
    ColumnUnit u;
    u.z0 = ((uint32_t)(unit - column * a.segments)) << 6;
    u.x = (uint32_t)(column / a.ny), u.y = (uint32_t)(column - (uint64_t)u.x * a.ny);
    u.base = (size_t)column * a.pitch;
    return u;
}

// unit `unit` of line_units(a), axis 0 or 1: 64 consecutive z of the LINES of one y (along x) or one x (along y); lane `lane`
// has z, and its sample of layer index t along the axis is the byte base + t * stride (`line` is wave-uniform, z may be >= nz)
template <class I> struct LineUnitOf {
    uint32_t line, z;
    I base, stride;
};
using LineUnit = LineUnitOf<size_t>;
// (device and host: at most 65536 lines of 1024 words)
template <class A> __host__ __device__ __forceinline__ uint64_t line_units(const A& a) { return (uint64_t)(a.axis == 0u ? a.ny : a.nx) * a.segments; }
template <class I = size_t, class A> __device__ __forceinline__ LineUnitOf<I> line_unit(const A& a, uint64_t unit, uint32_t lane)
{
    LineUnitOf<I> u;
    u.line = (uint32_t)(unit / a.segments);
    u.z = (((uint32_t)(unit - (uint64_t)u.line * a.segments)) << 6) + lane;
    u.stride = a.axis == 0u ? (I)a.ny * a.pitch : (I)a.pitch;
    u.base = (a.axis == 0u ? (I)u.line * a.pitch : (I)u.line * a.ny * a.pitch) + u.z;
    return u;
}

// a wavefront takes the units w, w + W, w + 2 W, ... of `units`, W the wavefronts of the grid (wave-uniform), and gathers over all
#define HU_FOR_UNITS(unit, units) \
    for (uint64_t unit = (uint64_t)blockIdx.x * 4u + hu_cells::uniform(threadIdx.x >> 6); unit < (units); unit += (uint64_t)gridDim.x * 4u)

// THE UNION-FIND over a uint32 label volume (instance_components.hip states THE INVARIANT: label[q] <= q, entries only ever fall,
// labels are buffer indices), for every kernel that labels: the components, and the layers of instance_reach.hip.
// The root of p: labels strictly decrease along the walk (THE INVARIANT, label[p] <= p), so it ends.  A value read here may
// be stale (a plain load may be served by L1 while another workgroup's atomic has lowered the entry since): a stale parent
// is still an ancestor -- whoever replaced the link p -> v took on uniting v with what it wrote --, so the walk still ends
// in p's component, merely not at its newest root.  unite() does not rest on it.
__device__ __forceinline__ uint32_t find(const uint32_t* label, uint32_t p)
{
    for (uint32_t l; (l = label[p]) != p; p = l) {}
    return p;
}

// Unites the components of a and b.  The value atomicMin RETURNS decides, never a plain load: old == a says a was a root
// and now points to b (done); anything else says label[a] was old < a already, and whether the atomic replaced it by b
// (old > b) or left it (old <= b), what remains is to unite old with b -- retried from the returned value.  max(a, b)
// strictly decreases from one iteration to the next (old < a by THE INVARIANT), every iteration progresses on this lane's
// own values, and label[a] is only ever lowered.
__device__ __forceinline__ void unite(uint32_t* label, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find(label, a);
        b = find(label, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(&label[a], b);
        if (old == a) return;
        a = old;
    }
}

// THE FLAG OF A ROOT, for the kernels that hand a property of whole layer components on from layer to layer over a flattened
// label volume of at most 2^31 entries: instance_reach.hip, for the escape of drainage and the grounding of islands.
constexpr uint32_t kFlag = 0x80000000u;     // a root's entry: index | kFlag once its component escapes

// an entry as the L2 holds it: flags are set by other workgroups while a kernel runs.  A stale one would cost an atomic or a
// pass, never a result.
__device__ __forceinline__ uint32_t live(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Is the root of the sample q of E, whose entry reads l != kNone, flagged?  After the flatten an entry is its root's index; a
// root's own entry is its index, with kFlag once it escapes.
__device__ __forceinline__ bool escapes(const uint32_t* labels, uint32_t l, uint32_t q)
{
    if (l & kFlag) return true;
    if (l == q) return false;
    return (live(labels + l) & kFlag) != 0u;
}

// The lanes of `want` flag their roots r (indices, no flag in them) -> this lane's atomic found the flag unset.  DISTINCT: no two
// lanes share a root (they lie in different layers); else one atomic per distinct root, issued by the first lane that has it.
template <bool DISTINCT>
__device__ __forceinline__ bool raise(uint32_t* labels, uint32_t lane, bool want, uint32_t r)
{
    bool fresh = false;
    if (DISTINCT) {
        if (want) fresh = (atomicOr(labels + r, kFlag) & kFlag) == 0u;
    } else {
        for (uint64_t todo = __ballot(want); todo != 0ull;) {              // wave-uniform
            const uint32_t first = (uint32_t)__builtin_ctzll(todo);
            const uint32_t root = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)first);
            todo &= ~__ballot(want && r == root);
            if (lane == first) fresh = (atomicOr(labels + root, kFlag) & kFlag) == 0u;
        }
    }
    return fresh;
}

// host side (`dims` is not NULL): the checks, and the fill of the lattice's fields
inline int check_pitch(const uint32_t dims[3], uint32_t pitch)
{
    if (pitch % 16u || pitch < dims[2] || pitch > 65536u)
        return hu_fail(HU_ERR_BAD_ARG, "pitch must be a multiple of 16 from dims[2] to 65536");
    return HU_OK;
}
template <class A> int lattice_of(const uint32_t dims[3], uint32_t pitch, A& a)
{
    for (int i = 0; i < 3; ++i)
        if (dims[i] == 0u || dims[i] > 65536u) return hu_fail(HU_ERR_BAD_ARG, "lattice dims must be in 1..65536");
    a.nx = dims[0], a.ny = dims[1], a.nz = dims[2], a.pitch = pitch;
    return check_pitch(dims, pitch);
}
template <class A> int lattice_axis(int axis, A& a)
{
    if (axis < 0 || axis > 2) return hu_fail(HU_ERR_BAD_ARG, "axis must be 0 (x), 1 (y) or 2 (z)");
    a.na = axis == 0 ? a.nx : axis == 1 ? a.ny : a.nz, a.segments = (a.nz + 63u) / 64u;
    return HU_OK;
}
// `solid`: the name of kSolid in the caller's part of include/hip_util.h
inline int check_of(uint32_t of, const char* solid)
{
    if (of > 63u && of != kSolid) return hu_fail(HU_ERR_BAD_ARG, std::string("of must be an instance index up to 63 or ") + solid);
    return HU_OK;
}

// blocks for HU_FOR_UNITS: `per_wavefront` units a wavefront at the least, so that small lattices walk too, and at most
// kMaxBlocks -- eight a compute unit of 256 --, which bounds the atomics on one accumulator whatever the lattice
constexpr uint64_t kMaxBlocks = 2048u;
inline uint32_t walking_blocks(uint64_t units, uint32_t per_wavefront)
{
    const uint64_t blocks = (units + 4u * per_wavefront - 1u) / (4u * per_wavefront);
    return (uint32_t)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace hu_cells
