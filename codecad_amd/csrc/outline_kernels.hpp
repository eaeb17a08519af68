// codecad_amd/csrc/outline_kernels.hpp -- the ONE body of the outline kernels: instance_outline.hip (a section's outlines,
// OutlineArgs) and instance_layers.hip (the same on a stack of parallel planes, LayerArgs) wrap it in their kernels.
//
// The OUTLINES of an assembly's section (codecad_amd/section_outlines.py): per instance k, the marching-squares contour of
// w_k on the section's lattice (instance_section.hip) with a ring of samples around it.  Samples carry the SHIFTED index
// s = (i + 1, j + 1), 0 .. nu + 1 by 0 .. nv + 1, and sit at plane_point((float)s - 1) -- the section's position formula,
// evaluated at -1 and at the section's dims too.  SQUARE (a, b), 0 <= a <= nu, 0 <= b <= nv, has the corner samples
// s = (a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1) and the edges 0 bottom, 1 right, 2 top, 3 left, each from its
// lower-index sample p to its higher-index sample q.  Inside is w < 0, strictly.  Instance k crosses an edge when exactly
// one of p, q is inside, at t = w_p / (w_p - w_q): one binary32 subtraction and one correctly rounded binary32 division
// (both units are built with -fhip-fp32-correctly-rounded-divide-sqrt like every other: the plain `/`), 0.5 where that is
// no number.  A square has 0, 1 or 2 SEGMENTS per instance, from a crossed edge to a crossed edge with the inside on the
// left (u to the right, v up); diagonal inside corners give two, each cutting off one inside corner.  A segment is a
// 16-byte record {a | b << 16, record_word(k, e_from, e_to), t_from, t_to}.
//
// Args describes the lattice of SQUARES here: dims = {nu + 1, nv + 1, 1}, a row is a tile {a0 | b0 << 16, word 1, mask lo,
// mask hi} of 8^k x 8^k squares, windows (n x 6) the squares an instance may cross.  One WAVEFRONT takes one tile.
//   outline_tiles (child side S >= 8): lane 8 i + j is the child at (a0 + i S, b0 + j S).  Every candidate is evaluated
//     at the child's centre, the shifted index a + S / 2 per axis.  The child's corner samples lie within S * step *
//     sqrt(2) / 2 of it; r = a.thr is (S + 1) * step * sqrt(2) / 2 times (1 + 2^-10), the slack of the section's tiles.
//     w >= r: outside at every corner sample; w <= -r: inside at every one -- no crossing either way.  A child keeps k when
//     its window reaches the child and neither holds; a value that is no number keeps its candidate.
//   outline_leaf (8 x 8 squares, 9 x 9 samples): per candidate, the 64 samples s = (a0 + i, b0 + j) on lane 8 j + i, then
//     the 17 of the tile's far rim on lanes 0..16, through the ONE interpreter call site; the 81 values go to the
//     wavefront's own 128 floats of LDS after the register file, each lane reads its square's four, forms 0-2 records and
//     places them with a ballot prefix: one atomic on the segment counter and one on the instance's count per wavefront
//     and candidate.  Records at or past the capacity are counted and not stored.
//
// WHAT THE TWO DIFFER IN is four overloaded hooks, resolved at compile time (the section's path decides nothing at run time):
//                      OutlineArgs                         LayerArgs
//   outline_row        cell_row() as it is                 absent too when word 1, the row's LAYER, is not below n_layers
//   plane_corner       c.corner, a kernel argument         layer_corners[layer] through constant_uniform: one scalar load
//   child_word         0                                   the layer: children inherit it
//   record_word        k | e_from << 8 | e_to << 16        k | e_from << 8 | e_to << 10 | layer << 12
// The registers of the eight kernels are recorded in DESIGN.md section 9; the host tests of both units read them from the ISA.
#pragma once

#include "instance_cells.hpp"

namespace hu_cells {

// the row of this wavefront: absent (`have` false, mask 0, layer 0) past the list's end and where it names no layer
__device__ __forceinline__ CellRow outline_row(const OutlineArgs& t) { return cell_row(t.c); }
__device__ __forceinline__ CellRow outline_row(const LayerArgs& t)
{
    CellRow row = cell_row(t.c);
    row.have &= row.z0 < t.n_layers;                              // wave-uniform; a row of no layer is no row
    return row.have ? row : CellRow{row.x0, row.y0, 0u, 0ull, false};   // (n_layers >= 1: the corner of layer 0 exists)
}

// the 3D position of the section's sample (0, 0) on the row's plane (wave-uniform)
__device__ __forceinline__ float4 plane_corner(const OutlineArgs& t, const CellRow&) { return make_float4(t.c.corner[0], t.c.corner[1], t.c.corner[2], 0.0f); }
__device__ __forceinline__ float4 plane_corner(const LayerArgs& t, const CellRow& row) { return constant_uniform(t.layer_corners)[row.z0]; }

// word 1 of the children of a row
__device__ __forceinline__ uint32_t child_word(const OutlineArgs&, const CellRow&) { return 0u; }
__device__ __forceinline__ uint32_t child_word(const LayerArgs&, const CellRow& row) { return row.z0; }

// word 1 of a record
__device__ __forceinline__ uint32_t record_word(const OutlineArgs&, const CellRow&, uint32_t k, uint32_t from, uint32_t to)
{
    return k | (from << 8) | (to << 16);
}
__device__ __forceinline__ uint32_t record_word(const LayerArgs&, const CellRow& row, uint32_t k, uint32_t from, uint32_t to)
{
    return k | (from << 8) | (to << 10) | (row.z0 << 12);
}

// the point of the plane with the sample (0, 0) at `corner`, at the SHIFTED lattice indices (fs, ft): the section's formula
// at the sample indices fs - 1, ft - 1 (whole and half-integer shifted indices below 2^17: the subtraction is exact)
template <class A> __device__ __forceinline__ Point plane_point(const A& t, const float4& corner, float fs, float ft)
{
    const float a = t.c.step * (fs - 1.0f), b = t.c.step * (ft - 1.0f);
    return Point{(corner.x + t.u[0] * a) + t.v[0] * b, (corner.y + t.u[1] * a) + t.v[1] * b, (corner.z + t.u[2] * a) + t.v[2] * b};
}

template <bool DO, class A> __device__ __forceinline__ void outline_tiles(const A& t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + a.scratch_offset);
    const uint32_t lane = threadIdx.x & 63u;
    const CellRow row = outline_row(t);
    const float4 corner = plane_corner(t, row);
    const uint32_t s = a.child_side;
    const uint32_t x = row.x0 + (lane >> 3) * s, y = row.y0 + (lane & 7u) * s;
    const bool live = row.have & (x < a.dims[0]) & (y < a.dims[1]);
    const float h = 0.5f * (float)s;
    const Point p = plane_point(t, corner, (float)x + h, (float)y + h);
    const uint32_t* windows = constant_uniform(a.windows);
    uint64_t keep = 0ull;
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {      // wave-uniform; the one interpreter call site
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
        const uint32_t* win = windows + 6u * n;
        const bool reach = (x <= win[3]) & (x + s - 1u >= win[0]) & (y <= win[4]) & (y + s - 1u >= win[1]);
        const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
        if (reach && !(w >= a.thr) && !(w <= -a.thr)) keep |= 1ull << n;   // may cross an edge of the child (a NaN keeps its candidate)
    }
    // (the count stays spelled out: through a shared function the tiles compile to other code)
    const uint64_t lives = __ballot(live);
    if (lane == 0u && lives) atomicAdd(a.evaluations, (unsigned long long)(__popcll(lives) * __popcll(row.mask)));
    const bool flag[1] = {live && keep != 0ull};
    uint32_t slot[1];
    sdfk::wg_compact_slots<1>(flag, a.counter, scratch, slot);   // every wavefront of the workgroup gets here (barriers)
    if (flag[0] && slot[0] < a.capacity)
        a.children[slot[0]] = make_uint4(x | (y << 16), child_word(t, row), (uint32_t)keep, (uint32_t)(keep >> 32));
}

// The segments of a square by its case, bit c set when corner c is inside: corner 0 at (a, b), 1 at (a + 1, b), 2 at
// (a, b + 1), 3 at (a + 1, b + 1).  A segment is e_from << 2 | e_to, four bits per case.  One inside corner is walked
// round counter-clockwise, one outside corner clockwise; two on a side give the segment across, the inside on its left.
// The saddles 6 (corners 1, 2) and 9 (corners 0, 3) have a second segment: each cuts off one inside corner.
constexpr uint32_t seg(uint32_t from, uint32_t to) { return from << 2 | to; }
constexpr uint64_t kFirst =
    (uint64_t)seg(0, 3) << 4 | (uint64_t)seg(1, 0) << 8 | (uint64_t)seg(1, 3) << 12 | (uint64_t)seg(3, 2) << 16 | (uint64_t)seg(0, 2) << 20 |
    (uint64_t)seg(1, 0) << 24 | (uint64_t)seg(1, 2) << 28 | (uint64_t)seg(2, 1) << 32 | (uint64_t)seg(0, 3) << 36 | (uint64_t)seg(2, 0) << 40 |
    (uint64_t)seg(2, 3) << 44 | (uint64_t)seg(3, 1) << 48 | (uint64_t)seg(0, 1) << 52 | (uint64_t)seg(3, 0) << 56;
constexpr uint32_t kSecond6 = seg(3, 2), kSecond9 = seg(2, 1);

// the crossing of an edge from the sample with wp to the sample with wq
__device__ __forceinline__ float crossing(float wp, float wq)
{
    const float t = wp / (wp - wq);
    return t != t ? 0.5f : t;
}

template <bool DO, class A> __device__ __forceinline__ void outline_leaf(const A& t)
{
    extern __shared__ float4 lds[];
    const Args& a = t.c;
    const CellRow row = outline_row(t);
    if (!row.have) return;                                        // wave-uniform; this kernel has no barrier
    const float4 corner = plane_corner(t, row);
    const uint32_t lane = threadIdx.x & 63u;
    // the wavefront's 81 values, [9 j + i] of the sample (a0 + i, b0 + j), in its 128 floats after the register file
    float* wl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + a.scratch_offset) + (threadIdx.x >> 6) * 128u;
    const uint32_t i = lane & 7u, j = lane >> 3;
    const uint32_t x = row.x0 + i, y = row.y0 + j;
    const bool live = (x < a.dims[0]) & (y < a.dims[1]);          // the lane's square exists: so do its four samples
    // the second pass: lanes 0..8 take the column i = 8, lanes 9..16 the row j = 8; the others repeat their own sample
    const bool rim = lane < 17u;
    const uint32_t ri = lane < 9u ? 8u : lane - 9u, rj = lane < 9u ? lane : 8u;
    const uint64_t below = (1ull << lane) - 1ull;
    unsigned long long* totals = static_cast<unsigned long long*>(a.pairs);
    // samples exist up to the shifted index dims (one more than squares)
    const uint64_t first_lives = __ballot((x <= a.dims[0]) & (y <= a.dims[1]));
    const uint64_t rim_lives = __ballot(rim & (row.x0 + ri <= a.dims[0]) & (row.y0 + rj <= a.dims[1]));
    for (uint64_t m = row.mask; m != 0ull; m &= m - 1ull) {       // wave-uniform
        const uint32_t n = uniform((uint32_t)__builtin_ctzll(m));
#pragma unroll 1
        for (uint32_t pass = 0u; pass < 2u; ++pass) {             // the one interpreter call site, used twice
            const bool second = (pass != 0u) & rim;
            const uint32_t si = second ? ri : i, sj = second ? rj : j;
            const Point p = plane_point(t, corner, (float)(row.x0 + si), (float)(row.y0 + sj));
            const float w = instance_dist<DO>(a, n, p.x, p.y, p.z, lds);
            if ((pass == 0u) | rim) wl[9u * sj + si] = w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float w0 = wl[9u * j + i], w1 = wl[9u * j + i + 1u], w2 = wl[9u * j + i + 9u], w3 = wl[9u * j + i + 10u];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // (the next candidate's values overwrite these)
        __builtin_amdgcn_wave_barrier();
        const uint32_t c = (w0 < 0.0f ? 1u : 0u) | (w1 < 0.0f ? 2u : 0u) | (w2 < 0.0f ? 4u : 0u) | (w3 < 0.0f ? 8u : 0u);
        const bool one = live & (c != 0u) & (c != 15u), two = live & ((c == 6u) | (c == 9u));
        const uint64_t b1 = __ballot(one), b2 = __ballot(two);
        const uint32_t total = (uint32_t)(__popcll(b1) + __popcll(b2));
        if (total == 0u) continue;                                // wave-uniform
        unsigned long long base = 0ull;
        if (lane == 0u) {
            base = atomicAdd(&totals[0], (unsigned long long)total);
            atomicAdd(&totals[1u + n], (unsigned long long)total);
        }
        base = ((unsigned long long)uniform((uint32_t)(base >> 32)) << 32) | uniform((uint32_t)base);
        const unsigned long long slot = base + (unsigned long long)(__popcll(b1 & below) + __popcll(b2 & below));
        // the four edges' crossings (those of edges not crossed are not used)
        const float t0 = crossing(w0, w1), t1 = crossing(w1, w3), t2 = crossing(w2, w3), t3 = crossing(w0, w2);
        const uint32_t where = x | (y << 16);
        for (uint32_t r = 0u; r < 2u; ++r) {
            const uint32_t code = r == 0u ? (uint32_t)(kFirst >> (4u * c)) & 15u : (c == 6u ? kSecond6 : kSecond9);
            const uint32_t from = code >> 2, to = code & 3u;
            const float tf = from == 0u ? t0 : from == 1u ? t1 : from == 2u ? t2 : t3;
            const float tt = to == 0u ? t0 : to == 1u ? t1 : to == 2u ? t2 : t3;
            if ((r == 0u ? one : two) && slot + r < t.segment_capacity)
                t.segments[slot + r] = make_uint4(where, record_word(t, row, n, from, to), __float_as_uint(tf), __float_as_uint(tt));
        }
    }
    if (lane == 0u) atomicAdd(a.evaluations, (unsigned long long)((__popcll(first_lives) + __popcll(rim_lives)) * __popcll(row.mask)));
}

// What the entry points of both units check and fill alike: cells_args() of a lattice of squares {dims a, dims b, 1} with
// windows, and the plane's frame.
template <class A>
int outline_frame_args(const hu_cells_launch* l, const float u[3], const float v[3], A& t)
{
    if (!u || !v) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    std::memset(&t, 0, sizeof(t));
    int rc;
    if ((rc = cells_args(kWindows | kStrict | kPlanar, l, t.c))) return rc;
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(u[i]) || !std::isfinite(v[i]) || !std::isfinite(l->corner[i])) return hu_fail(HU_ERR_BAD_ARG, "the plane's frame must be finite");
        t.u[i] = u[i];
        t.v[i] = v[i];
    }
    return HU_OK;
}

// ... what their tile levels add: cells_children() and the bounds of a tile's side and radius
inline int outline_children(Args& a, const hu_cells_children* c)
{
    int rc;
    if ((rc = cells_children(a, c))) return rc;
    if ((rc = check_child_side(a.child_side, 8u, 8192u))) return rc;
    if (std::isnan(a.thr) || a.thr < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    return HU_OK;
}

// ... and their leaves: the segment records and their totals
template <class A>
int outline_segments(A& t, void* segments_dev, uint32_t segment_capacity, uint64_t* totals_dev)
{
    if (!totals_dev || (!segments_dev && segment_capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = totals_dev;
    t.segments = static_cast<uint4*>(segments_dev);
    t.segment_capacity = segment_capacity;
    return HU_OK;
}

}  // namespace hu_cells
