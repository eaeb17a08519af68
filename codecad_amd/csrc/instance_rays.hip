// codecad_amd/csrc/instance_rays.hip
//
// The ray caster over the instances of an assembly (codecad_amd/rendering/assembly_picture.py): kernels.hpp
// ray_caster_pixels -- the one statement of the reference's sequence -- around a scene that walks the instance table of
// instance_pairs.hip.  Every instance keeps its own tape; the field at a point is
//     F(p).w = min_k e_k(p).w,  F(p).xyz = e_m(p).xyz,  id(p) = m, the LOWEST index with e_m(p).w == F(p).w,
// so a pixel knows which part it shows: a colour per part, a part-id map and a depth map.
//
// SKIPPING.  An instance that cannot be the nearest at a sample is not evaluated there.  A lane keeps the length L of the
// path its samples have travelled so far, rounded up at every step (|p - p'| * (1 + 2^-10), the slack clearance's cell
// level uses, then the sum moved up by more than its rounding), and for every instance k ONE float in LDS, laid out
// [instance][lane] like clearance's leaf: B_k = w_k + L at the sample where k was last evaluated, rounded down.  With
// |grad w| <= 1 -- what k_classify and the cell levels rest on; shapes.unsafe breaks it here as there -- the value of k at
// the present sample is at least w_k - |p - q_k| >= w_k - (L - L_k) >= B_k - L, and k is left out when that, rounded down
// again, is greater than the least value the lane has seen at this sample: such a k can neither be the minimum nor tie
// with it, so F and id are what evaluating every instance gives, bit for bit.  A path length bounds the distance between
// any two samples of it, so a change of phase (primary -> ambient occlusion -> shadow -> floor), which moves the sample
// discontinuously, needs no reset: the jump is one more step of the path.  The wavefront runs the tape of an instance that
// any active lane needs; every lane then takes the value (more values never hurt the minimum).  A lane's previous winner
// goes first, so that the minimum is tight from the first comparison; the tie rule compares indices and holds in any order.
// Four bytes per instance and lane instead of the 16 of (w_k, q_k): 64 instances take 16 KiB per wavefront, not 64 KiB
// (DESIGN.md section 9 has the arithmetic).
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).  The entry point is at the end of
// this file.
#include "instance_cells.hpp"
#include "launchers.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

// x moved up / down by at least the rounding error of the operation that made it (a NaN or an infinity gives a NaN or
// itself: a bound that is no number never skips)
__device__ __forceinline__ float moved_up(float x) { return x + __builtin_fmaxf(__builtin_fabsf(x) * 0x1p-23f, 0x1p-60f); }
__device__ __forceinline__ float moved_down(float x) { return x - __builtin_fmaxf(__builtin_fabsf(x) * 0x1p-23f, 0x1p-60f); }

struct InstanceScene {
    const RayArgs& t;
    const RayCasterArgs& a;
    float* bounds;             // this lane's B_k at bounds[k * blockDim.x]
    F3 last;                   // the previous sample
    float travelled;           // L
    uint32_t winner;           // id of the previous sample
    uint32_t runs, asked;      // wave-uniform: instance programs run / asked for (samples x instances)

    __device__ __forceinline__ InstanceScene(const RayArgs& t_, const RayCasterArgs& a_, void* lds)
        : t(t_), a(a_), bounds(reinterpret_cast<float*>(static_cast<char*>(lds) + t_.bounds_offset) + threadIdx.x),
          last(mk3(0.0f, 0.0f, 0.0f)), travelled(0.0f), winner(0u), runs(0u), asked(0u)
    {
        for (uint32_t k = 0; k < t.n_instances; ++k) bounds[k * blockDim.x] = -__builtin_inff();   // never evaluated: never skipped
    }

    __device__ __forceinline__ float4 evaluate(F3 p, void* lds, bool active, uint32_t& id)
    {
        const uint32_t n = t.n_instances;
        const F3 d = sub3(p, last);
        last = p;
        travelled = moved_up(travelled + sdf::sqrt_(dot3(d, d)) * (1.0f + 0x1p-10f));
        const bool skipping = (t.flags & kRaysNoSkip) == 0u;
        // the previous winners of the active lanes go first
        uint64_t first = 0ull;
        if (skipping)
            for (uint64_t pending = __ballot(active); pending != 0ull;) {       // wave-uniform
                const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)winner, (int)__builtin_ctzll(pending));
                first |= 1ull << k;
                pending &= ~__ballot(winner == k);
            }
        float4 best = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        uint32_t best_id = 0xffffffffu;
        bool none = true;                                                // wave-uniform: no instance evaluated at this sample yet
        for (uint64_t todo = n >= 64u ? ~0ull : (1ull << n) - 1ull; todo != 0ull;) {   // wave-uniform; ONE interpreter call site
            const bool forced = first != 0ull;
            const uint32_t k = uniform((uint32_t)__builtin_ctzll(forced ? first : todo));
            first &= first - 1ull;      // (0 stays 0)
            todo &= ~(1ull << k);
            float* bound = bounds + k * blockDim.x;
            if (skipping && !forced) {
                const bool need = active && !(moved_down(*bound - travelled) > best.w);   // (a NaN needs)
                if (__ballot(need) == 0ull) continue;
            }
            ++runs;
            const InstanceRec r = constant_uniform(t.table)[k];
            const float4 e = sdf::voxel(InterpEval<false>{constant_uniform(r.prog), constant_uniform(r.extra), uniform(r.n4)}(p.x, p.y, p.z, lds), 0);
            *bound = moved_down(e.w + travelled);
            // the first value as it is (one instance: the plain ray caster, NaNs included), then the hardware minimum of the
            // union chain; its direction from the lowest index that attains it (among values that are no numbers, too)
            const float w = none ? e.w : __builtin_fminf(best.w, e.w);
            const bool take = none | ((e.w == w) & ((best.w != w) | (k < best_id))) | ((e.w != e.w) & (best.w != best.w) & (k < best_id));
            none = false;
            best = make_float4(take ? e.x : best.x, take ? e.y : best.y, take ? e.z : best.z, w);
            best_id = take ? k : best_id;
        }
        asked += n;
        winner = best_id < n ? best_id : 0u;                             // (always: the first instance run is taken)
        id = winner;
        return best;
    }

    // the hue of part `id`: the table is read through the scalar path, once per distinct part of the wavefront
    __device__ __forceinline__ F3 flat_color(uint32_t id, float ambient, float diffuse, float specular) const
    {
        const float4* colors = constant_uniform(t.colors);
        F3 c = mk3(0.0f, 0.0f, 0.0f);
        for (uint64_t pending = __ballot(true); pending != 0ull;) {      // the lanes that ask, wave-uniform
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)__builtin_ctzll(pending));
            const float4 v = colors[k];
            const bool mine = id == k;                                   // (a select, not a branch: k stays a scalar index)
            c = mk3(mine ? v.x : c.x, mine ? v.y : c.y, mine ? v.z : c.z);
            pending &= ~__ballot(mine);
        }
        return map_color(ambient, diffuse, specular, c);
    }

    __device__ __forceinline__ void pixel(uint32_t px, uint32_t py, bool hit, uint32_t id, float distance) const
    {
        const size_t i = (size_t)py + (size_t)a.h * px;
        t.part_ids[i] = hit ? (int32_t)id : -1;
        t.depth[i] = hit ? distance : __builtin_inff();
    }
};

__global__ void __launch_bounds__(256) k_ray_caster_instances(const RayArgs t, const RayCasterArgs a)
{
    extern __shared__ float4 lds[];
    InstanceScene scene(t, a, lds);
    ray_caster_pixels(scene, a, lds);
    if (t.counters && (threadIdx.x & 63u) == 0u) {
        atomicAdd(&t.counters[0], (unsigned long long)scene.runs);
        atomicAdd(&t.counters[1], (unsigned long long)scene.asked);
    }
}

}  // namespace

HU_BIG_LDS(k_ray_caster_instances);

extern "C" int hu_ray_caster_instances(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const float origin[4],
                                       const float forward[4], const float up[4], const float right[4], float pixel_tolerance,
                                       float box_radius, float min_distance, float max_distance, float floor_z, uint32_t render_options,
                                       uint32_t width, uint32_t height, const void* colors_dev, void* out_dev, int32_t* part_ids_dev,
                                       float* depth_dev, uint32_t flags, uint64_t* counters_dev, void* stream)
{
    if (!table_dev || !origin || !forward || !up || !right || !colors_dev || !out_dev || !part_ids_dev || !depth_dev)
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (n == 0 || n > 64u) return hu_fail(HU_ERR_BAD_ARG, "1..64 instances");
    if (distance_only_kernel) return hu_fail(HU_ERR_BAD_ARG, "the ray caster needs a table of full programs (hu_instance_table)");
    if (lane_bytes == 0 || lane_bytes % 16u) return hu_fail(HU_ERR_BAD_ARG, "lane_bytes of a table of full programs is a multiple of 16");
    if (width == 0 || height == 0) return hu_fail(HU_ERR_BAD_ARG, "image must have at least one pixel");
    if (render_options > 3u) return hu_fail(HU_ERR_BAD_ARG, "unknown render option bits");
    if (flags > 1u) return hu_fail(HU_ERR_BAD_ARG, "unknown flag bits");
    // a lane's LDS: the register file every instance's program fits, then one float per instance (the bounds of SKIPPING)
    uint32_t block;
    size_t lds;
    int rc;
    if ((rc = hu_workgroup((size_t)lane_bytes + 4u * n, block, lds))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    const uint64_t tiles = (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u);
    const uint64_t blocks = (tiles + block / 64u - 1) / (block / 64u);
    if (blocks > 0x7fffffffull) return hu_fail(HU_ERR_BAD_ARG, "image too large for one launch");
    const RayCasterArgs a = hu_render::ray_caster_args(origin, forward, up, right, pixel_tolerance, box_radius, min_distance, max_distance,
                                                       floor_z, render_options, width, height, out_dev);
    RayArgs t;
    t.table = static_cast<const InstanceRec*>(table_dev);
    t.n_instances = n;
    t.colors = static_cast<const float4*>(colors_dev);
    t.part_ids = part_ids_dev;
    t.depth = depth_dev;
    t.counters = reinterpret_cast<unsigned long long*>(counters_dev);
    t.flags = flags;
    t.bounds_offset = lane_bytes * block;
    hipLaunchKernelGGL(k_ray_caster_instances, dim3((uint32_t)blocks), dim3(block), lds, (hipStream_t)stream, t, a);
    HU_HIP(hipGetLastError());
    return HU_OK;
}
