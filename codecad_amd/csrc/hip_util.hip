// codecad_amd/csrc/hip_util.hip -- the tape handle and the interpreter's launches.
//
// The one unit built with -mllvm -structurizecfg-skip-uniform-regions (codecad_amd/hip_util/builder.py), so it holds the
// kernels that need it and the host code that cannot live anywhere else:
//   the runtime wrappers of the C ABI (include/hip_util.h): devices, memory, streams, events, the thread's last error;
//   hu_tape_create / hu_tape_destroy / hu_tape_info (the handle: tape_handle.hpp; its own kernels: tape_build.hip);
//   launch_shape(), prepare_masks() and the launches of the dense, leaf-block and classification kernels, through the
//   interpreter or through the tape's own kernels, and of the tape's ray caster and bitmap (kernels: render.hip);
//   hu_instance_table, which reads the handles of an assembly's tapes.
// Every other entry point lives with its kernels (launchers.hpp lists the units).
//
// Kernels (reference counterparts, paths relative to the reference's codecad/):
//   k_grid_eval            grid_eval.cl:2-34 (both layouts), dense slab of a logical grid
//   k_grid_eval_blocks     the per-leaf-block launches of rendering/mesh.py:53-60, batched
//   k_classify<MASS,BATCH> subdivision.cl:12-30 and mass_properties.cl:7-56, either one block
//                          (reference-shaped) or every parent of a level in one launch
//
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math
//        -fhip-fp32-correctly-rounded-divide-sqrt -fPIC -shared (see codecad_amd/hip_util/builder.py)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"
#include "instance_args.hpp"
#include "kernels.hpp"
#include "launchers.hpp"
#include "tape.hpp"
#include "tape_handle.hpp"

using sdf::Rec;
using namespace sdfk;

namespace {

thread_local std::string g_last_error;

struct LaunchShape {
    const Rec* prog;   // the program variant this launch runs
    uint32_t n4;       // its float4 slot count
    uint32_t block;
    size_t lds;
    size_t regfile_bytes;
    int voxels_per_lane;
};

// Kernels that only consume the distance run the distance-only interpreter unless the tape has a
// rounded blend (the one op through which a direction feeds a distance) or the caller forces
// the full interpreter (HU_FULL_INTERPRETER=1, used by the parity tests to cover both).
bool distance_only(const hu_tape_s* t)
{
    static const bool forced_full = [] { const char* e = getenv("HU_FULL_INTERPRETER"); return e && e[0] == '1'; }();
    return !forced_full && t->recs_do_dev != nullptr;
}

// Voxels per lane and workgroup size from the register file: the rule of host.hpp hu_workgroup(), and around it the
// choices only the grid kernels have (voxels per lane, single wavefronts for lanes that share nothing).
// Two voxels per lane (packed float2) halve the scalar work per voxel (fetch, decode, compare
// tree, branch), which is what limits the interpreter once the VALU work is trimmed, but they
// double the LDS register file.  Measured on MI355X (tools/prof_shape.py):
// two win whenever a 256-lane workgroup's file still fits 48 KiB (>= 3 workgroups per CU):
// always for the distance-only program (48-52 B per voxel), for the full program up to 6 live
// float4 values (sponge(4): 5.3 vs 5.8 ms; sponge(5), 7 values: 8.0 vs 7.7 ms -> one voxel).
// HU_VOXELS_PER_LANE=1|2 forces a choice (the parity tests run both).
int launch_shape(const hu_tape_s* t, LaunchShape& ls, bool distance_only_kernel, int max_voxels_per_lane = 2,
                 bool lanes_are_independent = false)
{
    static const int forced = [] { const char* e = getenv("HU_VOXELS_PER_LANE"); return e ? atoi(e) : 0; }();
    const size_t lane_bytes = distance_only_kernel ? (size_t)t->n_point_slots * 16 + (size_t)t->n_result_slots * 4
                                                   : (size_t)t->n_slots * 16;
    // (with fused leaf records the scalar work per voxel fell and latency -- waves per SIMD -- took over for the full
    // program: sponge(4), 6 float4 slots: 3.17 ms with one voxel per lane (24 KiB per workgroup, 6 workgroups per
    // CU) against 3.74 ms with two (48 KiB, 3); csg_example, 3 slots: 0.96 against 1.06 ms the other way round)
    const size_t two_voxel_limit = distance_only_kernel ? 48 * 1024 : 32 * 1024;
    const int by_rule = (forced == 1 || forced == 2) ? forced : ((lane_bytes * 2 * 256 <= two_voxel_limit) ? 2 : 1);
    const int wanted = by_rule < max_voxels_per_lane ? by_rule : max_voxels_per_lane;
    const Rec* prog = distance_only_kernel ? t->recs_do_dev : t->recs_dev;
    ls.prog = prog;
    ls.n4 = (uint32_t)(distance_only_kernel ? t->n_point_slots : t->n_slots);
    for (int n = wanted; n >= 1; --n) {
        const size_t per_lane = lane_bytes * n;
        uint32_t bs;
        size_t lds;
        if (hu_workgroup(per_lane, bs, lds, nullptr)) continue;     // not even 64 lanes fit
        // The grid kernels' lanes share nothing, and the interpreter waits more than it computes (forcing 5 waves per SIMD
        // instead of 6 costs 14 %): where single-wavefront workgroups fit more wavefronts into a CU's LDS than workgroups of
        // 256 lanes, take them (sponge(4), 6 float4 values: 26 against 24 per CU, -1 %; sponge(5), 7 values: 22 against 20, -3 %).
        auto waves_per_cu = [&](uint32_t lanes) {
            const size_t groups = kMaxLds / (per_lane * lanes + kScratchBytes), waves = groups * (lanes / 64u);
            return waves < 32 ? waves : (size_t)32;
        };
        if (lanes_are_independent && bs == 256u && waves_per_cu(64u) > waves_per_cu(256u)) bs = 64u;
        ls.block = bs;
        ls.regfile_bytes = per_lane * bs;
        ls.lds = ls.regfile_bytes + kScratchBytes;
        ls.voxels_per_lane = n;
        return HU_OK;
    }
    return hu_fail(HU_ERR_UNSUPPORTED, "tape keeps " + std::to_string(t->n_slots) +
                                        " values live at once; at most 159 fit the 160 KiB LDS register file");
}

template <typename K>
int allow_big_lds(K kernel)
{
    HU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    return HU_OK;
}

template <int N>
int ensure_attrs_n()
{
    int rc;
    if ((rc = allow_big_lds(k_grid_eval<InterpEval<false>, 0, N>))) return rc;
    if ((rc = allow_big_lds(k_grid_eval<InterpEval<false>, 1, N>))) return rc;
    if ((rc = allow_big_lds(k_grid_eval<InterpEval<true>, 1, N>))) return rc;
    if ((rc = allow_big_lds(k_grid_eval_blocks<InterpEval<false>, 0, N>))) return rc;
    if ((rc = allow_big_lds(k_grid_eval_blocks<InterpEval<false>, 1, N>))) return rc;
    if ((rc = allow_big_lds(k_grid_eval_blocks<InterpEval<true>, 1, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<false>, false, false, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<false>, false, true, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<false>, true, false, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<false>, true, true, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<true>, false, false, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<true>, false, true, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<true>, true, false, N>))) return rc;
    if ((rc = allow_big_lds(k_classify<InterpEval<true>, true, true, N>))) return rc;
    return HU_OK;
}

// the units' HU_BIG_LDS callbacks: a function's static, so that it exists whichever unit's initialisers run first
std::vector<hipError_t (*)(size_t)>& big_lds_units()
{
    static std::vector<hipError_t (*)(size_t)> units;
    return units;
}

}  // namespace

bool hu_big_lds_unit(hipError_t (*allow)(size_t bytes))
{
    big_lds_units().push_back(allow);
    return true;
}

int hu_fail(int code, const std::string& message)
{
    if (code == HU_ERR_HIP) (void)hipGetLastError();  // reported through the return code, not left sticky
    g_last_error = message;
    return code;
}

int hu_ensure_attrs()
{
    static thread_local int done_for_device = -1;
    int dev = 0;
    HU_HIP(hipGetDevice(&dev));
    if (done_for_device == dev) return HU_OK;
    int rc;
    if ((rc = ensure_attrs_n<1>())) return rc;
    if ((rc = ensure_attrs_n<2>())) return rc;
    for (const auto allow : big_lds_units()) HU_HIP(allow(kMaxLds));   // every unit that said HU_BIG_LDS (host.hpp)
    done_for_device = dev;
    return HU_OK;
}

namespace {

// Launches of per-tape code go over 16^3 boxes of compact 4 x 4 x 8 bricks (kernels.hpp box_eval) when the slab's or the
// block's extents allow it without ragged bricks (the grid kernels take ragged boxes too: k_grid_eval_ragged).
uint32_t brick_tiles(uint32_t nx, uint32_t sy, uint32_t sz)
{
    return (nx % 4u == 0u && sy % 4u == 0u && sz % 8u == 0u) ? 1u : 0u;
}
// ... and are boxes worth it: do at least half of the voxels of the bricks they would walk exist?  (A 2D grid is one voxel deep:
// an eighth.)  Else the launch goes over runs of cells (k_grid_eval_runs).
bool boxes_worthwhile(uint64_t nx, uint64_t sy, uint64_t sz)
{
    const uint64_t padded = ((nx + 3u) & ~3ull) * ((sy + 3u) & ~3ull) * ((sz + 7u) & ~7ull);
    return padded <= 2u * nx * sy * sz;
}

// How many units (blocks / parents) of `chunks` workgroups of `threads` lanes go into one launch: a grid may
// have at most 2^31 - 1 workgroups and 2^32 - 1 work-items; longer lists are launched in pieces.
uint32_t units_per_launch(uint32_t chunks, uint32_t threads)
{
    const uint64_t by_items = 0xffffffffull / threads / chunks, by_groups = 0x7fffffffull / chunks;
    const uint64_t n = by_items < by_groups ? by_items : by_groups;
    return n < 1 ? 1u : (uint32_t)n;
}

int check_dims(const uint32_t dims[3], uint64_t& cells)
{
    if (!dims) return hu_fail(HU_ERR_BAD_ARG, "dims is NULL");
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return hu_fail(HU_ERR_BAD_ARG, "dims must be >= 1 on every axis");
    cells = (uint64_t)dims[0] * dims[1] * dims[2];
    return HU_OK;
}

// The flags a per-tape kernel is launched with: kFlagInRange when no sample coordinate of the launch can exceed the
// tape's limit (HU_INRANGE=0 never sets it: measurements).  A tape of one primitive has a limit too and runs in the plain form,
// which reads no flags: the flag may be set for code that ignores it.
uint32_t spec_flags(const hu_tape_s* t, double max_abs_coordinate)
{
    static const bool off = [] { const char* e = getenv("HU_INRANGE"); return e && e[0] == '0'; }();
    return (!off && t->spec && max_abs_coordinate < t->spec->coord_limit) ? sdf::kFlagInRange : 0u;
}
// |coordinate| of any sample of a grid: corner + step * [0, n)
double grid_reach(const float corner[3], float step, const uint32_t dims[3])
{
    double m = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double a = std::fabs((double)corner[c]), b = std::fabs((double)corner[c] + (double)step * (double)dims[c]);
        m = std::max(m, std::max(a, b));
    }
    return m;
}
// ... of any sample of blocks whose integer corners (32-bit) come from a device list: |int| * resolution + origin + the block
double list_reach(double resolution, double ox, double oy, double oz, double block_extent)
{
    return 2147483648.0 * std::fabs(resolution) + std::max(std::fabs(ox), std::max(std::fabs(oy), std::fabs(oz))) + std::fabs(block_extent);
}

// LDS bytes of a box's tables (sdf::BoxTabs: 16 entries per single-axis column; pair columns of 16 rows of 17 / 24 floats)
// (dist: the layout of the distance walks -- leaf blocks and grids of the float layout, classification)
uint32_t box_table_bytes(const SpecKernels* k, bool dist)
{
    const int* n = dist ? k->dtabs : k->tabs;
    return (uint32_t)((n[0] + n[1] + n[2]) * sdf::BoxTabs::kAxis + (n[3] + n[4]) * sdf::BoxTabs::kPairX + n[5] * sdf::BoxTabs::kPairYZ) * 4u;
}

// Box pruning: run the tape's mask kernel for the `m.n_boxes` workgroups of the launch that follows on `stream` and hand
// back their masks -- or NULL (nothing to prune in this tape, or a buffer that would have to grow while
// the stream is being captured into a graph): the launch then treats everything as alive.
int prepare_masks(hu_tape_s* t, MaskArgs& m, hipStream_t stream, const uint32_t** masks)
{
    *masks = nullptr;
    SpecKernels* k = t->spec;
    if (!k || !k->box_masks || k->prune_words <= 0 || m.n_boxes == 0) return HU_OK;
    const size_t bytes = (size_t)m.n_boxes * (size_t)k->prune_words * sizeof(uint32_t);
    SpecKernels::MaskBuffer* buf = nullptr;
    for (auto& b : k->mask_buffers) if (b.stream == stream) buf = &b;
    if (!buf || buf->bytes < bytes) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing(stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) return HU_OK;
        (void)hipGetLastError();
        if (!buf) { k->mask_buffers.push_back(SpecKernels::MaskBuffer{stream, nullptr, 0}); buf = &k->mask_buffers.back(); }
        // (hipFree waits for the device: a launch still reading the old buffer has finished before it goes)
        if (buf->ptr) HU_HIP(hipFree(buf->ptr));
        buf->ptr = nullptr; buf->bytes = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        HU_HIP(hipMalloc((void**)&buf->ptr, want));
        buf->bytes = want;
    }
    m.out = buf->ptr;
    SpecEval ev{t->extra_dev, 0u};
    void* args[] = {&ev, &m};
    HU_HIP(hipModuleLaunchKernel(k->box_masks, (m.n_boxes + 63u) / 64u, 1, 1, 64, 1, 1, 0, stream, args, nullptr));
    *masks = buf->ptr;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_abi_version(void) { return HU_ABI_VERSION; }
const char* hu_last_error(void) { return g_last_error.c_str(); }

int hu_device_count(int* count)
{
    if (!count) return hu_fail(HU_ERR_BAD_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hu_fail(HU_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return HU_OK;
}

int hu_set_device(int ordinal)
{
    HU_HIP(hipSetDevice(ordinal));
    return HU_OK;
}

int hu_device_name(int ordinal, char* buf, size_t buflen)
{
    if (!buf || !buflen) return hu_fail(HU_ERR_BAD_ARG, "buf is NULL");
    hipDeviceProp_t prop;
    HU_HIP(hipGetDeviceProperties(&prop, ordinal));
    std::snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return HU_OK;
}

int hu_synchronize(void)
{
    HU_HIP(hipDeviceSynchronize());
    return HU_OK;
}

int hu_malloc(void** out_dev, size_t bytes)
{
    if (!out_dev) return hu_fail(HU_ERR_BAD_ARG, "out_dev is NULL");
    *out_dev = nullptr;
    HU_HIP(hipMalloc(out_dev, bytes ? bytes : 1));
    return HU_OK;
}

int hu_free(void* dev)
{
    if (dev) HU_HIP(hipFree(dev));
    return HU_OK;
}

int hu_host_alloc(void** out_host, size_t bytes)
{
    if (!out_host) return hu_fail(HU_ERR_BAD_ARG, "out_host is NULL");
    HU_HIP(hipHostMalloc(out_host, bytes ? bytes : 1, hipHostMallocDefault));
    return HU_OK;
}

int hu_host_free(void* host)
{
    if (host) HU_HIP(hipHostFree(host));
    return HU_OK;
}

int hu_memcpy_h2d(void* dst, const void* src, size_t n, void* stream)
{
    HU_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (hipStream_t)stream));
    return HU_OK;
}

int hu_memcpy_d2h(void* dst, const void* src, size_t n, void* stream)
{
    HU_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return HU_OK;
}

int hu_memcpy_d2d(void* dst, const void* src, size_t n, void* stream)
{
    HU_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return HU_OK;
}

int hu_memset(void* dst, int value, size_t n, void* stream)
{
    HU_HIP(hipMemsetAsync(dst, value, n, (hipStream_t)stream));
    return HU_OK;
}

int hu_stream_create(void** out)
{
    if (!out) return hu_fail(HU_ERR_BAD_ARG, "out is NULL");
    hipStream_t s;
    HU_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return HU_OK;
}

int hu_stream_destroy(void* s)
{
    if (s) HU_HIP(hipStreamDestroy((hipStream_t)s));
    return HU_OK;
}

int hu_stream_synchronize(void* s)
{
    HU_HIP(hipStreamSynchronize((hipStream_t)s));
    return HU_OK;
}

int hu_stream_wait_event(void* s, void* ev)
{
    HU_HIP(hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)ev, 0));
    return HU_OK;
}

int hu_event_create(void** out)
{
    if (!out) return hu_fail(HU_ERR_BAD_ARG, "out is NULL");
    hipEvent_t e;
    HU_HIP(hipEventCreate(&e));
    *out = e;
    return HU_OK;
}

int hu_event_destroy(void* e)
{
    if (e) HU_HIP(hipEventDestroy((hipEvent_t)e));
    return HU_OK;
}

int hu_event_record(void* e, void* s)
{
    HU_HIP(hipEventRecord((hipEvent_t)e, (hipStream_t)s));
    return HU_OK;
}

int hu_event_synchronize(void* e)
{
    HU_HIP(hipEventSynchronize((hipEvent_t)e));
    return HU_OK;
}

int hu_event_elapsed_ms(void* a, void* b, float* out_ms)
{
    if (!out_ms) return hu_fail(HU_ERR_BAD_ARG, "out_ms is NULL");
    HU_HIP(hipEventElapsedTime(out_ms, (hipEvent_t)a, (hipEvent_t)b));
    return HU_OK;
}

int hu_tape_create(const float* tape, size_t n, hu_tape* out)
{
    if (!tape || !out) return hu_fail(HU_ERR_BAD_ARG, "tape/out is NULL");
    *out = nullptr;
    sdf::DecodedTape d;
    std::string err = sdf::decode_tape(tape, n, d);
    if (!err.empty()) return hu_fail(HU_ERR_BAD_TAPE, "malformed tape: " + err);
    hu_tape_s* t = new hu_tape_s();
    t->n_instr = d.n_instructions;
    t->n_regs = d.n_regs;
    t->n_slots = d.n_slots;
    t->n_point_slots = d.n_point_slots;
    t->n_result_slots = d.n_result_slots;
    t->flags = d.direction_feeds_distance ? 1 : 0;
    keep_programs(t, d);
    // the device holds the interpreter's (fused) programs; per-tape code is generated from the unfused ones
    hipError_t e = hipMalloc((void**)&t->recs_dev, d.fused.size() * sizeof(Rec));
    if (e == hipSuccess && !d.fused_do.empty()) {
        e = hipMalloc((void**)&t->recs_do_dev, d.fused_do.size() * sizeof(Rec));
        if (e == hipSuccess) e = hipMemcpy(t->recs_do_dev, d.fused_do.data(), d.fused_do.size() * sizeof(Rec), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&t->extra_dev, d.extra.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(t->recs_dev, d.fused.data(), d.fused.size() * sizeof(Rec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->extra_dev, d.extra.data(), d.extra.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(t->recs_dev);
        (void)hipFree(t->recs_do_dev);
        (void)hipFree(t->extra_dev);
        delete t;
        return hu_fail(HU_ERR_HIP, std::string("tape upload: ") + hipGetErrorString(e));
    }
    *out = t;
    return HU_OK;
}

int hu_tape_destroy(hu_tape t)
{
    if (!t) return HU_OK;
    if (t->spec) {
        for (auto& b : t->spec->mask_buffers) (void)hipFree(b.ptr);
        for (hipModule_t m : t->spec->modules) (void)hipModuleUnload(m);
        delete t->spec;
    }
    (void)hipFree(t->recs_dev);
    (void)hipFree(t->recs_do_dev);
    (void)hipFree(t->extra_dev);
    delete t;
    return HU_OK;
}

int hu_tape_info(hu_tape t, int* n_instructions, int* n_registers, int* flags)
{
    if (!t) return hu_fail(HU_ERR_BAD_ARG, "tape is NULL");
    if (n_instructions) *n_instructions = t->n_instr;
    if (n_registers) *n_registers = t->n_slots;
    if (flags) *flags = t->flags;
    return HU_OK;
}

int hu_grid_eval_slab(hu_tape t, const float corner[4], float step, const uint32_t dims[3],
                      uint32_t x0, uint32_t x_count, int layout, void* out_dev, void* stream)
{
    if (!t || !corner || !out_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (layout != 0 && layout != 1) return hu_fail(HU_ERR_BAD_ARG, "layout must be 0 (float4) or 1 (pymcubes float)");
    uint64_t cells;
    int rc;
    if ((rc = check_dims(dims, cells))) return rc;
    if ((uint64_t)x0 + x_count > dims[0]) return hu_fail(HU_ERR_BAD_ARG, "slab exceeds the grid's x extent");
    const uint64_t plane = (uint64_t)dims[1] * dims[2];
    if (plane >= (1ull << 30)) return hu_fail(HU_ERR_BAD_ARG, "dims[1]*dims[2] must be below 2^30");
    // (pieces of a slab too long for one launch start at multiples of 16 planes: they are ragged only where the slab is)
    const uint32_t spec_max_x = [&] { const uint32_t m = (uint32_t)((1ull << 30) / plane); return m >= 16u ? m & ~15u : m; }();
    // extents that are no multiples of (4, 4, 8) take the kernel whose boxes may end anywhere: an image of its own -- while it is
    // still being built the interpreter serves such launches
    const bool spec_ragged = t->spec && t->spec->deferred && !(brick_tiles(x_count, dims[1], dims[2]) && (x_count <= spec_max_x || spec_max_x % 4u == 0u));
    // ... unless boxes would be mostly padding: then over runs of cells, in the in-place form (a third image)
    const bool spec_runs = spec_ragged && !boxes_worthwhile(x_count < spec_max_x ? x_count : spec_max_x, dims[1], dims[2]);
    if (t->spec && t->spec->dense[layout] && (!spec_ragged || (spec_runs ? t->spec->dense_runs[layout] : t->spec->dense_ragged[layout]))) {
        const uint32_t max_x = spec_max_x;
        SpecEval ev{t->extra_dev, spec_flags(t, grid_reach(corner, step, dims))};
        float cx = corner[0], cy = corner[1], cz = corner[2];
        uint32_t sx = dims[0];
        Dim sy = make_dim(dims[1]), sz = make_dim(dims[2]);
        for (uint32_t done = 0; done < x_count;) {
            const uint32_t nx = (x_count - done < max_x) ? (x_count - done) : max_x;
            uint32_t n_cells = (uint32_t)(nx * plane), xs = x0 + done;
            void* o = (layout == 0) ? (void*)(static_cast<float4*>(out_dev) + (size_t)done * plane) : out_dev;
            // boxes of compact bricks pay where a wavefront's work depends on how many primitives win in it (deferred
            // directions) and where the tape has tables to fill; a tape that is bound by its store stream keeps the runs
            // along z (2 KiB contiguous per wavefront: sphere, 512^3 float4: 0.34 ms in runs, 0.42 ms in bricks)
            uint32_t boxes = (t->spec->deferred && !spec_runs) ? 1u : 0u;
            const bool ragged = boxes && !brick_tiles(nx, dims[1], dims[2]);
            // (runs of cells take 256 lanes per workgroup too: the lanes of a run kernel share nothing, but single-wavefront
            // workgroups were SLOWER on the store-bound tapes -- box, 512^3 float4: 0.409 against 0.373 ms, its distance grid
            // 0.265 against 0.180 ms)
            // A tape of a primitive or two (a box, a sphere: per-tape code in the plain form, over runs) is bound by its
            // store stream, and that stream runs FASTER with fewer wavefronts in flight: box, 512^3 float4: 0.373 ms at eight
            // wavefronts per SIMD (what its 20-odd registers allow), 0.328 ms at four -- the interpreter's rate, whose LDS
            // register file holds it near there anyway (measured with the register allocator held to 2 / 4 / 6 / 8 waves per
            // SIMD: 0.382 / 0.328 / 0.353 / 0.373 ms).  So such a launch asks for 40 KiB of LDS it never touches: four
            // workgroups, sixteen wavefronts per CU.  (Longer tapes -- sponge(4): 0.407 -> 0.429 ms at four -- keep all.)
            // (float4 launches only: the float grid of the same tape stores a quarter of the bytes and is slowed by the limit --
            // box, 512^3: 0.182 -> 0.206 ms; of 0..64 KiB, 32-40 are the best, 53 -- three workgroups per CU, the best for
            // stores ALONE, tools/experiments/store_patterns.hip -- leaves the arithmetic too few wavefronts: 0.38 ms)
            constexpr uint32_t kStoreBoundLds = 40u * 1024u;
            const uint32_t idle_lds = (layout == 0 && !boxes && !t->spec->deferred && t->n_instr <= 16) ? kStoreBoundLds : 0u;
            const uint32_t per_block = kSpecBlock * kSpecVoxelsPerLane;
            uint32_t grid = (n_cells + per_block - 1) / per_block;
            const uint32_t* masks = nullptr;
            if (boxes) {
                grid = ((nx + 15u) / 16u) * ((dims[1] + 15u) / 16u) * ((dims[2] + 15u) / 16u);   // a workgroup per 16^3 box
                MaskArgs m{};
                m.mode = 0u; m.n_boxes = grid; m.chunks = grid; m.boxes_y = (dims[1] + 15u) / 16u; m.boxes_z = (dims[2] + 15u) / 16u;
                m.nx = nx; m.ny = dims[1]; m.nz = dims[2]; m.xs0 = xs; m.cx = cx; m.cy = cy; m.cz = cz; m.step = step;
                if ((layout == 1 || t->spec->prune_all) && (rc = prepare_masks(t, m, (hipStream_t)stream, &masks))) return rc;
            }
            if (spec_runs) {
                void* args[] = {&ev, &cx, &cy, &cz, &step, &sx, &sy, &sz, &xs, &n_cells, &o};
                HU_HIP(hipModuleLaunchKernel(t->spec->dense_runs[layout], grid, 1, 1, kSpecBlock, 1, 1, 0u, (hipStream_t)stream, args, nullptr));
            } else {
                void* args[] = {&ev, &cx, &cy, &cz, &step, &sx, &sy, &sz, &xs, &n_cells, &boxes, &o, &masks};
                HU_HIP(hipModuleLaunchKernel(ragged ? t->spec->dense_ragged[layout] : t->spec->dense[layout], grid, 1, 1, kSpecBlock, 1, 1,
                                             boxes ? box_table_bytes(t->spec, layout != 0) : idle_lds, (hipStream_t)stream, args, nullptr));
            }
            done += nx;
        }
        return HU_OK;
    }
    LaunchShape ls;
    if ((rc = launch_shape(t, ls, layout == 1 && distance_only(t), 2, true))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    // at most 2^30 cells per launch keeps every in-kernel index in 32 bits
    const uint32_t max_x = (uint32_t)((1ull << 30) / plane);
    for (uint32_t done = 0; done < x_count;) {
        const uint32_t nx = (x_count - done < max_x) ? (x_count - done) : max_x;
        const uint32_t n_cells = (uint32_t)(nx * plane);
        const uint32_t per_block = ls.block * ls.voxels_per_lane;
        const uint32_t blocks = (n_cells + per_block - 1) / per_block;
        void* o = (layout == 0) ? (void*)(static_cast<float4*>(out_dev) + (size_t)done * plane) : out_dev;
#define HU_LAUNCH_DENSE(L, D, NV)                                                                                  \
    hipLaunchKernelGGL((k_grid_eval<InterpEval<D>, L, NV>), dim3(blocks), dim3(ls.block), ls.lds, (hipStream_t)stream, \
                       (InterpEval<D>{ls.prog, t->extra_dev, ls.n4}), corner[0], corner[1], corner[2], step, dims[0],  \
                       make_dim(dims[1]), make_dim(dims[2]), x0 + done, n_cells,                                       \
                       0u /* the interpreter evaluates every primitive anyway: runs along z */, o, (const uint32_t*)nullptr)
        const bool d_only = layout == 1 && distance_only(t);
        if (ls.voxels_per_lane == 2) {
            if (layout == 0) HU_LAUNCH_DENSE(0, false, 2);
            else if (d_only) HU_LAUNCH_DENSE(1, true, 2);
            else HU_LAUNCH_DENSE(1, false, 2);
        } else {
            if (layout == 0) HU_LAUNCH_DENSE(0, false, 1);
            else if (d_only) HU_LAUNCH_DENSE(1, true, 1);
            else HU_LAUNCH_DENSE(1, false, 1);
        }
#undef HU_LAUNCH_DENSE
        HU_HIP(hipGetLastError());
        done += nx;
    }
    return HU_OK;
}

int hu_grid_eval(hu_tape t, const float corner[4], float step, const uint32_t dims[3], void* out_dev, void* stream)
{
    if (!dims) return hu_fail(HU_ERR_BAD_ARG, "dims is NULL");
    return hu_grid_eval_slab(t, corner, step, dims, 0, dims[0], 0, out_dev, stream);
}

int hu_grid_eval_pymcubes(hu_tape t, const float corner[4], float step, const uint32_t dims[3], void* out_dev, void* stream)
{
    if (!dims) return hu_fail(HU_ERR_BAD_ARG, "dims is NULL");
    return hu_grid_eval_slab(t, corner, step, dims, 0, dims[0], 1, out_dev, stream);
}

// n_dev == NULL: exactly n_blocks blocks; else the launch covers n_blocks and workgroups past *n_dev leave at once
static int grid_eval_blocks_impl(hu_tape t, const int32_t* blocks_dev, uint32_t n_blocks, const uint32_t* n_dev, double resolution,
                                 const double origin[3], float step, const uint32_t dims[3], int layout,
                                 void* out_dev, void* stream)
{
    if (!t || !origin || !out_dev || (!blocks_dev && n_blocks)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (layout != 0 && layout != 1) return hu_fail(HU_ERR_BAD_ARG, "layout must be 0 or 1");
    uint64_t cells;
    int rc;
    if ((rc = check_dims(dims, cells))) return rc;
    if (cells > (1ull << 24)) return hu_fail(HU_ERR_BAD_ARG, "a block may have at most 2^24 cells (256^3)");
    if (n_blocks == 0) return HU_OK;
    const bool blocks_ragged = t->spec && t->spec->deferred && !brick_tiles(dims[0], dims[1], dims[2]);
    const bool blocks_runs = blocks_ragged && !boxes_worthwhile(dims[0], dims[1], dims[2]);     // (boxes would be mostly padding)
    if (t->spec && t->spec->blocks[layout] && (!blocks_ragged || (blocks_runs ? t->spec->blocks_runs[layout] : t->spec->blocks_ragged[layout]))) {
        const uint32_t per_block = kSpecBlock * kSpecVoxelsPerLane;
        uint32_t chunks = (uint32_t)((cells + per_block - 1) / per_block);
        // deferred-direction code over compact bricks (kernels.hpp): a workgroup per box of up to 16^3 voxels of the block,
        // its wavefronts walking 4 x 4 x 8 bricks along x; `bricks` carries the boxes along y and z
        uint32_t bricks = 0u;
        const bool ragged = blocks_ragged && !blocks_runs;      // boxes that may end anywhere (k_grid_eval_blocks_ragged)
        if (t->spec->deferred && !blocks_runs) {
            const uint32_t bxn = (dims[0] + 15u) / 16u, byn = (dims[1] + 15u) / 16u, bzn = (dims[2] + 15u) / 16u;
            bricks = (byn << 16) | bzn;
            chunks = bxn * byn * bzn;
        }
        const double extent = (double)step * (double)std::max(dims[0], std::max(dims[1], dims[2]));
        SpecEval ev{t->extra_dev, spec_flags(t, list_reach(resolution, origin[0], origin[1], origin[2], extent))};
        const int4* b = (const int4*)blocks_dev;
        double res = resolution, ox = origin[0], oy = origin[1], oz = origin[2];
        uint32_t sx = dims[0];
        Dim sy = make_dim(dims[1]), sz = make_dim(dims[2]);
        const uint32_t piece = units_per_launch(chunks, kSpecBlock);
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += piece) {
            uint32_t first = b0;
            const uint32_t count = n_blocks - b0 < piece ? n_blocks - b0 : piece;
            const uint32_t* masks = nullptr;
            if (bricks) {
                MaskArgs m{};
                m.mode = 1u; m.n_boxes = chunks * count; m.chunks = chunks; m.boxes_y = bricks >> 16; m.boxes_z = bricks & 0xffffu;
                m.nx = dims[0]; m.ny = dims[1]; m.nz = dims[2]; m.unit_base = b0; m.units = b; m.n_units_dev = n_dev; m.step = step;
                m.res = res; m.ox = ox; m.oy = oy; m.oz = oz;
                if ((layout == 1 || t->spec->prune_all) && (rc = prepare_masks(t, m, (hipStream_t)stream, &masks))) return rc;
            }
            if (blocks_runs) {
                void* args[] = {&ev, &b, &n_dev, &first, &chunks, &res, &ox, &oy, &oz, &step, &sx, &sy, &sz, &out_dev};
                HU_HIP(hipModuleLaunchKernel(t->spec->blocks_runs[layout], chunks * count, 1, 1, kSpecBlock, 1, 1, 0u, (hipStream_t)stream, args, nullptr));
            } else {
                void* args[] = {&ev, &b, &n_dev, &first, &chunks, &bricks, &res, &ox, &oy, &oz, &step, &sx, &sy, &sz, &out_dev, &masks};
                HU_HIP(hipModuleLaunchKernel(ragged ? t->spec->blocks_ragged[layout] : t->spec->blocks[layout], chunks * count, 1, 1, kSpecBlock, 1, 1,
                                             bricks ? box_table_bytes(t->spec, layout != 0) : 0u, (hipStream_t)stream, args, nullptr));
            }
        }
        return HU_OK;
    }
    LaunchShape ls;
    if ((rc = launch_shape(t, ls, layout == 1 && distance_only(t), 2, true))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    const uint32_t per_block = ls.block * ls.voxels_per_lane;
    const uint32_t chunks = (uint32_t)((cells + per_block - 1) / per_block);
    const dim3 block(ls.block);
    const uint32_t piece = units_per_launch(chunks, ls.block);
#define HU_LAUNCH_BLOCKS(L, D, NV)                                                                                 \
    hipLaunchKernelGGL((k_grid_eval_blocks<InterpEval<D>, L, NV>), grid, block, ls.lds, (hipStream_t)stream,           \
                       (InterpEval<D>{ls.prog, t->extra_dev, ls.n4}), (const int4*)blocks_dev, n_dev, b0, chunks, 0u, resolution, \
                       origin[0], origin[1], origin[2], step, dims[0], make_dim(dims[1]), make_dim(dims[2]), out_dev, (const uint32_t*)nullptr)
    const bool d_only = layout == 1 && distance_only(t);
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += piece) {
        const dim3 grid(chunks * (n_blocks - b0 < piece ? n_blocks - b0 : piece));
        if (ls.voxels_per_lane == 2) {
            if (layout == 0) HU_LAUNCH_BLOCKS(0, false, 2);
            else if (d_only) HU_LAUNCH_BLOCKS(1, true, 2);
            else HU_LAUNCH_BLOCKS(1, false, 2);
        } else {
            if (layout == 0) HU_LAUNCH_BLOCKS(0, false, 1);
            else if (d_only) HU_LAUNCH_BLOCKS(1, true, 1);
            else HU_LAUNCH_BLOCKS(1, false, 1);
        }
    }
#undef HU_LAUNCH_BLOCKS
    HU_HIP(hipGetLastError());
    return HU_OK;
}

int hu_grid_eval_blocks(hu_tape t, const int32_t* blocks_dev, uint32_t n_blocks, double resolution,
                        const double origin[3], float step, const uint32_t dims[3], int layout,
                        void* out_dev, void* stream)
{
    return grid_eval_blocks_impl(t, blocks_dev, n_blocks, nullptr, resolution, origin, step, dims, layout, out_dev, stream);
}

int hu_grid_eval_blocks_indirect(hu_tape t, const int32_t* blocks_dev, const uint32_t* n_blocks_dev, uint32_t max_blocks,
                                 double resolution, const double origin[3], float step, const uint32_t dims[3], int layout,
                                 void* out_dev, void* stream)
{
    if (!n_blocks_dev) return hu_fail(HU_ERR_BAD_ARG, "n_blocks_dev is NULL");
    return grid_eval_blocks_impl(t, blocks_dev, max_blocks, n_blocks_dev, resolution, origin, step, dims, layout, out_dev, stream);
}

}  // extern "C"

namespace {

template <bool MASS, bool BATCH>
int launch_classify(hu_tape t, ClassifyArgs& a, uint32_t n_parents, const uint32_t dims[3], void* stream)
{
    uint64_t cells;
    int rc;
    if ((rc = check_dims(dims, cells))) return rc;
    if (cells > (1ull << 24)) return hu_fail(HU_ERR_BAD_ARG, "at most 2^24 cells (256^3) per block: cell indices are uchar4");
    if (dims[0] > 256 || dims[1] > 256 || dims[2] > 256)
        return hu_fail(HU_ERR_BAD_ARG, "grid size > 256 would overflow the uchar4 cell index (reference subdivision.py:206-208)");
    if (n_parents == 0) return HU_OK;
    a.sx = dims[0]; a.sy = dims[1]; a.sz = dims[2];
    a.dy = make_dim(dims[1]); a.dz = make_dim(dims[2]);
    if (t->spec && t->spec->classify[MASS ? 1 : 0][BATCH ? 1 : 0]) {
        const uint32_t per_block = kSpecBlock * kSpecVoxelsPerLane;
        a.chunks = (uint32_t)((cells + per_block - 1) / per_block);
        a.scratch_offset = 0;
        a.boxes = 0;
        // Grids of more than one workgroup's worth of cells go over 16^3 boxes with their tables in LDS (kernels.hpp
        // k_classify / box_eval) where the extents allow it.  (Up to 256 cells the lane-order compaction of ONE workgroup

        // And only launches that fill the chip several times over: a box is one workgroup where the path below has eight,
        // and a level of a few hundred parents is a latency exercise (measured: C5's 704 parents of 16^3 0.21 -> 0.33 ms
        // over boxes; C3's mass properties at grid 8, 167 000 parents in the last level, 0.94 -> 0.80 ms).
        const uint64_t bxn = (dims[0] + 15u) / 16u, byn = (dims[1] + 15u) / 16u, bzn = (dims[2] + 15u) / 16u;
        // A tape with box pruning is another matter: only the box path prunes, the path below evaluates every primitive for
        // every sample (planetary, mass properties at grid 64, resolution 0.5: 45 parents = 2880 boxes: 0.93 -> 0.34 ms over boxes;
        // resolution 1.0: 8 parents, 0.32 -> 0.27 ms; tools/experiments/mass_scale.py): such tapes take the boxes from 64 on.
        uint64_t enough = t->spec->prune_bits > 0 ? 64u : 8192u;
        if (const char* e = getenv("HU_CLASSIFY_BOX_MIN")) enough = (uint64_t)atoll(e);   // (read per launch: the tests switch it)
        if (t->spec->deferred && cells > 256u && bxn * byn * bzn * n_parents >= enough && boxes_worthwhile(dims[0], dims[1], dims[2])) {   // (any extents: the rims of a box are predicated; not where boxes would be mostly padding: 2D)
            a.boxes = ((uint32_t)byn << 16) | (uint32_t)bzn;
            a.chunks = (uint32_t)(bxn * byn * bzn);
            a.scratch_offset = box_table_bytes(t->spec, true);
        }
        // (mass-property parents are fp64 corners on the device: their magnitude is not the host's to know)
        const double extent = (double)a.step * (double)std::max(dims[0], std::max(dims[1], dims[2]));
        const float c3[3] = {a.cx, a.cy, a.cz};
        const double reach = !BATCH ? grid_reach(c3, a.step, dims)
                             : MASS ? HUGE_VAL
                                    : list_reach(a.res, a.ox, a.oy, a.oz, extent + std::fabs((double)a.int_step * a.res));
        SpecEval ev{t->extra_dev, spec_flags(t, reach)};
        const uint32_t piece = units_per_launch(a.chunks, kSpecBlock);
        for (uint32_t p0 = 0; p0 < n_parents; p0 += piece) {
            a.parent_base = p0;
            a.masks = nullptr;
            if (a.boxes) {
                MaskArgs m{};
                m.mode = !BATCH ? 2u : MASS ? 4u : 3u;
                m.n_boxes = a.chunks * (n_parents - p0 < piece ? n_parents - p0 : piece); m.chunks = a.chunks;
                m.boxes_y = a.boxes >> 16; m.boxes_z = a.boxes & 0xffffu; m.nx = dims[0]; m.ny = dims[1]; m.nz = dims[2];
                m.unit_base = p0; m.units = a.parents; m.n_units_dev = a.n_parents_dev; m.cx = a.cx; m.cy = a.cy; m.cz = a.cz; m.step = a.step;
                m.int_step = a.int_step; m.dimension = a.dimension; m.res = a.res; m.ox = a.ox; m.oy = a.oy; m.oz = a.oz; m.s = a.s;
                if ((rc = prepare_masks(t, m, (hipStream_t)stream, &a.masks))) return rc;
            }
            void* args[] = {&ev, &a};
            HU_HIP(hipModuleLaunchKernel(t->spec->classify[MASS ? 1 : 0][BATCH ? 1 : 0],
                                         a.chunks * (n_parents - p0 < piece ? n_parents - p0 : piece), 1, 1, kSpecBlock, 1, 1,
                                         (unsigned)(a.scratch_offset + kScratchBytes), (hipStream_t)stream, args, nullptr));
        }
        return HU_OK;
    }
    LaunchShape ls;
    if ((rc = launch_shape(t, ls, distance_only(t)))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    const uint32_t per_block = ls.block * ls.voxels_per_lane;
    a.chunks = (uint32_t)((cells + per_block - 1) / per_block);
    a.scratch_offset = (uint32_t)ls.regfile_bytes;
    a.boxes = 0;
    a.masks = nullptr;
    const dim3 block(ls.block);
    const bool d_only = distance_only(t);
    const uint32_t piece = units_per_launch(a.chunks, ls.block);
#define HU_LAUNCH_CLASSIFY(D, NV)                                                                                \
    hipLaunchKernelGGL((k_classify<InterpEval<D>, MASS, BATCH, NV>), grid, block, ls.lds, (hipStream_t)stream,     \
                       (InterpEval<D>{ls.prog, t->extra_dev, ls.n4}), a)
    for (uint32_t p0 = 0; p0 < n_parents; p0 += piece) {
        a.parent_base = p0;
        const dim3 grid(a.chunks * (n_parents - p0 < piece ? n_parents - p0 : piece));
        if (ls.voxels_per_lane == 2) {
            if (d_only) HU_LAUNCH_CLASSIFY(true, 2);
            else HU_LAUNCH_CLASSIFY(false, 2);
        } else {
            if (d_only) HU_LAUNCH_CLASSIFY(true, 1);
            else HU_LAUNCH_CLASSIFY(false, 1);
        }
    }
#undef HU_LAUNCH_CLASSIFY
    HU_HIP(hipGetLastError());
    return HU_OK;
}

ClassifyArgs zeroed_args()
{
    ClassifyArgs a;
    std::memset(&a, 0, sizeof(a));
    return a;
}

// what the two single-block entry points fill alike (the caller has checked the pointers)
ClassifyArgs block_args(const float corner[4], float step, float threshold, uint32_t* counter_dev, void* list_dev)
{
    ClassifyArgs a = zeroed_args();
    a.cx = corner[0]; a.cy = corner[1]; a.cz = corner[2];
    a.step = step; a.thr = threshold;
    a.counter = counter_dev; a.list = list_dev; a.capacity = 0xffffffffu;
    return a;
}

// the launch record of a level (hip_util.h): hip_util/_lib.py mirrors it field by field
static_assert(sizeof(hu_level_launch) == HU_LEVEL_LAUNCH_BYTES, "hu_level_launch must have the size hip_util.h states");
static_assert(offsetof(hu_level_launch, max_parents) == 48 && offsetof(hu_level_launch, dims) == 64 && offsetof(hu_level_launch, thr) == 80,
              "hu_level_launch: six pointers, then 32-bit fields without padding between them");

// A level's record, checked for NULLs, as the kernels' arguments; `own` is the entry point's own pointer (the origin, the
// sums), refused with the record's.  world = 1 leaves `own` zero: every cell is kept (kernels.hpp owned()).
int level_args(const hu_level_launch* l, const void* own, ClassifyArgs& a)
{
    if (!l || !l->tape || !own || !l->counter_dev || (!l->children_dev && l->capacity) || (!l->parents_dev && l->max_parents))
        return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    a = zeroed_args();
    a.parents = l->parents_dev;
    a.n_parents_dev = l->n_parents_dev;
    a.step = l->step; a.thr = l->thr;
    a.counter = l->counter_dev; a.list = l->children_dev; a.capacity = l->capacity;
    if (l->world >= 2u) { a.own = make_dim(l->world); a.own_rank = l->rank; }
    return HU_OK;
}

// ... and its launch, after the entry point's own checks: n_parents_dev == NULL means exactly max_parents parents
template <bool MASS>
int launch_level(const hu_level_launch* l, ClassifyArgs& a)
{
    if (l->world == 0 || l->rank >= l->world) return hu_fail(HU_ERR_BAD_ARG, "rank must be below world");
    return launch_classify<MASS, true>(l->tape, a, l->max_parents, l->dims, l->stream);
}

}  // namespace

extern "C" {

int hu_subdivision_step(hu_tape t, const float corner[4], float step, float threshold, const uint32_t dims[3],
                        uint32_t* counter_dev, void* list_dev, void* stream)
{
    if (!t || !corner || !counter_dev || !list_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    ClassifyArgs a = block_args(corner, step, threshold, counter_dev, list_dev);
    return launch_classify<false, false>(t, a, 1, dims, stream);
}

int hu_mass_properties(hu_tape t, const float corner[4], float step, float threshold, const uint32_t dims[3],
                       uint32_t* sum_dev, uint32_t* counter_dev, void* list_dev, void* stream)
{
    if (!t || !corner || !sum_dev || !counter_dev || !list_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    ClassifyArgs a = block_args(corner, step, threshold, counter_dev, list_dev);
    a.sums = sum_dev;
    return launch_classify<true, false>(t, a, 1, dims, stream);
}

int hu_subdivision_level(const hu_level_launch* launch, int32_t int_step, int dimension, double resolution, const double origin[3])
{
    ClassifyArgs a;
    int rc;
    if ((rc = level_args(launch, origin, a))) return rc;
    if (dimension != 2 && dimension != 3) return hu_fail(HU_ERR_BAD_ARG, "dimension must be 2 or 3");
    a.int_step = int_step; a.dimension = dimension;
    a.res = resolution; a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
    return launch_level<false>(launch, a);
}

int hu_mass_properties_level(const hu_level_launch* launch, double s, uint32_t* sums_dev)
{
    ClassifyArgs a;
    int rc;
    if ((rc = level_args(launch, sums_dev, a))) return rc;
    a.s = s;
    a.sums = sums_dev;
    return launch_level<true>(launch, a);
}

int hu_instance_table(const hu_tape* tapes, uint32_t n, int full_programs, void* table_host, size_t bytes, int* distance_only_out,
                      uint32_t* lane_bytes)
{
    if (!tapes || !table_host || !distance_only_out || !lane_bytes) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (n == 0 || n > 64u) return hu_fail(HU_ERR_BAD_ARG, "an interference table holds 1..64 instances");
    if (bytes < (size_t)n * sizeof(hu_cells::InstanceRec)) return hu_fail(HU_ERR_BAD_ARG, "table buffer too small");
    bool all_do = !full_programs;
    for (uint32_t i = 0; i < n; ++i) {
        if (!tapes[i]) return hu_fail(HU_ERR_BAD_ARG, "NULL tape");
        all_do = all_do && distance_only(tapes[i]);
    }
    // one interpreter instantiation per kernel: the distance-only programs when every instance has one, else the full ones.
    // The wavefronts of a workgroup run different instances at once, and the register file interleaves every lane of the
    // workgroup (float4 slot r of lane l at r * block + l, the scalar slots after n4 * block of them): so every instance
    // gets the same n4, the largest, and no instance's float4 slots reach into another one's scalar slots.
    uint32_t n4 = 0, n_res = 0;
    for (uint32_t i = 0; i < n; ++i) {
        n4 = std::max(n4, (uint32_t)(all_do ? tapes[i]->n_point_slots : tapes[i]->n_slots));
        n_res = std::max(n_res, all_do ? (uint32_t)tapes[i]->n_result_slots : 0u);
    }
    // A table asked for with full_programs reports one slot at least: programs that store nothing (plain spheres) keep no
    // value, and hu_ray_caster_instances takes a lane_bytes of 0 for "not a table of full programs".
    if (full_programs) n4 = std::max(n4, 1u);
    auto* recs = static_cast<hu_cells::InstanceRec*>(table_host);
    for (uint32_t i = 0; i < n; ++i)
        recs[i] = hu_cells::InstanceRec{all_do ? tapes[i]->recs_do_dev : tapes[i]->recs_dev, tapes[i]->extra_dev, n4, 0u};
    *distance_only_out = all_do ? 1 : 0;
    *lane_bytes = n4 * 16u + n_res * 4u;
    return HU_OK;
}

int hu_ray_caster(hu_tape t, const float origin[4], const float forward[4], const float up[4], const float right[4],
                  float pixel_tolerance, float box_radius, float min_distance, float max_distance, float floor_z,
                  uint32_t render_options, uint32_t width, uint32_t height, void* out_dev, void* stream)
{
    if (!t || !origin || !forward || !up || !right || !out_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (width == 0 || height == 0) return hu_fail(HU_ERR_BAD_ARG, "image must have at least one pixel");
    if (render_options > 3u) return hu_fail(HU_ERR_BAD_ARG, "unknown render option bits");
    const uint64_t tiles = (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u);
    LaunchShape ls;
    int rc;
    if ((rc = launch_shape(t, ls, false, 1))) return rc;  // directions steer the march: full program
    if ((rc = hu_ensure_attrs())) return rc;
    const uint32_t waves_per_block = ls.block / 64u;
    const uint64_t blocks = (tiles + waves_per_block - 1) / waves_per_block;
    if (blocks > 0x7fffffffull) return hu_fail(HU_ERR_BAD_ARG, "image too large for one launch");
    RayCasterArgs a = hu_render::ray_caster_args(origin, forward, up, right, pixel_tolerance, box_radius, min_distance, max_distance,
                                                 floor_z, render_options, width, height, out_dev);
    if (t->spec && t->spec->ray_caster) {
        SpecEval ev{t->extra_dev, 0u};
        void* args[] = {&ev, &a};
        const uint64_t spec_blocks = (tiles + kSpecBlock / 64u - 1) / (kSpecBlock / 64u);
        HU_HIP(hipModuleLaunchKernel(t->spec->ray_caster, (uint32_t)spec_blocks, 1, 1, kSpecBlock, 1, 1, 0, (hipStream_t)stream,
                                     args, nullptr));
        return HU_OK;
    }
    HU_HIP(hu_render::ray_caster(InterpEval<false>{ls.prog, t->extra_dev, ls.n4}, a, (uint32_t)blocks, ls.block, ls.lds, (hipStream_t)stream));
    return HU_OK;
}

int hu_bitmap(hu_tape t, const float origin[4], float step_size, uint32_t width, uint32_t height, void* out_dev,
              void* stream)
{
    if (!t || !origin || !out_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (width == 0 || height == 0) return hu_fail(HU_ERR_BAD_ARG, "image must have at least one pixel");
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels > 0x7fffffffull) return hu_fail(HU_ERR_BAD_ARG, "image too large for one launch");
    uint8_t* out = static_cast<uint8_t*>(out_dev);
    if (t->spec && t->spec->bitmap) {
        SpecEval ev{t->extra_dev, 0u};
        float ox = origin[0], oy = origin[1], oz = origin[2];
        void* args[] = {&ev, &ox, &oy, &oz, &step_size, &width, &height, &out};
        HU_HIP(hipModuleLaunchKernel(t->spec->bitmap, (uint32_t)((pixels + kSpecBlock - 1) / kSpecBlock), 1, 1, kSpecBlock, 1, 1, 0,
                                     (hipStream_t)stream, args, nullptr));
        return HU_OK;
    }
    const bool d_only = distance_only(t);
    LaunchShape ls;
    int rc;
    if ((rc = launch_shape(t, ls, d_only, 1))) return rc;
    if ((rc = hu_ensure_attrs())) return rc;
    HU_HIP(hu_render::bitmap(d_only, ls.prog, t->extra_dev, ls.n4, origin[0], origin[1], origin[2], step_size, width, height, out,
                             (uint32_t)((pixels + ls.block - 1) / ls.block), ls.block, ls.lds, (hipStream_t)stream));
    return HU_OK;
}

}  // extern "C"
