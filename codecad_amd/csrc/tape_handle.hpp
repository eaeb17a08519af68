// codecad_amd/csrc/tape_handle.hpp -- the tape handle (hu_tape) and the kernels of its own that are loaded into it: what
// hip_util.hip (which launches them) and tape_build.hip (which builds and loads them) share.  Private, like host.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hip_util.h"
#include "specialise.hpp"

// ------------------------------------------------------------------------------------------
// Per-tape specialisation (the analogue of the reference's generate_fixed_eval_source_code,
// nodes/codegen.py:137-204): the decoded program is unrolled into straight-line HIP source --
// one exec_one call per record with the record as a literal -- and compiled with hipRTC against
// the SAME op library (interp.hpp).  With a literal record the opcode switch folds to one case
// and every slot index is a constant, so the register file dissolves into VGPRs: no dispatch,
// no scalar fetch, no LDS.  Kernels that only read the distance get the direction arithmetic
// removed by dead-code elimination.  The arithmetic is the interpreter's, operation for
// operation, so results are identical (tests run the parity suite on specialised tapes).
// ------------------------------------------------------------------------------------------
// A tape's kernels may sit in several modules: a synchronous build (hu_tape_specialize_groups without a cached image)
// compiles the requested set as ONE module, the background builds (codecad_amd/hip_util/buffer.py) make one image per
// KERNEL, side by side in several processes.  (Rounds 1-3 built all kernels, then families, together: in the plain form
// hipRTC spent its time on the one straight-line tape function every kernel shared.  The deferred form over boxes
// instantiates its own functions per kernel -- sponge(4), family of five: 1.40 s, its kernels one by one: 0.09 + 0.47 +
// 0.55 + 0.22 + 0.27 s with the precompiled header of tape_build.hip -- so a launch's kernel is ready in a third of the time.)
struct SpecKernels {
    std::vector<hipModule_t> modules;   // one per hu_tape_specialize_groups call that built something
    uint32_t groups = 0;                // the kernels that are loaded (bit i: kernel i of kSpecKernelNames)
    hipFunction_t dense[2] = {nullptr, nullptr};
    hipFunction_t blocks[2] = {nullptr, nullptr};
    // tapes with box code: the same over runs of cells, for extents that are no multiples of (4, 4, 8) (kernels.hpp k_grid_eval_ragged)
    hipFunction_t dense_ragged[2] = {nullptr, nullptr};
    hipFunction_t blocks_ragged[2] = {nullptr, nullptr};
    // ... and over runs of cells, in the in-place form, where boxes would be mostly padding (2D grids: kernels.hpp k_grid_eval_runs)
    hipFunction_t dense_runs[2] = {nullptr, nullptr};
    hipFunction_t blocks_runs[2] = {nullptr, nullptr};
    hipFunction_t classify[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [MASS][BATCH]
    hipFunction_t ray_caster = nullptr, bitmap = nullptr;
    hipFunction_t box_masks = nullptr;   // k_box_masks (box pruning), part of every family that launches over boxes
    bool deferred = false;   // the module was generated with deferred directions (specialise.hpp): dense launches use bricks
    double coord_limit = 0.0;   // a launch whose sample coordinates all stay below this sets sdf::kFlagInRange (specialise.hpp)
    int tabs[6] = {0, 0, 0, 0, 0, 0};   // columns of a box's tables: x, y, z, xy, xz, yz (specialise.hpp), float4 walks
    int dtabs[6] = {0, 0, 0, 0, 0, 0};  // ... of the distance walks' tables (kernels.hpp box_tables<true>)
    int prune_words = 0;     // 32-bit words of a box's pruning mask (0: nothing to prune in this tape)
    int prune_bits = 0;
    bool prune_all = false;  // the float4 code is guarded too (else only the distance walks: float4 launches skip the mask kernel)
    // the mask buffers of launches over boxes, one per stream that launched any (the mask kernel and the launch it prepares
    // are neighbours on their stream, so a stream's launches can share one buffer); grown when a launch needs more
    struct MaskBuffer { hipStream_t stream; uint32_t* ptr; size_t bytes; };
    std::vector<MaskBuffer> mask_buffers;
};

struct hu_tape_s {
    sdf::Rec* recs_dev = nullptr;     // full program
    sdf::Rec* recs_do_dev = nullptr;  // distance-only program (NULL when the tape has a rounded blend)
    float* extra_dev = nullptr;
    int n_instr = 0;
    int n_regs = 0;              // registers named by the tape
    int n_slots = 0;             // float4 slots of the full program after renaming
    int n_point_slots = 0, n_result_slots = 0;  // distance-only program
    int flags = 0;
    sdf::SpecProgram program;    // both programs on the host, kept for hu_tape_specialize (specialise.hpp)
    SpecKernels* spec = nullptr;
    std::string spec_source;     // the generated per-tape source, once it has been asked for (a tape's kernels are built and
    sdf::SpecMeta spec_meta;     // probed one by one: planetary's source takes tens of milliseconds to generate)
};

constexpr int kSpecVoxelsPerLane = 2;
constexpr uint32_t kSpecBlock = 256;

inline void keep_programs(hu_tape_s* t, const sdf::DecodedTape& d)
{
    t->program.full = d.recs;
    t->program.dist = d.recs_do;
    t->program.n_slots = d.n_slots;
    t->program.n_point_slots = d.n_point_slots;
    t->program.n_result_slots = d.n_result_slots;
}

struct SpecEval { const float* extra; uint32_t flags; };  // same layout as the generated sdfk::JitEval

constexpr int kSpecKernelCount = 19;
// bit i of a `groups` mask is kernel i below; the families of include/hip_util.h (HU_SPEC_*) are sets of them (the mask
// kernel of box pruning belongs to every family that launches over boxes)
constexpr uint32_t spec_bit(int i) { return 1u << i; }
constexpr uint32_t kSpecGroupOf[kSpecKernelCount] = {spec_bit(0), spec_bit(1), spec_bit(2), spec_bit(3), spec_bit(4), spec_bit(5), spec_bit(6), spec_bit(7),
                                                      spec_bit(8), spec_bit(9), spec_bit(10), spec_bit(11), spec_bit(12), spec_bit(13), spec_bit(14),
                                                      spec_bit(15), spec_bit(16), spec_bit(17), spec_bit(18)};
static_assert(HU_SPEC_DENSE == (spec_bit(0) | spec_bit(1) | spec_bit(10) | spec_bit(11) | spec_bit(12) | spec_bit(15) | spec_bit(16)), "hip_util.h");
static_assert(HU_SPEC_BLOCKS == (spec_bit(2) | spec_bit(3) | spec_bit(10) | spec_bit(13) | spec_bit(14) | spec_bit(17) | spec_bit(18)), "hip_util.h");
static_assert(HU_SPEC_CLASSIFY == (spec_bit(4) | spec_bit(5) | spec_bit(6) | spec_bit(7) | spec_bit(10)), "hip_util.h");
static_assert(HU_SPEC_RENDER == (spec_bit(8) | spec_bit(9)), "hip_util.h");
static_assert(HU_SPEC_ALL == (HU_SPEC_DENSE | HU_SPEC_BLOCKS | HU_SPEC_CLASSIFY | HU_SPEC_RENDER) && HU_SPEC_ALL == spec_bit(kSpecKernelCount) - 1u, "hip_util.h");
const char* const kSpecKernelNames[kSpecKernelCount] = {
    "sdfk::k_grid_eval<sdfk::JitEval, 0, 2>",           "sdfk::k_grid_eval<sdfk::JitEval, 1, 2>",
    "sdfk::k_grid_eval_blocks<sdfk::JitEval, 0, 2>",    "sdfk::k_grid_eval_blocks<sdfk::JitEval, 1, 2>",
    "sdfk::k_classify<sdfk::JitEval, false, false, 2>", "sdfk::k_classify<sdfk::JitEval, false, true, 2>",
    "sdfk::k_classify<sdfk::JitEval, true, false, 2>",  "sdfk::k_classify<sdfk::JitEval, true, true, 2>",
    "sdfk::k_ray_caster<sdfk::JitEval>",                "sdfk::k_bitmap<sdfk::JitEval>",
    "sdfk::k_box_masks<sdfk::JitEval>",
    "sdfk::k_grid_eval_ragged<sdfk::JitEval, 0, 2>",        "sdfk::k_grid_eval_ragged<sdfk::JitEval, 1, 2>",
    "sdfk::k_grid_eval_blocks_ragged<sdfk::JitEval, 0, 2>", "sdfk::k_grid_eval_blocks_ragged<sdfk::JitEval, 1, 2>",
    "sdfk::k_grid_eval_runs<sdfk::JitEval, 0, 2>",          "sdfk::k_grid_eval_runs<sdfk::JitEval, 1, 2>",
    "sdfk::k_grid_eval_blocks_runs<sdfk::JitEval, 0, 2>",   "sdfk::k_grid_eval_blocks_runs<sdfk::JitEval, 1, 2>"};
