// codecad_amd/csrc/host.hpp -- what the host code of every translation unit shares (private: not installed, and not the
// public include/hip_util.h): the thread's last error, the limits of the LDS register file and the workgroup-size rule.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/hip_util.h"

// hip_util.hip: sets the thread's last error (hu_last_error) and returns `code`; a HIP error (HU_ERR_HIP) is reported
// through the return code and not left sticky for the next launch check
int hu_fail(int code, const std::string& message);

#define HU_HIP(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return hu_fail(HU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr size_t kMaxLds = 160 * 1024;
constexpr size_t kScratchBytes = 128;

// hip_util.hip: dynamic LDS above 64 KiB for every interpreter kernel of the library, once per device and thread, through
// the hook of each unit that holds some
int hu_ensure_attrs();
namespace hu_render { hipError_t allow_big_lds(size_t bytes); }           // render.hip
namespace hu_cells {
hipError_t allow_big_lds(size_t bytes);                                   // instance_pairs.hip
hipError_t allow_big_lds_rays(size_t bytes);                              // instance_rays.hip
hipError_t allow_big_lds_section(size_t bytes);                           // instance_section.hip
hipError_t allow_big_lds_outline(size_t bytes);                           // instance_outline.hip
hipError_t allow_big_lds_layers(size_t bytes);                            // instance_layers.hip
hipError_t allow_big_lds_mass(size_t bytes);                             // instance_mass.hip
hipError_t allow_big_lds_mesh(size_t bytes);                              // instance_mesh.hip
hipError_t allow_big_lds_voxels(size_t bytes);                            // instance_voxels.hip
hipError_t allow_big_lds_gap(size_t bytes);                               // instance_gap.hip
}  // namespace hu_cells

// The workgroup of a kernel that keeps `lane_bytes` of LDS per lane (the interpreter's register file and what follows it
// per lane): the largest of 256, 128, 64 lanes that keeps them within 48 KiB (three workgroups or more per CU), else 64;
// `lds` is that and the scratch after it.  HU_ERR_UNSUPPORTED above 160 KiB, with `too_big` as the error (NULL: the
// caller has a message of its own).
inline int hu_workgroup(size_t lane_bytes, uint32_t& block, size_t& lds,
                        const char* too_big = "an instance keeps more values live than fit the 160 KiB LDS register file")
{
    block = 256;
    while (block > 64u && lane_bytes * block > 48 * 1024) block >>= 1;
    lds = lane_bytes * block + kScratchBytes;
    if (lds <= kMaxLds) return HU_OK;
    return too_big ? hu_fail(HU_ERR_UNSUPPORTED, too_big) : HU_ERR_UNSUPPORTED;
}
