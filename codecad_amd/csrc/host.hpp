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

// hip_util.hip: dynamic LDS above 64 KiB for every interpreter kernel of the library, once per device and thread.  A unit
// that holds some says HU_BIG_LDS(its kernels, or arrays of them of any rank) once, at namespace scope: a static initialiser
// appends the unit's callback to a list that hu_ensure_attrs() walks (filled before any call, read only inside one).
int hu_ensure_attrs();
bool hu_big_lds_unit(hipError_t (*allow)(size_t bytes));
template <class... A> hipError_t hu_big_lds(size_t bytes, void (*kernel)(A...))
{
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
template <class T, size_t N> hipError_t hu_big_lds(size_t bytes, T (&kernels)[N])
{
    hipError_t e = hipSuccess;
    for (auto& k : kernels)
        if (e == hipSuccess) e = hu_big_lds(bytes, k);
    return e;
}
template <class... K> hipError_t hu_big_lds_all(size_t bytes, K&... kernels)
{
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? hu_big_lds(bytes, kernels) : e), ...);
    return e;
}
#define HU_BIG_LDS(...) \
    static const bool hu_big_lds_listed = hu_big_lds_unit([](size_t bytes) { return hu_big_lds_all(bytes, __VA_ARGS__); })

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
