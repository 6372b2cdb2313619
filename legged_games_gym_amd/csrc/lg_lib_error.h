// lg_lib_error.h -- what every single-unit library says about a refused call: the thread's last message, refuse(), the two forms of HIP_TRY
// and raise_lds_limit.  Everything has internal linkage: each library that includes it keeps a message text of its own, returned by its own
// *_last_error entry point.  The main library does not include it (lg::fail and lg_last_error, lg_kernels.hip).  Include it after
// lg_host.h where a unit reads that header: HIP_TRY is redefined here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace lg {

static thread_local char g_error[512] = "";
static int refuse(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

// A dynamic-LDS size above the 64 KB a kernel gets without asking: hipFuncSetAttribute once per device for this process, at the first call
// (not capture-safe: the first call happens in a warm-up, outside any capture)
[[maybe_unused]] static hipError_t raise_lds_limit(const void *kernel, const size_t bytes, bool (&raised)[64]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
    return hipSuccess;
}

}  // namespace lg

#undef HIP_TRY                     // lg_host.h's reports through the main library's lg::fail
#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::refuse(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)
// in an entry point that names itself: static const char *const who = "lg_...";
#define HIP_TRY_WHO(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::refuse(-10, "%s: HIP error: %s", who, hipGetErrorString(_e)); } while (0)
