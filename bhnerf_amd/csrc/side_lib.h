// Host-side skeleton of a side library (libbhnerf_kerr.so, libbhnerf_eht.so, libbhnerf_grf.so, libbhnerf_eql.so, libbhnerf_flow.so, libbhnerf_rec.so, libbhnerf_cls.so, libbhnerf_pol.so, libbhnerf_reg.so, libbhnerf_jnt.so): the per-thread error message, the
// argument check and, under hipcc, the launch check and the grid size of a one-lane-per-element launch.
//
// No HIP dependency outside the __HIPCC__ block: tools/side_lib_host.cpp compiles the rest with a plain C++ compiler and runs it
// under a sanitizer.  Included by the one .hip file of each side library and by nothing of libbhnerf_hip.so.  A library exports
// the message under its own name:   extern "C" const char *bhn_<x>_last_error(void) { return side_last_error(); }
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include "../../include/bhnerf_hip.h"        // BHN_OK / BHN_EINVAL / BHN_EHIP

static thread_local char g_side_err[512] = "";

// the message of the calling thread's last failure: never longer than 511 characters, always terminated
static inline int side_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_side_err, sizeof(g_side_err), fmt, ap);
    va_end(ap);
    return code;
}

static inline const char *side_last_error(void) { return g_side_err; }

#define BHN_CHECK_ARG(cond, ...) \
    do {                         \
        if (!(cond)) return side_fail(BHN_EINVAL, __VA_ARGS__); \
    } while (0)

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// after a launch: BHN_OK, or BHN_EHIP with the runtime's message
static inline int side_launched(const char *kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return side_fail(BHN_EHIP, "launch of %s failed: %s", kernel, hipGetErrorString(e));
    return BHN_OK;
}

// workgroups of `block` lanes over `total` elements, or 0 when there are none or more than one launch takes
static inline long long side_blocks(long long total, int block) {
    if (total < 1) return 0;
    const long long blocks = total / block + (total % block != 0);
    return blocks <= 0x7fffffffLL ? blocks : 0;
}
#endif
