// bhn_kerr_trace: the image-plane Kerr ray tracer of bhnerf_amd/geodesics.py (_integrate) on the device.
//
// One lane per ray, both passes of a ray in the same lane (kerr_trace.h holds the stepping code, shared with the CPU build of
// tools/kerr_trace_host.cpp).  The rays are independent: no LDS, no atomics, no cross-lane operation, so a ray's result depends on
// nothing but its own (alpha, beta) and two launches give the same bytes.  All arithmetic is float64.  Workgroups of ONE wave: the
// time of a launch is the step count of its slowest ray (4,000-20,000 dependent RK4 steps per pass), not the ray count, so a
// 128 x 128 image is spread as 256 single waves over the 256 CUs instead of filling a handful of them.
//
// Built into a library of its own, libbhnerf_kerr.so (include/bhnerf_kerr.h): the ABI of libbhnerf_hip.so is not touched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_kerr.h"
#include "kerr_trace.h"
#include "side_lib.h"

extern "C" const char *bhn_kerr_last_error(void) { return side_last_error(); }

#define KT_BLOCK 64

__global__ __launch_bounds__(KT_BLOCK) void kerr_trace_kernel(const double *__restrict__ alpha, const double *__restrict__ beta, long long n,
                                                              KtParams p, double *__restrict__ samples, double *__restrict__ end,
                                                              int32_t *__restrict__ status) {
    const long long i = (long long)blockIdx.x * KT_BLOCK + threadIdx.x;
    if (i >= n) return;
    kt_trace_ray(p, alpha[i], beta[i], i, n, samples, end, status);
}

extern "C" int bhn_kerr_trace(const double *alpha, const double *beta, int64_t n, double spin, double inclination, double distance,
                              double M, double h, double r_c, int32_t max_steps, int32_t ngeo, double *samples, double *end,
                              int32_t *status, void *stream) {
    BHN_CHECK_ARG(alpha && beta && end && status, "null pointer");
    BHN_CHECK_ARG(n >= 1, "bad ray count n=%lld", (long long)n);
    const char *why = kt_params_error(spin, inclination, distance, M, h, r_c, max_steps, ngeo);
    BHN_CHECK_ARG(!why, "%s (spin %g, inclination %g, M %g, h %g, r_c %g, max_steps %d, ngeo %d)", why, spin, inclination, M, h, r_c,
                  max_steps, ngeo);
    BHN_CHECK_ARG(ngeo == 0 || samples, "ngeo = %d samples per ray asked for, samples is NULL", ngeo);
    const long long blocks = side_blocks(n, KT_BLOCK);
    BHN_CHECK_ARG(blocks > 0, "too many rays (%lld) for one launch", (long long)n);
    const KtParams p = kt_make_params(spin, inclination, distance, M, h, r_c, max_steps, ngeo);
    hipLaunchKernelGGL(kerr_trace_kernel, dim3((unsigned)blocks), dim3(KT_BLOCK), 0, (hipStream_t)stream, alpha, beta, (long long)n, p,
                       samples, end, status);
    return side_launched("kerr_trace_kernel");
}
