// bhn_eql_crossings: the equatorial crossings of image-plane Kerr rays (geodesics.equatorial_crossings) on the device.
//
// One lane per ray, one pass (equatorial.h holds the per-ray code, shared with the CPU build of tools/equatorial_host.cpp; the RK4
// step is kerr_trace.h's, the one bhn_kerr_trace runs).  The rays are independent: no LDS, no atomics, no cross-lane operation, so a
// ray's columns depend on nothing but its own (alpha, beta) and two launches give the same bytes.  All arithmetic is float64.
// Workgroups of ONE wave, as in kerr_trace.hip: a launch lasts as long as its slowest ray.
//
// Built into a library of its own, libbhnerf_eql.so (include/bhnerf_eql.h): the symbol tables of the other libraries are not touched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_eql.h"
#include "equatorial.h"
#include "side_lib.h"

extern "C" const char *bhn_eql_last_error(void) { return side_last_error(); }

#define EQ_BLOCK 64

__global__ __launch_bounds__(EQ_BLOCK) void eql_crossings_kernel(const double *__restrict__ alpha, const double *__restrict__ beta, long long n,
                                                                 KtParams p, int32_t nmax, double *__restrict__ cross,
                                                                 int32_t *__restrict__ count, int32_t *__restrict__ status) {
    const long long i = (long long)blockIdx.x * EQ_BLOCK + threadIdx.x;
    if (i >= n) return;
    eq_trace_ray(p, nmax, alpha[i], beta[i], i, n, cross, count, status);
}

extern "C" int bhn_eql_crossings(const double *alpha, const double *beta, int64_t n, double spin, double inclination, double distance,
                                 double M, double h, double r_c, int32_t max_steps, int32_t nmax, double *cross, int32_t *count,
                                 int32_t *status, void *stream) {
    BHN_CHECK_ARG(alpha && beta && cross && count && status, "null pointer");
    BHN_CHECK_ARG(n >= 1, "bad ray count n=%lld", (long long)n);
    const char *why = eq_params_error(spin, inclination, distance, M, h, r_c, max_steps, nmax);
    BHN_CHECK_ARG(!why, "%s (spin %g, inclination %g, M %g, h %g, r_c %g, max_steps %d, nmax %d)", why, spin, inclination, M, h, r_c,
                  max_steps, nmax);
    const long long blocks = side_blocks(n, EQ_BLOCK);
    BHN_CHECK_ARG(blocks > 0, "too many rays (%lld) for one launch", (long long)n);
    const KtParams p = kt_make_params(spin, inclination, distance, M, h, r_c, max_steps, 0);
    hipLaunchKernelGGL(eql_crossings_kernel, dim3((unsigned)blocks), dim3(EQ_BLOCK), 0, (hipStream_t)stream, alpha, beta, (long long)n, p,
                       nmax, cross, count, status);
    return side_launched("eql_crossings_kernel");
}
