// libbhnerf_grf.so: Doppler factor, fluid-frame magnetic field, domain mean and polarised transport factors of kgeo.py on the device.
//
// One lane per sample point, workgroups of GRF_BLOCK = 256 lanes over the n * ngeo points (gr_factors.h holds the per-point
// arithmetic, shared with the CPU build of tools/gr_factors_host.cpp).  Point p = ray * ngeo + k reads its fields at p and, for the
// signs of the wave vector, r / theta / affine at p -+ 1 of the same ray: adjacent lanes, adjacent addresses.  No LDS, no atomics and
// no cross-lane operation outside the domain mean, whose two stages sum in one fixed order (an LDS tree per workgroup into the
// caller's workspace, then one workgroup over the partial sums).  All arithmetic is float64.
//
// Built into a library of its own (include/bhnerf_grf.h): the ABIs of the other three libraries are not touched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_grf.h"
#include "gr_factors.h"
#include "side_lib.h"

extern "C" const char *bhn_grf_last_error(void) { return side_last_error(); }

__global__ __launch_bounds__(GRF_BLOCK) void grf_doppler_kernel(GrfGeos g, const double *__restrict__ Omega, double fillna, int fill,
                                                                double *__restrict__ out, long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    out[p] = grf_point_doppler(g, p, Omega[p], fillna, fill);
}

__global__ __launch_bounds__(GRF_BLOCK) void grf_fluid_field_kernel(GrfGeos g, const double *__restrict__ Omega, double arad, double avert,
                                                                    double ator, double *__restrict__ b, long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    double v[3];
    grf_point_fluid_field(g, p, Omega[p], arad, avert, ator, v);
    for (int i = 0; i < 3; ++i) b[3 * p + i] = v[i];
}

// v[0] of the tree sum over the workgroup's GRF_BLOCK values, the order of grf_tree_sum_host
__device__ __forceinline__ void grf_tree_sum(double *v) {
    for (int s = GRF_BLOCK / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) v[threadIdx.x] += v[threadIdx.x + s];
    }
    __syncthreads();
}

// stage 1: partial[block] = sum of |b| over the block's selected points, count[block] = how many
__global__ __launch_bounds__(GRF_BLOCK) void grf_domain_partial_kernel(GrfGeos g, const double *__restrict__ b, double z_width, double rmin,
                                                                       double rmax, double *__restrict__ partial, double *__restrict__ count,
                                                                       long long total) {
    __shared__ double s_sum[GRF_BLOCK], s_cnt[GRF_BLOCK];
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    double mag = 0.0, one = 0.0;
    if (p < total && grf_in_domain(g, p, z_width, rmin, rmax)) {
        const double v[3] = {b[3 * p], b[3 * p + 1], b[3 * p + 2]};
        mag = grf_field_magnitude(v);
        one = 1.0;
    }
    s_sum[threadIdx.x] = mag;
    s_cnt[threadIdx.x] = one;
    grf_tree_sum(s_sum);
    grf_tree_sum(s_cnt);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s_sum[0];
        count[blockIdx.x] = s_cnt[0];
    }
}

// stage 2, one workgroup: lane t sums partial[t], partial[t + 256], .. in that order, then the same tree; mean = sum / count
__global__ __launch_bounds__(GRF_BLOCK) void grf_domain_final_kernel(const double *__restrict__ partial, const double *__restrict__ count,
                                                                     long long blocks, double *__restrict__ mean) {
    __shared__ double s_sum[GRF_BLOCK], s_cnt[GRF_BLOCK];
    double s = 0.0, c = 0.0;
    for (long long i = threadIdx.x; i < blocks; i += GRF_BLOCK) {
        s += partial[i];
        c += count[i];
    }
    s_sum[threadIdx.x] = s;
    s_cnt[threadIdx.x] = c;
    grf_tree_sum(s_sum);
    grf_tree_sum(s_cnt);
    if (threadIdx.x == 0) mean[0] = s_sum[0] / s_cnt[0];
}

__global__ __launch_bounds__(GRF_BLOCK) void grf_transport_kernel(GrfGeos g, const double *__restrict__ Omega, const double *__restrict__ gfac,
                                                                  const double *__restrict__ b, const double *__restrict__ divisor,
                                                                  double Q_frac, double V_frac, double spectral_index, int with_v,
                                                                  double *__restrict__ J, long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    double v[3] = {b[3 * p], b[3 * p + 1], b[3 * p + 2]};
    if (divisor) {
        const double d = divisor[0];
        for (int i = 0; i < 3; ++i) v[i] = v[i] / d;
    }
    double out[4];
    grf_point_transport(g, p, Omega[p], gfac[p], v, Q_frac, V_frac, spectral_index, with_v, out);
    const int S = with_v ? 4 : 3;
    for (int s = 0; s < S; ++s) J[(long long)s * total + p] = out[s];
}

// blocks of GRF_BLOCK points over n * ngeo, or 0 when the sizes are outside what one launch takes
static long long grf_blocks(int64_t n, int32_t ngeo) {
    if (n < 1 || ngeo < 2) return 0;
    if (n > ((int64_t)1 << 40) / ngeo) return 0;                  // 4 n ngeo doubles of J stay far inside 2^63 bytes
    return side_blocks((long long)n * ngeo, GRF_BLOCK);
}

// Checks the record, which every entry point takes, and fills the kernels' view of it; the message is set on failure
static int grf_prepare(const bhn_grf_geos *geos, GrfGeos *out, long long *blocks) {
    BHN_CHECK_ARG(geos, "null geos");
    GrfGeos g;
    g.n = geos->n;
    g.ngeo = geos->ngeo;
    g.r = geos->r; g.theta = geos->theta; g.affine = geos->affine; g.Delta = geos->Delta; g.Sigma = geos->Sigma; g.Xi = geos->Xi;
    g.R = geos->R; g.Theta = geos->Theta; g.lam = geos->lam; g.alpha = geos->alpha; g.beta = geos->beta;
    g.a = geos->spin; g.M = geos->M; g.E = geos->E;
    g.sin_inc = sin(geos->inc);
    const char *why = grf_geos_error(g);
    BHN_CHECK_ARG(!why, "%s (n %lld, ngeo %d)", why, (long long)geos->n, geos->ngeo);
    *blocks = grf_blocks(geos->n, geos->ngeo);
    BHN_CHECK_ARG(*blocks > 0, "too many points (n %lld, ngeo %d) for one launch", (long long)geos->n, geos->ngeo);
    *out = g;
    return BHN_OK;
}

extern "C" size_t bhn_grf_ws_bytes(int64_t n, int32_t ngeo) { return (size_t)grf_blocks(n, ngeo) * 2 * sizeof(double); }

extern "C" int bhn_grf_doppler(const bhn_grf_geos *geos, const double *Omega, double fillna, int32_t fill, double *g, void *stream) {
    GrfGeos k;
    long long blocks;
    if (int rc = grf_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(Omega, "null Omega");
    BHN_CHECK_ARG(g, "null output g");
    hipLaunchKernelGGL(grf_doppler_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, Omega, fillna, fill != 0, g,
                       k.n * k.ngeo);
    return side_launched("grf_doppler_kernel");
}

extern "C" int bhn_grf_fluid_field(const bhn_grf_geos *geos, const double *Omega, double arad, double avert, double ator, double *b,
                                   void *stream) {
    GrfGeos k;
    long long blocks;
    if (int rc = grf_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(Omega, "null Omega");
    BHN_CHECK_ARG(b, "null output b");
    hipLaunchKernelGGL(grf_fluid_field_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, Omega, arad, avert, ator, b,
                       k.n * k.ngeo);
    return side_launched("grf_fluid_field_kernel");
}

extern "C" int bhn_grf_domain_mean(const bhn_grf_geos *geos, const double *b, double z_width, double rmin, double rmax, double *mean,
                                   void *ws, size_t ws_bytes, void *stream) {
    GrfGeos k;
    long long blocks;
    if (int rc = grf_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(b && mean, "null b or mean");
    BHN_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0, "null or misaligned workspace");
    const size_t need = (size_t)blocks * 2 * sizeof(double);
    if (ws_bytes < need) return side_fail(BHN_EWORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes, need);
    double *partial = (double *)ws, *count = partial + blocks;
    hipLaunchKernelGGL(grf_domain_partial_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, b, z_width, rmin, rmax,
                       partial, count, k.n * k.ngeo);
    if (int rc = side_launched("grf_domain_partial_kernel")) return rc;
    hipLaunchKernelGGL(grf_domain_final_kernel, dim3(1), dim3(GRF_BLOCK), 0, (hipStream_t)stream, partial, count, blocks, mean);
    return side_launched("grf_domain_final_kernel");
}

extern "C" int bhn_grf_transport(const bhn_grf_geos *geos, const double *Omega, const double *g, const double *b, const double *divisor,
                                 double Q_frac, double V_frac, double spectral_index, double *J, void *stream) {
    GrfGeos k;
    long long blocks;
    if (int rc = grf_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(Omega, "null Omega");
    BHN_CHECK_ARG(g && b && J, "null g, b or J");
    BHN_CHECK_ARG(!(Q_frac > 1.0 || Q_frac < 0.0), "Q_frac should be in [0,1], not %g", Q_frac);
    hipLaunchKernelGGL(grf_transport_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, Omega, g, b, divisor, Q_frac,
                       V_frac, spectral_index, V_frac != 0.0 ? 1 : 0, J, k.n * k.ngeo);
    return side_launched("grf_transport_kernel");
}
