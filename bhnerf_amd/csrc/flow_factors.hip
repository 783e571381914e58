// libbhnerf_flow.so: Doppler factor, fluid-frame magnetic field and polarised transport factors of kgeo.py for a general 4-velocity
// (a umu array per point, or the boosted ZAMO) on the device.
//
// One lane per sample point, workgroups of GRF_BLOCK = 256 lanes over the n * ngeo points (flow_factors.h, on gr_factors.h, holds the
// per-point arithmetic, shared with the CPU build of tools/flow_factors_host.cpp).  Point p = ray * ngeo + k reads its fields and
// its umu at p and, for the signs of the wave vector, r / theta / affine at p -+ 1 of the same ray.  No LDS, no atomics, no
// cross-lane operation.  All arithmetic is float64.
//
// Built into a library of its own (include/bhnerf_flow.h): the ABIs of the other five libraries are not touched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_flow.h"
#include "flow_factors.h"
#include "side_lib.h"

extern "C" const char *bhn_flow_last_error(void) { return side_last_error(); }

__global__ __launch_bounds__(GRF_BLOCK) void flow_zamo_velocity_kernel(FlowGeos g, double beta, double chi, double *__restrict__ umu,
                                                                       long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    double u[4];
    flow_zamo_frame_velocity(g, p, beta, chi, u);
    for (int i = 0; i < 4; ++i) umu[4 * p + i] = u[i];
}

__global__ __launch_bounds__(GRF_BLOCK) void flow_doppler_kernel(FlowGeos g, const double *__restrict__ umu, double fillna, int fill,
                                                                 double *__restrict__ out, long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    const double u[4] = {umu[4 * p], umu[4 * p + 1], umu[4 * p + 2], umu[4 * p + 3]};
    out[p] = flow_point_doppler(g, p, u, fillna, fill);
}

__global__ __launch_bounds__(GRF_BLOCK) void flow_fluid_field_kernel(FlowGeos g, const double *__restrict__ umu, double arad, double avert,
                                                                     double ator, double *__restrict__ b, long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    const double u[4] = {umu[4 * p], umu[4 * p + 1], umu[4 * p + 2], umu[4 * p + 3]};
    double v[3];
    flow_point_fluid_field(g, p, u, arad, avert, ator, v);
    for (int i = 0; i < 3; ++i) b[3 * p + i] = v[i];
}

// umu != NULL: the fluid tetrad of umu (S = 4 when with_v); umu == NULL: the ZAMO tetrad of (beta, chi), S = 3
__global__ __launch_bounds__(GRF_BLOCK) void flow_transport_kernel(FlowGeos g, const double *__restrict__ umu, double beta, double chi,
                                                                   const double *__restrict__ gfac, const double *__restrict__ b,
                                                                   const double *__restrict__ divisor, double Q_frac, double V_frac,
                                                                   double spectral_index, int with_v, double *__restrict__ J,
                                                                   long long total) {
    const long long p = (long long)blockIdx.x * GRF_BLOCK + threadIdx.x;
    if (p >= total) return;
    double v[3] = {b[3 * p], b[3 * p + 1], b[3 * p + 2]};
    if (divisor) {
        const double d = divisor[0];
        for (int i = 0; i < 3; ++i) v[i] = v[i] / d;
    }
    double out[4];
    if (umu) {
        const double u[4] = {umu[4 * p], umu[4 * p + 1], umu[4 * p + 2], umu[4 * p + 3]};
        flow_point_transport(g, p, u, gfac[p], v, Q_frac, V_frac, spectral_index, with_v, out);
    } else {
        flow_point_transport_zamo(g, p, beta, chi, gfac[p], v, Q_frac, spectral_index, out);
    }
    const int S = with_v ? 4 : 3;
    for (int s = 0; s < S; ++s) J[(long long)s * total + p] = out[s];
}

// Checks the record, which every entry point takes, and fills the kernels' view of it; the message is set on failure
static int flow_prepare(const bhn_flow_geos *geos, FlowGeos *out, long long *blocks) {
    BHN_CHECK_ARG(geos, "null geos");
    FlowGeos g;
    g.n = geos->n;
    g.ngeo = geos->ngeo;
    g.r = geos->r; g.theta = geos->theta; g.affine = geos->affine; g.Delta = geos->Delta; g.Sigma = geos->Sigma; g.Xi = geos->Xi;
    g.R = geos->R; g.Theta = geos->Theta; g.lam = geos->lam; g.alpha = geos->alpha; g.beta = geos->beta;
    g.a = geos->spin; g.M = geos->M; g.E = geos->E;
    g.sin_inc = sin(geos->inc);
    g.omega = geos->omega;
    const char *why = flow_geos_error(g);
    BHN_CHECK_ARG(!why, "%s (n %lld, ngeo %d)", why, (long long)geos->n, geos->ngeo);
    // 4 n ngeo doubles of umu or J stay far inside 2^63 bytes
    *blocks = geos->n > ((int64_t)1 << 40) / geos->ngeo ? 0 : side_blocks((long long)geos->n * geos->ngeo, GRF_BLOCK);
    BHN_CHECK_ARG(*blocks > 0, "too many points (n %lld, ngeo %d) for one launch", (long long)geos->n, geos->ngeo);
    *out = g;
    return BHN_OK;
}

extern "C" int bhn_flow_zamo_velocity(const bhn_flow_geos *geos, double beta, double chi, double *umu, void *stream) {
    FlowGeos k;
    long long blocks;
    if (int rc = flow_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(umu, "null output umu");
    hipLaunchKernelGGL(flow_zamo_velocity_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, beta, chi, umu,
                       k.n * k.ngeo);
    return side_launched("flow_zamo_velocity_kernel");
}

extern "C" int bhn_flow_doppler(const bhn_flow_geos *geos, const double *umu, double fillna, int32_t fill, double *g, void *stream) {
    FlowGeos k;
    long long blocks;
    if (int rc = flow_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(umu, "null umu");
    BHN_CHECK_ARG(g, "null output g");
    hipLaunchKernelGGL(flow_doppler_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, umu, fillna, fill != 0, g,
                       k.n * k.ngeo);
    return side_launched("flow_doppler_kernel");
}

extern "C" int bhn_flow_fluid_field(const bhn_flow_geos *geos, const double *umu, double arad, double avert, double ator, double *b,
                                    void *stream) {
    FlowGeos k;
    long long blocks;
    if (int rc = flow_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(umu, "null umu");
    BHN_CHECK_ARG(b, "null output b");
    hipLaunchKernelGGL(flow_fluid_field_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, umu, arad, avert, ator, b,
                       k.n * k.ngeo);
    return side_launched("flow_fluid_field_kernel");
}

extern "C" int bhn_flow_transport(const bhn_flow_geos *geos, const double *umu, const double *g, const double *b, const double *divisor,
                                  double Q_frac, double V_frac, double spectral_index, double *J, void *stream) {
    FlowGeos k;
    long long blocks;
    if (int rc = flow_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(umu, "null umu");
    BHN_CHECK_ARG(g && b && J, "null g, b or J");
    BHN_CHECK_ARG(!(Q_frac > 1.0 || Q_frac < 0.0), "Q_frac should be in [0,1], not %g", Q_frac);
    hipLaunchKernelGGL(flow_transport_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, umu, 0.0, 0.0, g, b, divisor,
                       Q_frac, V_frac, spectral_index, V_frac != 0.0 ? 1 : 0, J, k.n * k.ngeo);
    return side_launched("flow_transport_kernel");
}

extern "C" int bhn_flow_transport_zamo(const bhn_flow_geos *geos, double beta, double chi, const double *g, const double *b,
                                       const double *divisor, double Q_frac, double spectral_index, double *J, void *stream) {
    FlowGeos k;
    long long blocks;
    if (int rc = flow_prepare(geos, &k, &blocks)) return rc;
    BHN_CHECK_ARG(g && b && J, "null g, b or J");
    BHN_CHECK_ARG(!(Q_frac > 1.0 || Q_frac < 0.0), "Q_frac should be in [0,1], not %g", Q_frac);
    hipLaunchKernelGGL(flow_transport_kernel, dim3((unsigned)blocks), dim3(GRF_BLOCK), 0, (hipStream_t)stream, k, (const double *)nullptr, beta,
                       chi, g, b, divisor, Q_frac, 0.0, spectral_index, 0, J, k.n * k.ngeo);
    return side_launched("flow_transport_kernel");
}
