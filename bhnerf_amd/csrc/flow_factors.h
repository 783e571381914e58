// Per-point arithmetic of libbhnerf_flow.so: the GR pre-compute of bhnerf_amd/kgeo.py for a GENERAL 4-velocity -- one handed in per
// point, or the boosted ZAMO of kgeo.zamo_frame_velocity -- restated for one sample point of one ray.
//
// No HIP dependency: flow_factors.hip compiles it for the device (one lane per sample point), tools/flow_factors_host.cpp for the CPU
// with a plain C++ compiler.  It stands on gr_factors.h (metric, wave vector, index lowering, the fluid tetrad of a given umu, the
// field, the transport in a frame) and keeps its rules: float64, floating-point contraction off, NumPy's order of operations
// expression for expression, nothing clamped -- beta >= 1 gives the NaN or inf that NumPy gives.
//
// 4-vectors are (t, r, theta, phi); a umu array is (n, ngeo, 4), the component index last, as the Python functions return it.
#pragma once
#include "gr_factors.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// The record of gr_factors.h and the frame-dragging frequency omega = 2 a M r / Xi per point, which the ZAMO functions read
struct FlowGeos : GrfGeos {
    const double *omega;
};

// What the ZAMO functions share: gam = 1 / sqrt(1 - beta^2), cos / sin chi, sqrt(Xi / Delta), sqrt(Delta), sqrt(Xi)
struct FlowZamo {
    double r, om, gam, c, s, sxd, sd, sx;
};

GRF_HD FlowZamo flow_zamo(const FlowGeos &g, long long p, double beta, double chi) {
    FlowZamo z;
    z.r = g.r[p];
    z.om = g.omega[p];
    z.gam = 1.0 / sqrt(1.0 - beta * beta);
    z.c = cos(chi);
    z.s = sin(chi);
    z.sxd = sqrt(g.Xi[p] / g.Delta[p]);
    z.sd = sqrt(g.Delta[p]);
    z.sx = sqrt(g.Xi[p]);
    return z;
}

// zamo_frame_velocity: the observer boosted by beta at angle chi relative to the ZAMO
GRF_HD void flow_zamo_frame_velocity(const FlowGeos &g, long long p, double beta, double chi, double umu[4]) {
    const FlowZamo z = flow_zamo(g, p, beta, chi);
    const double ut = (z.gam / z.r) * z.sxd;
    umu[0] = ut;
    umu[1] = (beta * z.gam * z.c / z.r) * z.sd;
    umu[2] = 0.0;
    umu[3] = ut * z.om + z.r * beta * z.gam * z.s / z.sx;
}

// zamo_frame_tetrad (Gelles et al. 2021, eq. A4): e[mu][a], component index then leg
GRF_HD void flow_zamo_frame_tetrad(const FlowGeos &g, long long p, double beta, double chi, double e[4][4]) {
    const FlowZamo z = flow_zamo(g, p, beta, chi);
    const double r = z.r, om = z.om, gam = z.gam, c = z.c, s = z.s, sxd = z.sxd, sd = z.sd, sx = z.sx;
    e[0][0] = (gam / r) * sxd;
    e[1][0] = (beta * gam * c / r) * sd;
    e[2][0] = 0.0;
    e[3][0] = (gam * om / r) * sxd + r * beta * gam * s / sx;
    e[0][1] = (beta * gam * c / r) * sxd;
    e[1][1] = ((1.0 + (gam - 1.0) * (c * c)) / r) * sd;
    e[2][1] = 0.0;
    e[3][1] = beta * gam * om * c / r * sxd + r * (gam - 1.0) * c * s / sx;
    e[0][2] = 0.0;
    e[1][2] = 0.0;
    e[2][2] = 1.0 / r;
    e[3][2] = 0.0;
    e[0][3] = (beta * gam * s / r) * sxd;
    e[1][3] = ((gam - 1.0) * c * s / r) * sd;
    e[2][3] = 0.0;
    e[3][3] = beta * om * s * (gam / r) * sxd + r * ((gam - 1.0) * (s * s) + 1.0) / sx;
}

// The frame co-moving with a given umu: metric, u_mu, fluid_frame_tetrad
GRF_HD void flow_frame(const GrfGeos &g, long long p, const double umu[4], GrfFrame &f) {
    f.sin_th = sin(g.theta[p]);
    f.cos_th = cos(g.theta[p]);
    f.m = grf_spacetime_metric(g, p, f.sin_th);
    for (int i = 0; i < 4; ++i) f.umu[i] = umu[i];
    grf_raise_or_lower_indices(f.m, f.umu, f.u_mu);
    grf_fluid_frame_tetrad(f.m, f.umu, f.u_mu, g.Delta[p], f.sin_th, f.e);
}

// ---- the per-point bodies of the library's kernels

// doppler_factor(geos, umu, fillna)
GRF_HD double flow_point_doppler(const GrfGeos &g, long long p, const double umu[4], double fillna, int fill) {
    const long long ray = p / g.ngeo;
    const int k = (int)(p - ray * g.ngeo);
    double kmu[4];
    grf_wave_vector(g, ray, k, kmu);
    return grf_doppler_factor(g, kmu, umu, fillna, fill);
}

// magnetic_field_fluid_frame(geos, umu, arad, avert, ator)
GRF_HD void flow_point_fluid_field(const GrfGeos &g, long long p, const double umu[4], double arad, double avert, double ator, double b[3]) {
    GrfFrame f;
    flow_frame(g, p, umu, f);
    grf_magnetic_field_fluid_frame(f.m, f.u_mu, f.e, f.sin_th, f.cos_th, arad, avert, ator, b);
}

// parallel_transport(geos, umu, g, b, ...): the transport of gr_factors.h in the fluid tetrad of umu; J[3] = V when with_v
GRF_HD void flow_point_transport(const GrfGeos &g, long long p, const double umu[4], double gfac, const double b[3], double Q_frac,
                                 double V_frac, double spectral_index, int with_v, double J[4]) {
    GrfFrame f;
    flow_frame(g, p, umu, f);
    grf_transport_in_frame(g, p, f, gfac, b, Q_frac, V_frac, spectral_index, with_v, J);
}

// parallel_transport_zamo(geos, beta, chi, g, b, ...): the same in the boosted ZAMO tetrad, J[0..2] = I, Q, U
GRF_HD void flow_point_transport_zamo(const FlowGeos &g, long long p, double beta, double chi, double gfac, const double b[3],
                                      double Q_frac, double spectral_index, double J[4]) {
    GrfFrame f;                                   // the transport reads e, sin_th and cos_th of it
    f.sin_th = sin(g.theta[p]);
    f.cos_th = cos(g.theta[p]);
    flow_zamo_frame_tetrad(g, p, beta, chi, f.e);
    grf_transport_in_frame(g, p, f, gfac, b, Q_frac, 0.0, spectral_index, 0, J);
}

// Why the arguments are outside the contract, or NULL.  Host only.
inline const char *flow_geos_error(const FlowGeos &g) {
    if (!g.omega) return "null field in geos";
    return grf_geos_error(g);
}
