// Per-ray code of bhn_eql_crossings: where a ray of the image-plane tracer meets the equatorial plane for the first, second, ...
// time (geodesics._integrate_crossings of bhnerf_amd/geodesics.py restated for one ray).
//
// No HIP dependency: equatorial.hip compiles it for the device (one lane per ray), tools/equatorial_host.cpp for the CPU with a
// plain C++ compiler.  The integration is kerr_trace.h's, in a single pass: the same initial state, step rule, RK4 step
// (kt_rk4_step), velocity re-derivation, capture and escape tests.  A taken step whose ends lie on opposite sides of theta = pi/2,
// or whose new end lies exactly on it, holds one crossing; its place w in (0, 1] of the step is the root of the cubic Hermite
// interpolant of theta over the step (values and derivatives at both ends: the interpolant the tracer writes its samples with),
// and the seven output rows are that Hermite combination at w.
//
// Root finder (eq_hermite_root): bisection on [0, 1], EQ_BISECTIONS halvings, always all of them.  The bracket keeps the sign of
// theta - pi/2 at the step's start on its lower end, so it never leaves [0, 1] and its upper end, which is returned, is never 0;
// after 53 halvings the two ends are neighbouring doubles (or equal), so w is accurate to rounding, and the remaining halvings
// change nothing.  No tolerance, no early exit: nothing in it can end differently on another back end.  Every expression keeps
// NumPy's order of operations and contraction is off, as in kerr_trace.h.
#pragma once
#include "kerr_trace.h"

#define EQ_ROWS KT_ROWS     // mino, r, theta, phi, t, vr, vth
#define EQ_BISECTIONS 64
#define EQ_HALF_PI 1.5707963267948966        // numpy.pi / 2
#define EQ_PLANE_MARGIN 1e-6                 // an observer this close to the plane is refused

// Why the arguments are outside the contract, or NULL.  Host only.
inline const char *eq_params_error(double spin, double inclination, double distance, double M, double h, double r_c, int32_t max_steps,
                                   int32_t nmax) {
    const char *why = kt_params_error(spin, inclination, distance, M, h, r_c, max_steps, 0);
    if (why) return why;
    if (nmax < 1) return "nmax must be at least 1";
    if (!(fabs(inclination - EQ_HALF_PI) > EQ_PLANE_MARGIN)) return "inclination must be away from pi/2: the observer sits in the plane";
    return nullptr;
}

// theta of the Hermite interpolant at w, minus pi/2
KT_HD double eq_theta_offset(double w, double dl, double th, double f, double thn, double fn) {
    const double w2 = w * w, w3 = w * w * w;
    const double c0 = 2 * w3 - 3 * w2 + 1, c1 = (w3 - 2 * w2 + w) * dl, c2 = 3 * w2 - 2 * w3, c3 = (w3 - w2) * dl;
    return kt_hermite(c0, c1, c2, c3, th, f, thn, fn) - EQ_HALF_PI;
}

// The place in (0, 1] at which the interpolant leaves the side of the plane it starts on (below: theta < pi/2 at w = 0).
KT_HD double eq_hermite_root(bool below, double dl, double th, double f, double thn, double fn) {
    double lo = 0.0, hi = 1.0;
    for (int it = 0; it < EQ_BISECTIONS; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double g = eq_theta_offset(mid, dl, th, f, thn, fn);
        const bool same = below ? g < 0.0 : g > 0.0;
        lo = same ? mid : lo;
        hi = same ? hi : mid;
    }
    return hi;
}

// One ray.  cross (7, n, nmax), count (n), status (n); this call writes column i of each, every element of it.
KT_HD void eq_trace_ray(const KtParams &p, int32_t nmax, double alpha, double beta, int64_t i, int64_t n, double *cross, int32_t *count,
                        int32_t *status) {
    const KtRay k = kt_make_ray(p, alpha, beta);
    const double vth_scale = kt_vth_scale(k);
    double *const out = cross + i * (int64_t)nmax;                              // row stride n * nmax
    const int64_t row = n * (int64_t)nmax;
    KtState y = kt_initial_state(p, k, beta);
    double mino = 0.0;
    int32_t found = 0, step = 0;
    bool done = false;
    while (step < p.max_steps && !done) {
        ++step;
        KtState k1;
        double dl;
        const KtState yn = kt_rk4_step(p, k, vth_scale, y, &k1, &dl);
        const bool captured = !(yn.r > p.r_cap);                               // (also a NaN): the step is not taken
        if (!captured) {
            const double d0 = y.th - EQ_HALF_PI, d1 = yn.th - EQ_HALF_PI;
            if ((d0 < 0.0 && d1 > 0.0) || (d0 > 0.0 && d1 < 0.0) || d1 == 0.0) {
                const KtState fn = kt_rhs(k, yn);
                const double w = eq_hermite_root(d0 < 0.0, dl, y.th, k1.th, yn.th, fn.th);
                kt_store(out + found, row, mino + w * dl, kt_hermite_state(w, dl, y, k1, yn, fn));
                ++found;
            }
            y = yn;
            mino = mino + dl;
        }
        done = captured || (y.r > p.distance && y.vr > 0.0) || found >= nmax;
    }
    status[i] = done ? step : -1;
    count[i] = found;
    const double nan = NAN;
    for (int32_t j = found; j < nmax; ++j)
        for (int r = 0; r < EQ_ROWS; ++r) out[r * row + j] = nan;
}
