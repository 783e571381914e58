/*
 * bhnerf_kerr.h -- C ABI of libbhnerf_kerr.so: the image-plane Kerr ray tracer behind kgeo.image_plane_geos (kgeo.py:6-63; the
 * reference calls the external kgeo.raytrace_ana there) on the MI355X (gfx950).
 *
 * A library of its own, beside libbhnerf_hip.so: the tracer is the float64 geodesic pre-compute that runs once per ray set, not a
 * piece of the training step, and the ABI of include/bhnerf_hip.h (version 5, 33 entry points) stays exactly what it is.  The
 * conventions are that header's: 0 on success or a BHN_E* code (bhn_kerr_last_error() gives a thread-local message; nothing aborts,
 * nothing prints); the CALLER owns every buffer, what an output holds on entry is irrelevant and every element of it is written,
 * nothing outside the array shapes named here is; no allocation, no synchronisation, no environment reads, no state but the error
 * string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the calling thread's current device.
 */
#ifndef BHNERF_KERR_H
#define BHNERF_KERR_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP */

#ifdef __cplusplus
extern "C" {
#endif

BHN_API const char *bhn_kerr_last_error(void);

/* bhnerf_amd/geodesics.py `_integrate` restated on the device -- the same scheme, step rule and constants, one lane per ray
 * (csrc/kerr_trace.h holds the stepping code; it also compiles for the CPU).  Ray i starts at r = distance, theta = inclination
 * with lam = -alpha[i] sin(inclination), eta = (alpha[i]^2 - a^2) cos^2(inclination) + beta[i]^2 (a = spin M) and is followed backwards
 * in Mino time by classical RK4 with the step h (1 + r/r_c) / r^2 * clip((sin theta / 0.25)^2, 0.05, 1) until a step would end at
 * !(r > 1.02 r_hor) (captured; that step is not taken) or r > distance with v_r > 0 (escaped).  A second pass over the same steps
 * writes ngeo samples per ray at k / ngeo of the ray's final Mino time (k = 1..ngeo; cubic Hermite inside the crossing step);
 * samples a ray does not reach (a captured ray's, a last one missed by rounding) hold its end state.  All float64, device memory:
 *   alpha, beta (n);  samples (7, n, ngeo), rows mino, r, theta, phi, t, v_r, v_theta -- may be NULL when ngeo = 0 (end states only);
 *   end (7, n): final Mino time, then r, theta, phi, t, v_r, v_theta;  status (n) int32: steps the first pass took, or -1 when the
 *   ray was not finished after max_steps (its `end` column and its samples then hold the state reached: non-termination is data, a
 *   launch is bounded by 2 max_steps steps per lane).  phi and t are those of the forward equations: the caller negates them.
 * Every element of samples, end and status is written.  Rays are independent and the result is bitwise reproducible; a ray's
 * columns do not depend on the rays traced with it.  BHN_EINVAL before any launch: null alpha / beta / end / status, n < 1, ngeo < 0,
 * ngeo > 0 with samples NULL, h <= 0, r_c <= 0, max_steps < 1, M <= 0, |spin| > 1, inclination outside (0, pi/2 + 1e-12]. */
BHN_API int bhn_kerr_trace(const double *alpha, const double *beta, int64_t n, double spin, double inclination, double distance,
                   double M, double h, double r_c, int32_t max_steps, int32_t ngeo, double *samples, double *end,
                   int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_KERR_H */
