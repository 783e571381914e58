/*
 * bhnerf_eql.h -- C ABI of libbhnerf_eql.so: where image-plane Kerr rays meet the equatorial plane, the primitive behind
 * emission.equatorial_ring (emission.py:119-141) and kgeo.equatorial_lensing (r_equatorial, rho_of_req; the reference takes both from
 * closed forms of the external kgeo package) on the MI355X (gfx950).
 *
 * A library of its own, beside libbhnerf_hip.so and the other side libraries: a float64 pre-compute, not a piece of the training
 * step.  The conventions are those of include/bhnerf_hip.h: 0 on success or a BHN_E* code (bhn_eql_last_error() gives a thread-local
 * message; nothing aborts, nothing prints); the CALLER owns every buffer, what an output holds on entry is irrelevant and every
 * element of it is written, nothing outside the array shapes named here is; no allocation, no synchronisation, no environment reads,
 * no state but the error string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the calling thread's current
 * device.
 */
#ifndef BHNERF_EQL_H
#define BHNERF_EQL_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP */

#ifdef __cplusplus
extern "C" {
#endif

BHN_API const char *bhn_eql_last_error(void);

/* bhnerf_amd/geodesics.py `_integrate_crossings` restated on the device, one lane per ray (csrc/equatorial.h holds the per-ray code;
 * it also compiles for the CPU).  Ray i is the image-plane tracer's: it starts at r = distance, theta = inclination with
 * lam = -alpha[i] sin(inclination), eta = (alpha[i]^2 - a^2) cos^2(inclination) + beta[i]^2 (a = spin M) and is followed backwards in
 * Mino time by classical RK4 with the step h (1 + r/r_c) / r^2 * clip((sin theta / 0.25)^2, 0.05, 1) until a step would end at
 * !(r > 1.02 r_hor) (captured; that step is not taken) or r > distance with v_r > 0 (escaped), in one pass.  A taken step with
 * theta - pi/2 of opposite sign at its two ends, or with its new end exactly on pi/2, holds one crossing, at the root w in (0, 1] of
 * the cubic Hermite interpolant of theta over the step (64 bisections, always all of them); column j of `cross` is the Hermite
 * combination of the step's ends at the w of the ray's (j+1)-th crossing.  A lane stops at the ray's end, after its nmax-th
 * crossing, or after max_steps steps.  All float64, device memory:
 *   alpha, beta (n);  cross (7, n, nmax), rows mino, r, theta, phi, t, v_r, v_theta: columns count[i]..nmax-1 of ray i are NaN;
 *   count (n) int32: crossings found, 0..nmax;  status (n) int32: steps taken, or -1 when the ray was neither finished nor at its
 *   nmax-th crossing after max_steps (non-termination is data; count and cross then hold what was found).
 * mino is the Mino time elapsed since the observer (positive); phi and t are those of the forward equations: the caller negates them.
 * Every element of cross, count and status is written.  Rays are independent and the result is bitwise reproducible; a ray's
 * columns do not depend on the rays traced with it.  BHN_EINVAL before any launch: null alpha / beta / cross / count / status, n < 1,
 * nmax < 1, h <= 0, r_c <= 0, max_steps < 1, M <= 0, |spin| > 1, inclination outside (0, pi/2 + 1e-12] or within 1e-6 of pi/2 (the
 * observer sits in the plane). */
BHN_API int bhn_eql_crossings(const double *alpha, const double *beta, int64_t n, double spin, double inclination, double distance,
                   double M, double h, double r_c, int32_t max_steps, int32_t nmax, double *cross, int32_t *count,
                   int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_EQL_H */
