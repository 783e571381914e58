/*
 * bhnerf_grf.h -- C ABI of libbhnerf_grf.so: the Doppler factor g, the fluid-frame magnetic field b and the polarised transport
 * factors J of bhnerf_amd/kgeo.py (azimuthal_velocity_vector, doppler_factor, magnetic_field_fluid_frame, parallel_transport;
 * reference kgeo.py:92-519) on the MI355X (gfx950): what alma.image_plane_model computes after the geodesics are traced.
 *
 * A library of its own, beside libbhnerf_hip.so, libbhnerf_kerr.so and libbhnerf_eht.so: their ABIs stay exactly what they are.
 * The conventions are those of include/bhnerf_hip.h: 0 on success or a BHN_E* code (bhn_grf_last_error() gives a thread-local
 * message; nothing aborts, nothing prints); the CALLER owns every buffer, what an output or the workspace holds on entry is
 * irrelevant, every element of an output is written and nothing outside the sizes named here is; no allocation, no
 * synchronisation, no environment reads, no state but the error string; all work is enqueued on `stream` (a hipStream_t passed as
 * void*) of the calling thread's current device.
 *
 * All arrays are FLOAT64 in device memory.  The arithmetic is kgeo.py's, expression for expression (csrc/gr_factors.h holds it; it
 * also compiles for the CPU), one lane per sample point: a point's outputs depend on its own ray only (the k -+ 1 neighbours along
 * the ray for the signs of the wave vector), so a ray's results do not depend on the rays computed with it and every result is
 * bitwise reproducible.  Nothing is clamped: NaN and inf are written where NumPy produces them (a superluminal Omega, 0 / 0 in
 * the gradient quotient); nan_to_num stays with the caller.  The 4-velocity is the azimuthal one, given as Omega per point.
 */
#ifndef BHNERF_GRF_H
#define BHNERF_GRF_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP / BHN_EWORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

/* The fields kgeo.py reads from the geodesic record: n rays of ngeo samples.  Per point (n, ngeo) row-major: r, theta, affine,
 * Delta, Sigma, Xi, R, Theta;  per ray (n): lam, alpha, beta;  scalars: spin (kgeo.py's `a`), M, E, inc (radians). */
typedef struct bhn_grf_geos {
    int64_t n;
    int32_t ngeo;
    const double *r, *theta, *affine, *Delta, *Sigma, *Xi, *R, *Theta;
    const double *lam, *alpha, *beta;
    double spin, M, E, inc;
} bhn_grf_geos;

BHN_API const char *bhn_grf_last_error(void);

/* Bytes of workspace bhn_grf_domain_mean needs for n rays of ngeo samples (the partial sums and counts of its first stage);
 * 0 when n < 1, ngeo < 2 or the sizes are too large for one call.  The workspace must be 8-byte aligned. */
BHN_API size_t bhn_grf_ws_bytes(int64_t n, int32_t ngeo);

/* Every call below returns BHN_EINVAL before any launch for: a null geos or a null field in it, n < 1, ngeo < 2 (np.gradient
 * needs two samples), n * ngeo too large for one launch, a null Omega (n, ngeo) or a null input / output array. */

/* doppler_factor(geos, azimuthal_velocity_vector(geos, Omega), fillna): g (n, ngeo).  A NaN becomes `fillna` when fill != 0 and
 * stays a NaN when fill == 0 (kgeo's fillna=False / None). */
BHN_API int bhn_grf_doppler(const bhn_grf_geos *geos, const double *Omega, double fillna, int32_t fill, double *g, void *stream);

/* magnetic_field_fluid_frame(geos, azimuthal_velocity_vector(geos, Omega), arad, avert, ator): b (n, ngeo, 3). */
BHN_API int bhn_grf_fluid_field(const bhn_grf_geos *geos, const double *Omega, double arad, double avert, double ator, double *b,
                        void *stream);

/* mean[0] = the mean of |b| over the points with |r cos(theta)| < z_width, r > rmin and r < rmax (the recovery domain of
 * alma.image_plane_model); b (n, ngeo, 3), mean one float64 on the device.  A two-stage reduction in one fixed order, partial
 * sums in ws, no atomics.  A NaN among the selected points makes the mean NaN, no selected point makes it NaN (0 / 0), as
 * ndarray.mean() does.  ws: bhn_grf_ws_bytes(n, ngeo) bytes; BHN_EINVAL for a null or misaligned ws, BHN_EWORKSPACE when
 * ws_bytes is too small, both before any launch. */
BHN_API int bhn_grf_domain_mean(const bhn_grf_geos *geos, const double *b, double z_width, double rmin, double rmax, double *mean,
                        void *ws, size_t ws_bytes, void *stream);

/* parallel_transport(geos, azimuthal_velocity_vector(geos, Omega), g, b / divisor[0], Q_frac, V_frac, spectral_index):
 * J (S, n, ngeo), rows I, Q, U and, when V_frac != 0, V (S = 4, else S = 3).  g (n, ngeo) and b (n, ngeo, 3) are read as given;
 * divisor is one float64 on the device (bhn_grf_domain_mean's output) or NULL for no division.  BHN_EINVAL also for Q_frac
 * outside [0, 1]. */
BHN_API int bhn_grf_transport(const bhn_grf_geos *geos, const double *Omega, const double *g, const double *b, const double *divisor,
                      double Q_frac, double V_frac, double spectral_index, double *J, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_GRF_H */
