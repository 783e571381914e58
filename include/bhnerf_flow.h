/*
 * bhnerf_flow.h -- C ABI of libbhnerf_flow.so: the Doppler factor g, the fluid-frame magnetic field b and the polarised transport
 * factors J of bhnerf_amd/kgeo.py for a GENERAL 4-velocity on the MI355X (gfx950): a umu array handed in per sample point, or the
 * boosted ZAMO of Gelles et al. 2021 (zamo_frame_velocity, zamo_frame_tetrad, doppler_factor, magnetic_field_fluid_frame,
 * parallel_transport, parallel_transport_zamo), what the polarised-ring study computes for every (beta, chi, field) setting.
 *
 * A library of its own, the sixth: the ABIs of the other five stay exactly what they are (the azimuthal 4-velocity, given as
 * Omega per point, is the (g, J) library's).  The conventions are those of include/bhnerf_hip.h: 0 on success or a BHN_E* code (the
 * last-error call below gives a thread-local message; nothing aborts, nothing prints); the CALLER owns every buffer, what an
 * output holds on entry is irrelevant, every element of an output is written and nothing outside the sizes named here is; no
 * allocation, no synchronisation, no environment reads, no state but the error string; all work is enqueued on `stream` (a
 * hipStream_t passed as void*) of the calling thread's current device.
 *
 * All arrays are FLOAT64 in device memory.  The arithmetic is kgeo.py's, expression for expression (csrc/flow_factors.h on
 * csrc/gr_factors.h; both also compile for the CPU), one lane per sample point: a point's outputs depend on its own ray only (the
 * k -+ 1 neighbours along the ray for the signs of the wave vector), so a ray's results do not depend on the rays computed with it
 * and every result is bitwise reproducible.  Nothing is clamped and beta, chi are not validated: NaN and inf are written where
 * NumPy produces them (beta >= 1, a spacelike umu, 0 / 0 in the gradient quotient); nan_to_num stays with the caller.
 *
 * A umu array is (n, ngeo, 4), contravariant components (t, r, theta, phi) last, as the Python functions return it.  The mean of
 * |b| over the recovery domain is the (g, J) library's reduction, called on the same device buffers.
 */
#ifndef BHNERF_FLOW_H
#define BHNERF_FLOW_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP */

#ifdef __cplusplus
extern "C" {
#endif

/* The fields kgeo.py reads from the geodesic record: n rays of ngeo samples.  Per point (n, ngeo) row-major: r, theta, affine,
 * Delta, Sigma, Xi, R, Theta;  per ray (n): lam, alpha, beta;  scalars: spin (kgeo.py's `a`), M, E, inc (radians);  and omega
 * (n, ngeo), the record's frame-dragging frequency, which the ZAMO functions read. */
typedef struct bhn_flow_geos {
    int64_t n;
    int32_t ngeo;
    const double *r, *theta, *affine, *Delta, *Sigma, *Xi, *R, *Theta;
    const double *lam, *alpha, *beta;
    double spin, M, E, inc;
    const double *omega;
} bhn_flow_geos;

BHN_API const char *bhn_flow_last_error(void);

/* Every call below returns BHN_EINVAL before any launch for: a null geos or a null field in it (omega included), n < 1, ngeo < 2
 * (np.gradient needs two samples), n * ngeo too large for one launch, or a null input / output array. */

/* zamo_frame_velocity(geos, beta, chi): umu (n, ngeo, 4). */
BHN_API int bhn_flow_zamo_velocity(const bhn_flow_geos *geos, double beta, double chi, double *umu, void *stream);

/* doppler_factor(geos, umu, fillna): g (n, ngeo).  A NaN becomes `fillna` when fill != 0 and stays a NaN when fill == 0. */
BHN_API int bhn_flow_doppler(const bhn_flow_geos *geos, const double *umu, double fillna, int32_t fill, double *g, void *stream);

/* magnetic_field_fluid_frame(geos, umu, arad, avert, ator): b (n, ngeo, 3). */
BHN_API int bhn_flow_fluid_field(const bhn_flow_geos *geos, const double *umu, double arad, double avert, double ator, double *b,
                         void *stream);

/* parallel_transport(geos, umu, g, b / divisor[0], Q_frac, V_frac, spectral_index) in the fluid tetrad of umu: J (S, n, ngeo),
 * rows I, Q, U and, when V_frac != 0, V (S = 4, else S = 3).  g (n, ngeo) and b (n, ngeo, 3) are read as given; divisor is one
 * float64 on the device or NULL for no division.  BHN_EINVAL also for Q_frac outside [0, 1]. */
BHN_API int bhn_flow_transport(const bhn_flow_geos *geos, const double *umu, const double *g, const double *b, const double *divisor,
                       double Q_frac, double V_frac, double spectral_index, double *J, void *stream);

/* parallel_transport_zamo(geos, beta, chi, g, b / divisor[0], Q_frac, spectral_index) in the boosted ZAMO tetrad:
 * J (3, n, ngeo), rows I, Q, U.  BHN_EINVAL also for Q_frac outside [0, 1]. */
BHN_API int bhn_flow_transport_zamo(const bhn_flow_geos *geos, double beta, double chi, const double *g, const double *b,
                            const double *divisor, double Q_frac, double spectral_index, double *J, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_FLOW_H */
