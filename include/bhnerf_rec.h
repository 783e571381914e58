/*
 * bhnerf_rec.h -- C ABI of libbhnerf_rec.so: the geodesic record of bhnerf_amd/geodesics.py (`_build_record`) from the samples of the
 * ray tracer, and the Keplerian angular velocity of alma.image_plane_model, on the MI355X (gfx950).  With it a record is created in
 * device memory, where bhn_kerr_trace left its samples, and the (g, J) libraries read it there: geodesics.DeviceGeodesics.
 *
 * A library of its own, the seventh: the ABIs of the other six stay exactly what they are.  The conventions are those of
 * include/bhnerf_hip.h: 0 on success or a BHN_E* code (the last-error call below gives a thread-local message; nothing aborts, nothing
 * prints); the CALLER owns every buffer, what an output holds on entry is irrelevant, every element of an output is written and
 * nothing outside the sizes named here is; no allocation, no synchronisation, no environment reads, no state but the error string;
 * all work is enqueued on `stream` (a hipStream_t passed as void*) of the calling thread's current device.
 *
 * All arrays are FLOAT64 in device memory.  The arithmetic is geodesics.py's, expression for expression (csrc/geo_record.h; it also
 * compiles for the CPU), with floating-point contraction off: r, theta, phi, t, mino, vr, vth and dtau carry the bits of the samples
 * (copies and sign flips), the other fields differ from NumPy's by the device's sin / cos / tan / pow only.  A ray's outputs depend on
 * its own samples only, so they do not depend on the rays built with it and every result is bitwise reproducible.  Nothing is
 * clamped: NaN and inf are written where NumPy produces them.
 */
#ifndef BHNERF_REC_H
#define BHNERF_REC_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP */

#ifdef __cplusplus
extern "C" {
#endif

/* The 18 per-point fields of the record, each (n, ngeo) row-major. */
typedef struct bhn_rec_fields {
    double *r, *theta, *phi, *t, *mino, *Delta, *Sigma, *Xi, *omega, *x, *y, *z, *R, *Theta, *vr, *vth, *dtau, *affine;
} bhn_rec_fields;

BHN_API const char *bhn_rec_last_error(void);

/* _build_record on n rays of ngeo samples.  samples (7, n, ngeo): the output of bhn_kerr_trace, rows mino, r, theta, phi, t, v_r,
 * v_theta of the forward equations;  lam, eta (n): the rays' constants of motion;  spin, M: those of the trace.  Written, per point:
 * r, theta, v_r, v_theta as sampled;  phi, t, mino negated (the rays were followed backwards);  Delta, Sigma, Xi, omega
 * (kerr_functions);  x, y, z;  R, Theta (radial_potential, angular_potential with a = spin M);  dtau[i, k] = the Mino sample
 * samples[0, i, 0] of the ray;  affine = -cumsum(Sigma dtau) along the ray in np.cumsum's order (sample 0 first, one product and one
 * add per sample, no fused multiply-add), so that its differences round as NumPy's do.  A chunk of rays is a contiguous slab of
 * every output: a caller that traces `chunk` rays at a time passes the fields' pointers offset by first_ray * ngeo.
 * BHN_EINVAL before any launch for: a null samples, lam, eta, out or field of out, n < 1, ngeo < 1, n * ngeo too large for one
 * launch. */
BHN_API int bhn_rec_build(const double *samples, const double *lam, const double *eta, int64_t n, int32_t ngeo, double spin, double M,
                  const bhn_rec_fields *out, void *stream);

/* Omega[p] = (factor sqrt(M)) / (pow(r[p], 1.5) + spin sqrt(M)) for p < count: the Keplerian angular velocity of
 * alma.image_plane_model in its order of evaluation (factor = Omega_frac times +-1 for the sense of rotation).  r = 0 gives what
 * NumPy gives (factor / spin, or the inf / NaN of a division by zero).  BHN_EINVAL before any launch for: a null r or Omega,
 * count < 1, count too large for one launch. */
BHN_API int bhn_rec_kepler(const double *r, int64_t count, double spin, double M, double factor, double *Omega, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_REC_H */
