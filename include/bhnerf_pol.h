/*
 * bhnerf_pol.h -- C ABI of libbhnerf_pol.so: the polarimetric EHT losses from the baselines' (u, v) coordinates, on the MI355X
 * (gfx950): the polarised visibility P = Q + iU ('pvis', the calibrated term) and the visibility-domain fractional polarisation
 * m = P / I ('m', free of every complex station gain common to the Stokes planes of a baseline), with the image gradient.
 *
 * A library of its own, beside libbhnerf_eht.so and libbhnerf_cls.so: their ABIs stay exactly what they are.  The conventions are
 * those of include/bhnerf_cls.h: 0 on success or a BHN_E* code (the last-error call of this header gives a thread-local message;
 * nothing aborts, nothing prints); the CALLER owns every buffer, what an output or the workspace holds on entry is irrelevant,
 * every element of an output is written and nothing outside the sizes named here is; no allocation, no synchronisation, no
 * environment reads, no state but the error string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the
 * calling thread's current device and can be captured into a graph.
 *
 * The operator is that of include/bhnerf_eht.h: planes, frames, uv, pixel centres and V[n, k] as defined there, computed by the
 * same kernels in the same order -- V is bitwise what the forward-only call of that header returns.
 *
 * The loss.  Sx is 3 or 4: the planes of frame b are I, Q, U[, V] = planes b Sx + 0, 1, 2[, 3].  With V_s = V[b Sx + s, k] and
 * P = V_1 + i V_2, scale (w_pvis chi^2_pvis + w_m chi^2_m) over the terms that are present:
 *   pvis   |P - target|^2 / sigma^2 per (frame, baseline)
 *   m      |P / V_0 - target|^2 / sigma^2 per (frame, baseline); a baseline with V_0 == 0 contributes 0 to the loss and nothing
 *          to the gradient
 * target (B, nvis) complex64 as interleaved float pairs and sigma (B, nvis) float32, B = N / Sx.  An entry with sigma = +inf
 * gives exactly 0 loss and gradient whatever finite target stands there.  The effective scale of a term is scale * weight, the
 * product formed once in float64 on the host and rounded once to float32.  Every sum has one fixed order, there are no atomics:
 * the result is bitwise reproducible and a frame's terms and gradient do not depend on the frames computed with it.
 */
#ifndef BHNERF_POL_H
#define BHNERF_POL_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP / BHN_EWORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

/* One data term, a HOST struct: target and sigma are DEVICE pointers, target to (B, nvis) float pairs, sigma to (B, nvis) float32. */
typedef struct bhn_pol_term {
    const float *target;
    const float *sigma;
    double weight;             /* w_d >= 0, finite */
} bhn_pol_term;

BHN_API const char *bhn_pol_last_error(void);

/* Bytes of workspace a call with these sizes needs; 0 when a size is below 1 or too large for one call.  The workspace must be
 * 8-byte aligned. */
BHN_API size_t bhn_pol_ws_bytes(int32_t N, int32_t nvis, int32_t H, int32_t W);

/* loss[3] = {total, pvis, m} (device), each term the frames' sums added in order, an absent term 0, total = pvis + m; unless
 * dimages is NULL, dimages (N, H, W) = d total / d images, plane 3 of a frame, when present, written with zeros.  pvis / m: NULL
 * for an absent term.  ws: bhn_pol_ws_bytes(N, nvis, H, W) bytes.  With dimages NULL nothing of the backward pass is launched.
 * BHN_EINVAL before any launch: no term present; a present term with a NULL target or sigma or a weight that is negative or not
 * finite; Sx other than 3 or 4; a null images / uv / loss / ws, a size below 1, N not a multiple of Sx, a pixel size that is not
 * positive and finite, a misaligned ws / uv.  BHN_EWORKSPACE before any launch: ws_bytes too small. */
BHN_API int bhn_pol_chi2(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                 double psize_x, double psize_y, const bhn_pol_term *pvis, const bhn_pol_term *m, float scale, float *loss,
                 float *dimages, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_POL_H */
