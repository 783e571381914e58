/*
 * bhnerf_cls.h -- C ABI of libbhnerf_cls.so: EHT log closure amplitudes and ONE weighted sum of real-valued data terms
 * ('amp', 'cphase', 'logcamp') from one visibility pass over the baselines' (u, v) coordinates, on the MI355X (gfx950).
 *
 * A library of its own, beside libbhnerf_eht.so: the ABI of include/bhnerf_eht.h stays exactly what it is.  The conventions are
 * that header's: 0 on success or a BHN_E* code (the last-error call of this header gives a thread-local message; nothing aborts,
 * nothing prints); the CALLER owns every buffer, what an output or the workspace holds on entry is irrelevant, every element of
 * an output is written and nothing outside the sizes named here is; no allocation, no synchronisation, no environment reads, no
 * state but the error string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the calling thread's current
 * device and can be captured into a graph.
 *
 * The operator is that of include/bhnerf_eht.h: planes, frames, uv, pixel centres and V[n, k] as defined there, computed by the
 * same kernels in the same order -- V is bitwise what the forward-only call of that header returns.
 *
 * The loss.  scale (w_amp chi^2_amp + w_cphase chi^2_cphase + w_logcamp chi^2_logcamp) over the terms that are present:
 *   amp      ((|V_k| - target) / sigma)^2 per baseline, target / sigma (N, nvis) float32
 *   cphase   (1 - cos(target - phi)) / sigma^2 per triangle, phi = sum_legs sign atan2(Im V, Re V) through tri (ncp, 3) int32 and
 *            tri_sign (ncp, 3) int8 as in include/bhnerf_eht.h; target / sigma (N, ncp) float32, radians
 *   logcamp  ((y - target) / sigma)^2 per quadrangle, y = 1/2 (log m_0 + log m_1 - log m_2 - log m_3) with m_l = |V|^2 of leg l
 *            of quad (nca, 4) int32 baseline indices: legs 0, 1 the numerator, legs 2, 3 the denominator (no signs:
 *            |V_ab| = |V_ba|); target / sigma (N, nca) float32.  A quadrangle with a leg of zero amplitude contributes 0 to
 *            the loss and nothing to the gradient.
 * 'amp' and 'cphase' are the arithmetic of include/bhnerf_eht.h term for term at the effective scale scale * weight (the product
 * formed once in float64 on the host and rounded once to float32): alone and at weight 1, loss and dimages are bitwise that
 * header's.  Table indices outside [0, nvis) are the caller's error; they are clamped and cannot read outside a plane.
 * Every sum has one fixed order, there are no atomics: the result is bitwise reproducible and a plane's terms and gradient do
 * not depend on the planes computed with it.
 */
#ifndef BHNERF_CLS_H
#define BHNERF_CLS_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP / BHN_EWORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

/* One data term, a HOST struct: target and sigma are DEVICE pointers to float32 arrays of the term's shape. */
typedef struct bhn_cls_term {
    const float *target;
    const float *sigma;
    double weight;             /* w_d >= 0, finite */
} bhn_cls_term;

BHN_API const char *bhn_cls_last_error(void);

/* Bytes of workspace a call with these sizes needs (ncp / nca = 0 without that table); 0 when a size is below 1 (ncp, nca below
 * 0) or too large for one call.  The workspace must be 8-byte aligned. */
BHN_API size_t bhn_cls_ws_bytes(int32_t N, int32_t nvis, int32_t ncp, int32_t nca, int32_t H, int32_t W);

/* loss[4] = {total, amp, cphase, logcamp} (device), each term the planes' sums added in order, an absent term 0,
 * total = amp + cphase + logcamp added in that order; unless dimages is NULL, dimages (N, H, W) = d total / d images, from
 * gv_k = gv_amp + gv_cphase + gv_logcamp added in that order.  amp / cphase / logcamp: NULL for an absent term.
 * ws: bhn_cls_ws_bytes(N, nvis, ncp, nca, H, W) bytes.  With dimages NULL nothing of the backward pass is launched.
 * BHN_EINVAL before any launch: no term present; a present term with a NULL target or sigma or a weight that is negative or not
 * finite; cphase present with ncp < 1 or a NULL table; logcamp present with nca < 1 or a NULL table; a null images / uv / loss /
 * ws, a size below 1 (ncp, nca below 0), N not a multiple of Sx, a pixel size that is not positive and finite, a misaligned
 * ws / uv.  BHN_EWORKSPACE before any launch: ws_bytes too small. */
BHN_API int bhn_cls_chi2(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                 double psize_x, double psize_y, const bhn_cls_term *amp, const bhn_cls_term *cphase,
                 const bhn_cls_term *logcamp, const int32_t *tri, const int8_t *tri_sign, int32_t ncp, const int32_t *quad,
                 int32_t nca, float scale, float *loss, float *dimages, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_CLS_H */
