/*
 * bhnerf_eht.h -- C ABI of libbhnerf_eht.so: the EHT visibility-domain chi-square of loss_fn_eht (network.py:541-564) computed
 * from the (u, v) coordinates of the baselines on the MI355X (gfx950), without the dense DFT matrices bhn_chi2_eht takes.
 *
 * A library of its own, beside libbhnerf_hip.so and libbhnerf_kerr.so: the ABI of include/bhnerf_hip.h (version 5, 33 entry
 * points) stays exactly what it is.  The conventions are that header's: 0 on success or a BHN_E* code (bhn_eht_last_error() gives
 * a thread-local message; nothing aborts, nothing prints); the CALLER owns every buffer, what an output or the workspace holds on
 * entry is irrelevant, every element of an output is written and nothing outside the sizes named here is; no allocation, no
 * synchronisation, no environment reads, no state but the error string; all work is enqueued on `stream` (a hipStream_t passed
 * as void*) of the calling thread's current device and can be captured into a graph.
 *
 * The operator.  Plane n (of N = B Sx planes, H x W float32 pixels each, row-major) belongs to frame n / Sx; frame b observes with
 * the baselines uv[b] = (u, v)_k, k < nvis, in wavelengths, FLOAT64 on the device.  Pixel (y, x) sits at the angles
 * ((x - (W - 1) / 2) psize_x, (y - (H - 1) / 2) psize_y) radians -- observation.dft_matrix's pixel centres -- and
 *     V[n, k] = sum_{y, x} I[n, y, x] exp(-2 pi i (u_k x_x + v_k y_y)).
 * The exponential is separable: each call builds the tables Eu (B, nvis, W) and Ev (B, nvis, H) in the workspace (float64 phase,
 * reduced to turns, rounded to complex64) and computes V = sum_x Eu sum_y I Ev and the adjoint from them (csrc/eht_uv.hip).
 * Every sum has one fixed order: visibilities, loss and gradient are bitwise reproducible, and a plane's visibilities and
 * gradient do not depend on the planes computed with it.
 */
#ifndef BHNERF_EHT_H
#define BHNERF_EHT_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP / BHN_EWORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

BHN_API const char *bhn_eht_last_error(void);

/* Bytes of workspace a call with these sizes needs (ncp = 0 for bhn_eht_vis and for 'vis' / 'amp' without a table); 0 when a
 * size is below 1 (ncp below 0) or too large for one call.  The workspace must be 8-byte aligned. */
BHN_API size_t bhn_eht_ws_bytes(int32_t N, int32_t nvis, int32_t ncp, int32_t H, int32_t W);

/* Forward only: vis_out (N, nvis) interleaved complex64 (8-byte aligned).  ws: bhn_eht_ws_bytes(N, nvis, 0, H, W) bytes.
 * BHN_EINVAL before any launch: a null pointer, a size below 1, N not a multiple of Sx, a pixel size that is not positive and
 * finite, a misaligned ws / uv / vis_out;  BHN_EWORKSPACE before any launch: ws_bytes too small. */
BHN_API int bhn_eht_vis(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                double psize_x, double psize_y, float *vis_out, void *ws, size_t ws_bytes, void *stream);

/* loss[0] = scale * chi^2 and, unless dimages is NULL, dimages (N, H, W) = d loss / d images.  dtype: 0 'vis' (target (N, nvis)
 * interleaved complex64), 1 'amp' (target (N, nvis) float32), 2 'cphase' (target (N, ncp) float32 radians); sigma float32 in the
 * target's shape -- the layouts of bhn_chi2_eht, and its arithmetic term for term, the zero gradient at |vis| = 0 included.
 * 'cphase' takes each baseline's visibility ONCE and a triangle table shared by all frames, on the device: tri (ncp, 3) int32
 * baseline indices in [0, nvis), tri_sign (ncp, 3) int8, +1 the visibility as stored, -1 its conjugate;
 * phi = sum_legs sign atan2(Im V, Re V), term (1 - cos(target - phi)) / sigma^2.  The gradient of a baseline that sits in several
 * triangles is gathered in table order.  For 'vis' and 'amp' the table is not read (ncp counts only towards the workspace).
 * ws: bhn_eht_ws_bytes(N, nvis, ncp, H, W) bytes.  With dimages NULL nothing of the backward pass is launched.
 * BHN_EINVAL / BHN_EWORKSPACE before any launch: as bhn_eht_vis, and a dtype outside 0..2, ncp > 0 with a NULL table, 'cphase'
 * with ncp < 1. */
BHN_API int bhn_eht_chi2_uv(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                    double psize_x, double psize_y, int32_t dtype, const float *target, const float *sigma, float scale,
                    const int32_t *tri, const int8_t *tri_sign, int32_t ncp, float *loss, float *dimages, void *ws,
                    size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_EHT_H */
