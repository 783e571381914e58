// libbhnerf_pol.so (include/bhnerf_pol.h): the polarimetric EHT losses 'pvis' (P = Q + iU) and 'm' (P / I, free of station gains
// common to the Stokes planes) with their image gradient, from ONE visibility pass over the baselines' (u, v) coordinates.
//
// csrc/eht_pol.h holds the plan and the arithmetic of the terms, shared with the CPU build of tools/eht_pol_host.cpp;
// csrc/eht_uv_kernels.h holds the kernels shared with libbhnerf_eht.so.  The launches of a call, all on the caller's stream:
//   eht_twiddle_kernel, eht_fwd_kernel   as in csrc/eht_uv.hip (eht_forward): the partial sums of every visibility
//   pol_loss_kernel      one workgroup per FRAME, lanes strided over the baselines: a lane combines the row splits' partial sums
//                        of the Sx planes of its baseline in order (kept in the workspace), computes both terms and leaves gv of
//                        all Sx planes; two block sums per frame
//   eht_terms_sum_kernel the frames' sums of each term in order, and their total (csrc/eht_terms.h, as are the terms of a call)
//   eht_adjoint_kernel   as in csrc/eht_uv.hip (eht_launch_adjoint)
// The terms are per baseline: no gather stage.  No atomics, no allocation, no synchronisation: every sum has one fixed order that
// does not depend on how many frames a call holds.  With dimages NULL the adjoint is not launched and gv is not written.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_pol.h"
#include "eht_pol.h"
#include "eht_terms.h"
#include "eht_uv_kernels.h"
#include "side_lib.h"

extern "C" const char *bhn_pol_last_error(void) { return side_last_error(); }

typedef EhtTerms<POL_TERMS> PolTerms;

// A lane adds its baselines in order, the workgroup adds the lanes in a fixed order (eht_block_sum_256): terms[d, b] does not
// depend on the frames computed with it.  Every index is below N nvis (planes b Sx + s < N, k < nvis) or B nvis (b < B).
__global__ __launch_bounds__(256) void pol_loss_kernel(const EhtC *__restrict__ part, PolPlan p, int Sx, PolTerms a, EhtC *__restrict__ vis,
                                                       EhtC *__restrict__ gv, float *__restrict__ terms, int want_grad) {
    __shared__ float red[POL_TERMS][4];
    const int b = blockIdx.x, nvis = p.e.nvis, n0 = b * Sx;
    float term[POL_TERMS] = {0.f, 0.f};
    for (int k = threadIdx.x; k < nvis; k += 256) {
        EhtC v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < Sx) {
                v[s] = eht_combine(p.e, part, n0 + s, k);
                vis[(size_t)(n0 + s) * nvis + k] = v[s];
            }
        const size_t t = (size_t)b * nvis + k;
        const bool has_p = a.present[POL_PVIS] != 0, has_m = a.present[POL_M] != 0;
        float tp, tm;
        EhtC g[3];
        pol_baseline(v[0], v[1], v[2], has_p, has_p ? a.target[POL_PVIS] + 2 * t : nullptr, has_p ? a.sigma[POL_PVIS][t] : 1.f,
                     a.scale[POL_PVIS], has_m, has_m ? a.target[POL_M] + 2 * t : nullptr, has_m ? a.sigma[POL_M][t] : 1.f, a.scale[POL_M],
                     &tp, &tm, g);
        term[POL_PVIS] += tp;
        term[POL_M] += tm;
        if (want_grad) {
#pragma unroll
            for (int s = 0; s < 3; ++s) gv[(size_t)(n0 + s) * nvis + k] = g[s];
            if (Sx == 4) {
                const EhtC zero = {0.f, 0.f};
                gv[(size_t)(n0 + 3) * nvis + k] = zero;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < POL_TERMS; ++d) {
        const float tot = eht_block_sum_256(term[d], red[d]);
        if (threadIdx.x == 0) terms[(size_t)d * p.e.N + b] = a.scale[d] * tot;
    }
}

extern "C" size_t bhn_pol_ws_bytes(int32_t N, int32_t nvis, int32_t H, int32_t W) {
    PolPlan p;
    return pol_make_plan(N, nvis, H, W, &p) ? p.bytes : 0;
}

extern "C" int bhn_pol_chi2(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                            double psize_x, double psize_y, const bhn_pol_term *pvis, const bhn_pol_term *m, float scale, float *loss,
                            float *dimages, void *ws, size_t ws_bytes, void *stream) {
    PolPlan p;
    PolTerms a;
    const bhn_pol_term *const in[POL_TERMS] = {pvis, m};
    static const char *const names[POL_TERMS] = {"pvis", "m"};
    BHN_CHECK_ARG(images && uv && ws && loss, "null pointer");
    BHN_CHECK_ARG(pvis || m, "no term present");
    if (int rc = eht_terms_take(in, names, scale, &a)) return rc;
    BHN_CHECK_ARG(pol_stokes_ok(Sx), "the polarimetric terms need the planes I, Q, U[, V]: Sx must be 3 or 4 (Sx = %d)", Sx);
    const char *why = eht_sizes_error(N, Sx, nvis, 0, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(!why, "%s (N %d, Sx %d, nvis %d, H %d, W %d, pixel %g x %g rad)", why, N, Sx, nvis, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(pol_make_plan(N, nvis, H, W, &p), "sizes too large for one call (N %d, nvis %d, H %d, W %d)", N, nvis, H, W);
    BHN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(uv) & 7) == 0, "ws and uv must be 8-byte aligned");
    if (ws_bytes < p.bytes)
        return side_fail(BHN_EWORKSPACE, "workspace of %zu bytes, bhn_pol_ws_bytes(%d, %d, %d, %d) = %zu", ws_bytes, N, nvis, H, W, p.bytes);

    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    EhtC *vis = reinterpret_cast<EhtC *>(w + p.e.off_vis), *gv = reinterpret_cast<EhtC *>(w + p.off_gv);
    float *terms = reinterpret_cast<float *>(w + p.off_terms);
    const int B = N / Sx;
    const int rf = eht_forward(images, uv, p.e, Sx, psize_x, psize_y, w, nullptr, st);
    if (rf != BHN_OK) return rf;
    hipLaunchKernelGGL(pol_loss_kernel, dim3((unsigned)B), dim3(256), 0, st, reinterpret_cast<const EhtC *>(w + p.e.off_part), p, (int)Sx, a, vis,
                       gv, terms, dimages ? 1 : 0);
    if (int rc = side_launched("pol_loss_kernel")) return rc;
    hipLaunchKernelGGL(eht_terms_sum_kernel<POL_TERMS>, dim3(1), dim3(256), 0, st, loss, terms, (int)N, B);
    if (int rc = side_launched("eht_terms_sum_kernel")) return rc;
    if (!dimages) return BHN_OK;
    return eht_launch_adjoint(gv, w, p.e, Sx, dimages, st);
}
