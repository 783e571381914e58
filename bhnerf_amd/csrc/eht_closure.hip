// libbhnerf_cls.so (include/bhnerf_cls.h): EHT log closure amplitudes and one weighted sum of the real-valued data terms
// 'amp' | 'cphase' | 'logcamp' with its image gradient, from ONE visibility pass over the baselines' (u, v) coordinates.
//
// csrc/eht_closure.h holds the plan and the arithmetic of the new term, shared with the CPU build of tools/eht_closure_host.cpp;
// csrc/eht_uv_kernels.h holds the kernels shared with libbhnerf_eht.so.  The launches of a call, all on the caller's stream:
//   eht_twiddle_kernel, eht_fwd_kernel   as in csrc/eht_uv.hip (eht_forward): the partial sums of every visibility
//   cls_loss_kernel      one workgroup per plane: a visibility = its row splits' partial sums in order, KEPT in the workspace;
//                        'amp' one lane per visibility, its gv into a buffer of its own; then one lane per triangle leaves
//                        dL/dphi and one lane per quadrangle dL/dy, in lane-stride loops; three block sums per plane
//   eht_terms_sum_kernel the planes' sums of each term in order, and their total (csrc/eht_terms.h, as are the terms of a call)
//   cls_gather_kernel    one wave per (plane, baseline): the triangle and the quadrangle table scanned in 64-lane slices with a
//                        butterfly sum each; gv = gv_amp + gv_cphase + gv_logcamp
//   eht_adjoint_kernel   as in csrc/eht_uv.hip (eht_launch_adjoint)
// No atomics, no allocation, no synchronisation: every sum has one fixed order that does not depend on how many frames a call
// holds.  With dimages NULL the last two are not launched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_cls.h"
#include "eht_closure.h"
#include "eht_terms.h"
#include "eht_uv_kernels.h"
#include "side_lib.h"

extern "C" const char *bhn_cls_last_error(void) { return side_last_error(); }

typedef EhtTerms<CLS_TERMS> ClsTerms;

// A lane adds its terms in order, the workgroup adds the lanes in a fixed order (eht_block_sum_256, the order of eht_loss_kernel):
// terms[d, n] does not depend on the planes computed with it.  `vis` is written and, after the barrier, read by this workgroup.
__global__ __launch_bounds__(256) void cls_loss_kernel(const EhtC *__restrict__ part, ClsPlan p, ClsTerms a, EhtC *vis,
                                                       const int32_t *__restrict__ tri, const int8_t *__restrict__ tri_sign,
                                                       const int32_t *__restrict__ quad, EhtC *__restrict__ gva, float *__restrict__ dphi,
                                                       float *__restrict__ dy, float *__restrict__ terms, int want_grad) {
    __shared__ float red[CLS_TERMS][4];
    const int n = blockIdx.x, nvis = p.e.nvis;
    float term[CLS_TERMS] = {0.f, 0.f, 0.f};
    for (int k = threadIdx.x; k < nvis; k += 256) {
        const size_t t = (size_t)n * nvis + k;
        const EhtC v = eht_combine(p.e, part, n, k);
        vis[t] = v;
        if (a.present[CLS_AMP]) {
            EhtC gv;
            term[CLS_AMP] += eht_term_amp(v, a.target[CLS_AMP][t], a.sigma[CLS_AMP][t], a.scale[CLS_AMP], &gv);
            if (want_grad) gva[t] = gv;
        }
    }
    __syncthreads();                                       // the plane's visibilities, written above by this workgroup
    if (a.present[CLS_CPHASE])
        for (int c = threadIdx.x; c < p.e.ncp; c += 256) {
            const size_t t = (size_t)n * p.e.ncp + c;
            float d;
            term[CLS_CPHASE] += eht_term_cphase(vis + (size_t)n * nvis, nvis, tri, tri_sign, c, a.target[CLS_CPHASE][t], a.sigma[CLS_CPHASE][t],
                                                a.scale[CLS_CPHASE], &d);
            dphi[t] = d;
        }
    if (a.present[CLS_LOGCAMP])
        for (int q = threadIdx.x; q < p.nca; q += 256) {
            const size_t t = (size_t)n * p.nca + q;
            float d;
            term[CLS_LOGCAMP] += cls_term_logcamp(vis + (size_t)n * nvis, nvis, quad, q, a.target[CLS_LOGCAMP][t], a.sigma[CLS_LOGCAMP][t],
                                                  a.scale[CLS_LOGCAMP], &d);
            dy[t] = d;
        }
#pragma unroll
    for (int d = 0; d < CLS_TERMS; ++d) {
        const float tot = eht_block_sum_256(term[d], red[d]);
        if (threadIdx.x == 0) terms[(size_t)d * p.e.N + n] = a.scale[d] * tot;
    }
}

// one wave per (plane, baseline); the lanes share a table, their sums are added in a butterfly (the order of eht_gather_kernel)
__global__ __launch_bounds__(256) void cls_gather_kernel(const EhtC *__restrict__ vis, ClsPlan p, ClsTerms a, const int32_t *__restrict__ tri,
                                                         const int8_t *__restrict__ tri_sign, const int32_t *__restrict__ quad,
                                                         const EhtC *__restrict__ gva, const float *__restrict__ dphi,
                                                         const float *__restrict__ dy, EhtC *__restrict__ gv) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.e.N * p.e.nvis) return;                      // (a whole wave leaves)
    const int n = t / p.e.nvis, k = t % p.e.nvis, lane = threadIdx.x & 63;
    const EhtC v = vis[t];
    EhtC g = {0.f, 0.f};
    bool first = true;
    if (a.present[CLS_AMP]) {
        g = gva[t];
        first = false;
    }
    if (a.present[CLS_CPHASE]) {
        float w = eht_gather_weight(k, tri, tri_sign, dphi + (size_t)n * p.e.ncp, p.e.ncp, lane, 64);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        g = cls_add_gv(first, g, eht_gather_gv(v, w));
        first = false;
    }
    if (a.present[CLS_LOGCAMP]) {
        float w = cls_gather_weight(k, quad, dy + (size_t)n * p.nca, p.nca, lane, 64);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        g = cls_add_gv(first, g, cls_gather_gv(v, w));
    }
    if (lane == 0) gv[t] = g;
}

extern "C" size_t bhn_cls_ws_bytes(int32_t N, int32_t nvis, int32_t ncp, int32_t nca, int32_t H, int32_t W) {
    ClsPlan p;
    return cls_make_plan(N, nvis, ncp, nca, H, W, &p) ? p.bytes : 0;
}

extern "C" int bhn_cls_chi2(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                            double psize_x, double psize_y, const bhn_cls_term *amp, const bhn_cls_term *cphase,
                            const bhn_cls_term *logcamp, const int32_t *tri, const int8_t *tri_sign, int32_t ncp, const int32_t *quad,
                            int32_t nca, float scale, float *loss, float *dimages, void *ws, size_t ws_bytes, void *stream) {
    ClsPlan p;
    ClsTerms a;
    const bhn_cls_term *const in[CLS_TERMS] = {amp, cphase, logcamp};
    static const char *const names[CLS_TERMS] = {"amp", "cphase", "logcamp"};
    BHN_CHECK_ARG(images && uv && ws && loss, "null pointer");
    BHN_CHECK_ARG(amp || cphase || logcamp, "no term present");
    if (int rc = eht_terms_take(in, names, scale, &a)) return rc;
    BHN_CHECK_ARG(!cphase || (ncp >= 1 && tri && tri_sign), "closure phases need a triangle table (ncp = %d, tri %s)", ncp,
                  tri && tri_sign ? "given" : "NULL");
    BHN_CHECK_ARG(!logcamp || (nca >= 1 && quad), "log closure amplitudes need a quadrangle table (nca = %d, quad %s)", nca,
                  quad ? "given" : "NULL");
    const char *why = eht_sizes_error(N, Sx, nvis, ncp, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(!why, "%s (N %d, Sx %d, nvis %d, ncp %d, H %d, W %d, pixel %g x %g rad)", why, N, Sx, nvis, ncp, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(nca >= 0, "nca must be >= 0 (nca = %d)", nca);
    BHN_CHECK_ARG(cls_make_plan(N, nvis, ncp, nca, H, W, &p), "sizes too large for one call (N %d, nvis %d, ncp %d, nca %d, H %d, W %d)", N, nvis,
                  ncp, nca, H, W);
    BHN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(uv) & 7) == 0, "ws and uv must be 8-byte aligned");
    if (ws_bytes < p.bytes)
        return side_fail(BHN_EWORKSPACE, "workspace of %zu bytes, bhn_cls_ws_bytes(%d, %d, %d, %d, %d, %d) = %zu", ws_bytes, N, nvis, ncp, nca, H, W,
                         p.bytes);

    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    EhtC *vis = reinterpret_cast<EhtC *>(w + p.e.off_vis), *gva = reinterpret_cast<EhtC *>(w + p.off_gva);
    EhtC *gv = reinterpret_cast<EhtC *>(w + p.off_gv);
    float *dphi = reinterpret_cast<float *>(w + p.e.off_dphi), *dy = reinterpret_cast<float *>(w + p.off_dy);
    float *terms = reinterpret_cast<float *>(w + p.off_terms);
    const int rf = eht_forward(images, uv, p.e, Sx, psize_x, psize_y, w, nullptr, st);
    if (rf != BHN_OK) return rf;
    // 'amp' alone: its gv is the sum, written where the adjoint reads it
    const bool amp_only = amp && !cphase && !logcamp;
    hipLaunchKernelGGL(cls_loss_kernel, dim3((unsigned)N), dim3(256), 0, st, reinterpret_cast<const EhtC *>(w + p.e.off_part), p, a, vis, tri,
                       tri_sign, quad, amp_only ? gv : gva, dphi, dy, terms, dimages ? 1 : 0);
    if (int rc = side_launched("cls_loss_kernel")) return rc;
    hipLaunchKernelGGL(eht_terms_sum_kernel<CLS_TERMS>, dim3(1), dim3(256), 0, st, loss, terms, (int)N, (int)N);
    if (int rc = side_launched("eht_terms_sum_kernel")) return rc;
    if (!dimages) return BHN_OK;
    if (!amp_only) {
        hipLaunchKernelGGL(cls_gather_kernel, dim3((unsigned)((N * nvis + 3) / 4)), dim3(256), 0, st, vis, p, a, tri, tri_sign, quad, gva, dphi, dy,
                           gv);
        if (int rc = side_launched("cls_gather_kernel")) return rc;
    }
    return eht_launch_adjoint(gv, w, p.e, Sx, dimages, st);
}
