// libbhnerf_eht.so (include/bhnerf_eht.h): the EHT chi-square ('vis' | 'amp' | 'cphase') and its image gradient from the (u, v)
// coordinates of the baselines, without the dense DFT matrices of bhn_chi2_eht (csrc/simple_kernels.hip).
//
// csrc/eht_uv.h holds the plan (workspace layout, row splits) and the per-element arithmetic, shared with the CPU build of
// tools/eht_uv_host.cpp; csrc/eht_uv_kernels.h holds the twiddle, forward, combine and adjoint kernels with their launches (eht_forward,
// eht_launch_adjoint), shared with libbhnerf_cls.so and libbhnerf_pol.so.  The launches of a call, all on the caller's stream:
//   eht_twiddle_kernel   Eu (B, nvis, W), Ev (B, nvis, H) into the workspace: float64 phase, reduced to turns, rounded to complex64
//   eht_fwd_kernel       grid (baseline blocks of EHT_KB, row splits, planes): a lane owns image columns; a pixel is loaded into
//                        a register once and multiplies the Ev of all EHT_KB baselines, the column sums are then rotated by Eu and
//                        summed over the workgroup (xor butterfly per wave, the waves in order): one partial sum per
//                        (plane, baseline, row split)
//   eht_combine_kernel   bhn_eht_vis only: a visibility = its row splits' partial sums in order
//   eht_loss_kernel      one workgroup per plane: the same combination, then the chi^2 terms -- 'vis' / 'amp' one lane per visibility,
//                        'cphase' one lane per triangle, phi from the index table
//   eht_loss_sum_kernel  the planes' loss sums in order
//   eht_gather_kernel    'cphase' only: a baseline's gradient gathered from its triangles, one wave per (plane, baseline)
//   eht_adjoint_kernel   (eht_launch_adjoint) grid (column blocks, EHT_ADJ_ROWS-row strips, planes): per pixel a loop over the baselines
// No atomics, no allocation, no synchronisation: every sum has one fixed order, and that order does not depend on how many frames
// a call holds.  The image is read nvis / EHT_KB times in the forward pass (from L2 after the first), the tables are the only
// other traffic: nothing of size nvis x H x W is ever read or written.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_eht.h"
#include "eht_uv.h"
#include "eht_uv_kernels.h"      // the kernels shared with libbhnerf_cls.so and libbhnerf_pol.so, eht_forward, eht_launch_adjoint
#include "side_lib.h"

extern "C" const char *bhn_eht_last_error(void) { return side_last_error(); }

// Stage 2 and the loss, one workgroup per plane: a visibility = its row splits' partial sums in order; 'vis' | 'amp': the chi^2
// term of each visibility and, with want_grad, gv = dL/dRe(vis) + i dL/dIm(vis) written in its place; 'cphase': the visibilities are
// written first, then one lane per triangle takes phi from the index table and leaves dL/dphi in dphi.  A lane adds its terms in
// order, the workgroup adds the lanes in a fixed order: loss_part[n] does not depend on the planes computed with it.
__global__ __launch_bounds__(256) void eht_loss_kernel(const EhtC *__restrict__ part, EhtPlan p, EhtC *__restrict__ vis,
                                                       const int32_t *__restrict__ tri, const int8_t *__restrict__ tri_sign,
                                                       const float *__restrict__ target, const float *__restrict__ sigma, float scale,
                                                       int dtype, float *__restrict__ dphi, float *__restrict__ loss_part, int want_grad) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    float term = 0.f;
    for (int k = threadIdx.x; k < p.nvis; k += 256) {
        const size_t t = (size_t)n * p.nvis + k;
        const EhtC v = eht_combine(p, part, n, k);
        EhtC gv = v;
        if (dtype == EHT_DTYPE_VIS)
            term += eht_term_vis(v, target[2 * t], target[2 * t + 1], sigma[t], scale, &gv);
        else if (dtype == EHT_DTYPE_AMP)
            term += eht_term_amp(v, target[t], sigma[t], scale, &gv);
        vis[t] = (want_grad || dtype == EHT_DTYPE_CPHASE) ? gv : v;
    }
    if (dtype == EHT_DTYPE_CPHASE) {
        __syncthreads();                                   // the plane's visibilities, written above by this workgroup
        for (int c = threadIdx.x; c < p.ncp; c += 256) {
            const size_t t = (size_t)n * p.ncp + c;
            float d;
            term += eht_term_cphase(vis + (size_t)n * p.nvis, p.nvis, tri, tri_sign, c, target[t], sigma[t], scale, &d);
            dphi[t] = d;
        }
    }
    const float tot = eht_block_sum_256(term, red);
    if (threadIdx.x == 0) loss_part[n] = scale * tot;
}

// 'cphase': one wave per (plane, baseline); the lanes share the table, their sums are added in a butterfly
__global__ __launch_bounds__(256) void eht_gather_kernel(EhtC *__restrict__ vis, EhtPlan p, const int32_t *__restrict__ tri,
                                                         const int8_t *__restrict__ tri_sign, const float *__restrict__ dphi) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.N * p.nvis) return;                          // (a whole wave leaves)
    const int n = t / p.nvis, k = t % p.nvis;
    float w = eht_gather_weight(k, tri, tri_sign, dphi + (size_t)n * p.ncp, p.ncp, threadIdx.x & 63, 64);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if ((threadIdx.x & 63) == 0) vis[t] = eht_gather_gv(vis[t], w);
}

__global__ __launch_bounds__(256) void eht_loss_sum_kernel(float *__restrict__ loss, const float *__restrict__ part, int n) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    const float tot = eht_block_sum_256(acc, red);
    if (threadIdx.x == 0) loss[0] = tot;
}

extern "C" size_t bhn_eht_ws_bytes(int32_t N, int32_t nvis, int32_t ncp, int32_t H, int32_t W) {
    EhtPlan p;
    return eht_make_plan(N, nvis, ncp, H, W, &p) ? p.bytes : 0;
}

// the argument checks and the plan of both entry points; nothing is launched when this fails
static int eht_prepare(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t ncp, int32_t H, int32_t W,
                       double psize_x, double psize_y, void *ws, size_t ws_bytes, EhtPlan *p) {
    BHN_CHECK_ARG(images && uv && ws, "null pointer");
    const char *why = eht_sizes_error(N, Sx, nvis, ncp, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(!why, "%s (N %d, Sx %d, nvis %d, ncp %d, H %d, W %d, pixel %g x %g rad)", why, N, Sx, nvis, ncp, H, W, psize_x, psize_y);
    BHN_CHECK_ARG(eht_make_plan(N, nvis, ncp, H, W, p), "sizes too large for one call (N %d, nvis %d, ncp %d, H %d, W %d)", N, nvis, ncp, H, W);
    BHN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(uv) & 7) == 0, "ws and uv must be 8-byte aligned");
    if (ws_bytes < p->bytes)
        return side_fail(BHN_EWORKSPACE, "workspace of %zu bytes, bhn_eht_ws_bytes(%d, %d, %d, %d, %d) = %zu", ws_bytes, N, nvis, ncp, H, W, p->bytes);
    return BHN_OK;
}

extern "C" int bhn_eht_vis(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W, double psize_x,
                           double psize_y, float *vis_out, void *ws, size_t ws_bytes, void *stream) {
    EhtPlan p;
    BHN_CHECK_ARG(vis_out, "null pointer");
    BHN_CHECK_ARG((reinterpret_cast<uintptr_t>(vis_out) & 7) == 0, "vis_out must be 8-byte aligned");
    const int rc = eht_prepare(images, uv, N, Sx, nvis, 0, H, W, psize_x, psize_y, ws, ws_bytes, &p);
    if (rc != BHN_OK) return rc;
    return eht_forward(images, uv, p, Sx, psize_x, psize_y, static_cast<char *>(ws), reinterpret_cast<EhtC *>(vis_out), (hipStream_t)stream);
}

extern "C" int bhn_eht_chi2_uv(const float *images, const double *uv, int32_t N, int32_t Sx, int32_t nvis, int32_t H, int32_t W,
                               double psize_x, double psize_y, int32_t dtype, const float *target, const float *sigma, float scale,
                               const int32_t *tri, const int8_t *tri_sign, int32_t ncp, float *loss, float *dimages, void *ws,
                               size_t ws_bytes, void *stream) {
    EhtPlan p;
    BHN_CHECK_ARG(target && sigma && loss, "null pointer");
    BHN_CHECK_ARG(dtype >= 0 && dtype <= 2, "eht dtype (%d) not supported", dtype);
    BHN_CHECK_ARG(ncp <= 0 || (tri && tri_sign), "ncp = %d closure triangles with a NULL table", ncp);
    BHN_CHECK_ARG(dtype != EHT_DTYPE_CPHASE || ncp >= 1, "closure phases need a triangle table (ncp = %d)", ncp);
    const int rc = eht_prepare(images, uv, N, Sx, nvis, ncp, H, W, psize_x, psize_y, ws, ws_bytes, &p);
    if (rc != BHN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    EhtC *vis = reinterpret_cast<EhtC *>(w + p.off_vis);
    float *dphi = reinterpret_cast<float *>(w + p.off_dphi), *loss_part = reinterpret_cast<float *>(w + p.off_loss);
    const int rf = eht_forward(images, uv, p, Sx, psize_x, psize_y, w, nullptr, st);
    if (rf != BHN_OK) return rf;
    hipLaunchKernelGGL(eht_loss_kernel, dim3((unsigned)N), dim3(256), 0, st, reinterpret_cast<const EhtC *>(w + p.off_part), p, vis, tri, tri_sign,
                       target, sigma, scale, dtype, dphi, loss_part, dimages ? 1 : 0);
    if (int rc = side_launched("eht_loss_kernel")) return rc;
    hipLaunchKernelGGL(eht_loss_sum_kernel, dim3(1), dim3(256), 0, st, loss, loss_part, (int)N);
    if (int rc = side_launched("eht_loss_sum_kernel")) return rc;
    if (!dimages) return BHN_OK;
    if (dtype == EHT_DTYPE_CPHASE) {
        hipLaunchKernelGGL(eht_gather_kernel, dim3((unsigned)((N * nvis + 3) / 4)), dim3(256), 0, st, vis, p, tri, tri_sign, dphi);
        if (int rc = side_launched("eht_gather_kernel")) return rc;
    }
    return eht_launch_adjoint(vis, w, p, Sx, dimages, st);
}
