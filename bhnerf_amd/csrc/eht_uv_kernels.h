// The device kernels that libbhnerf_eht.so (csrc/eht_uv.hip), libbhnerf_cls.so (csrc/eht_closure.hip) and libbhnerf_pol.so
// (csrc/eht_pol.hip) share: twiddle tables, forward partial sums, their combination, the 256-lane block sum and the adjoint, with
// eht_forward, the launches of the first three, and eht_launch_adjoint, the launch of the last.  One text for the libraries: the
// visibilities and the adjoint of each are the same arithmetic in the same order, so V and dimages of one are bitwise another's.  HIP only; the plan and the per-element arithmetic are csrc/eht_uv.h.
#ifndef BHNERF_EHT_UV_KERNELS_H
#define BHNERF_EHT_UV_KERNELS_H

#include <hip/hip_runtime.h>

#include "eht_uv.h"
#include "side_lib.h"

__global__ __launch_bounds__(256) void eht_twiddle_kernel(const double *__restrict__ uv, EhtPlan p, int B, double psize_x, double psize_y,
                                                          EhtC *__restrict__ Eu, EhtC *__restrict__ Ev) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int span = p.W + p.H;
    if (t >= (long long)B * p.nvis * span) return;
    const long long bk = t / span;
    const int i = (int)(t - bk * span);
    if (i < p.W)
        Eu[bk * p.W + i] = eht_twiddle(uv[2 * bk], i, p.W, psize_x);
    else
        Ev[bk * p.H + (i - p.W)] = eht_twiddle(uv[2 * bk + 1], i - p.W, p.H, psize_y);
}

__global__ __launch_bounds__(256) void eht_fwd_kernel(const float *__restrict__ images, const EhtC *__restrict__ Eu, const EhtC *__restrict__ Ev,
                                                      EhtPlan p, int Sx, EhtC *__restrict__ part) {
    __shared__ EhtC red[EHT_KB][4];
    const int k0 = blockIdx.x * EHT_KB, s = blockIdx.y, n = blockIdx.z, b = n / Sx;
    EhtC acc[EHT_KB];
#pragma unroll
    for (int j = 0; j < EHT_KB; ++j) acc[j].x = acc[j].y = 0.f;
    for (int x = threadIdx.x; x < p.W; x += blockDim.x) {
        EhtC col[EHT_KB];
        eht_columns(p, images, Eu, Ev, n, b, k0, s, x, col);
#pragma unroll
        for (int j = 0; j < EHT_KB; ++j) {
            acc[j].x += col[j].x;
            acc[j].y += col[j].y;
        }
    }
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int j = 0; j < EHT_KB; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc[j].x += __shfl_xor(acc[j].x, o, 64);
            acc[j].y += __shfl_xor(acc[j].y, o, 64);
        }
        if ((threadIdx.x & 63) == 0) red[j][wave] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < EHT_KB && k0 + (int)threadIdx.x < p.nvis) {
        EhtC v = red[threadIdx.x][0];
        for (int w = 1; w < waves; ++w) {
            v.x += red[threadIdx.x][w].x;
            v.y += red[threadIdx.x][w].y;
        }
        part[eht_part_index(p, n, k0 + threadIdx.x, s)] = v;
    }
}

__global__ __launch_bounds__(256) void eht_combine_kernel(const EhtC *__restrict__ part, EhtPlan p, EhtC *__restrict__ vis) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.N * p.nvis) return;
    vis[t] = eht_combine(p, part, t / p.nvis, t % p.nvis);
}

__device__ __forceinline__ float eht_block_sum_256(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void eht_adjoint_kernel(const EhtC *__restrict__ gv, const EhtC *__restrict__ Eu, const EhtC *__restrict__ Ev,
                                                          EhtPlan p, int Sx, float *__restrict__ dimages) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y0 = blockIdx.y * EHT_ADJ_ROWS, n = blockIdx.z, b = n / Sx;
    if (x >= p.W) return;
    float acc[EHT_ADJ_ROWS];
    int yy[EHT_ADJ_ROWS];
#pragma unroll
    for (int r = 0; r < EHT_ADJ_ROWS; ++r) {
        acc[r] = 0.f;
        yy[r] = y0 + r < p.H ? y0 + r : p.H - 1;          // rows past the image repeat the last one and are not stored
    }
#pragma unroll 4
    for (int k = 0; k < p.nvis; ++k) {                      // (unrolled: the loads of four baselines in flight)
        const EhtC z = eht_adjoint_z(gv[(size_t)n * p.nvis + k], Eu[eht_eu_index(p, b, k, x)]);
        const size_t ev = eht_ev_index(p, b, k, 0);
#pragma unroll
        for (int r = 0; r < EHT_ADJ_ROWS; ++r) acc[r] = eht_adjoint_mac(acc[r], z, Ev[ev + yy[r]]);
    }
#pragma unroll
    for (int r = 0; r < EHT_ADJ_ROWS; ++r)
        if (y0 + r < p.H) dimages[((size_t)n * p.H + y0 + r) * p.W + x] = acc[r];
}

// twiddle tables, forward partial sums and, given `vis`, their combination into it
static int eht_forward(const float *images, const double *uv, const EhtPlan &p, int32_t Sx, double psize_x, double psize_y, char *ws,
                       EhtC *vis, hipStream_t st) {
    EhtC *Eu = reinterpret_cast<EhtC *>(ws + p.off_eu), *Ev = reinterpret_cast<EhtC *>(ws + p.off_ev);
    EhtC *part = reinterpret_cast<EhtC *>(ws + p.off_part);
    const int B = p.N / Sx;
    const long long tw = (long long)B * p.nvis * (p.W + p.H);
    hipLaunchKernelGGL(eht_twiddle_kernel, dim3((unsigned)((tw + 255) / 256)), dim3(256), 0, st, uv, p, B, psize_x, psize_y, Eu, Ev);
    if (int rc = side_launched("eht_twiddle_kernel")) return rc;
    hipLaunchKernelGGL(eht_fwd_kernel, dim3((unsigned)p.kblocks, (unsigned)p.RS, (unsigned)p.N), dim3((unsigned)p.block), 0, st, images, Eu, Ev, p,
                       Sx, part);
    if (int rc = side_launched("eht_fwd_kernel")) return rc;
    if (!vis) return BHN_OK;                               // (bhn_eht_chi2_uv combines in its loss stage)
    hipLaunchKernelGGL(eht_combine_kernel, dim3((unsigned)((p.N * p.nvis + 255) / 256)), dim3(256), 0, st, part, p, vis);
    return side_launched("eht_combine_kernel");
}

// the adjoint of gv (N, nvis) into dimages, from the twiddle tables eht_forward left in the workspace
static int eht_launch_adjoint(const EhtC *gv, const char *ws, const EhtPlan &p, int32_t Sx, float *dimages, hipStream_t st) {
    hipLaunchKernelGGL(eht_adjoint_kernel, dim3((unsigned)((p.W + p.block - 1) / p.block), (unsigned)((p.H + EHT_ADJ_ROWS - 1) / EHT_ADJ_ROWS),
                                                (unsigned)p.N),
                       dim3((unsigned)p.block), 0, st, gv, reinterpret_cast<const EhtC *>(ws + p.off_eu),
                       reinterpret_cast<const EhtC *>(ws + p.off_ev), p, Sx, dimages);
    return side_launched("eht_adjoint_kernel");
}

#endif /* BHNERF_EHT_UV_KERNELS_H */
