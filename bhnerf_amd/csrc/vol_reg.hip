// libbhnerf_reg.so (include/bhnerf_reg.h): the volume priors tv, tsv and l1 on the recovered 3-D emission, with the gradient in
// the volumes.
//
// csrc/vol_reg.h holds the plan and the per-voxel arithmetic, shared with the CPU build of tools/vol_reg_host.cpp.  The launches
// of a call, both on the caller's stream:
//   reg_voxel_kernel   one workgroup per chunk of REG_CHUNK voxels of one volume, k contiguous over the lanes: a lane takes
//                      REG_TRIPS voxels REG_BLOCK apart, adds their terms in order and writes their gradient (the gather form:
//                      13 loads of e per voxel, served by L1 / L2 but for the voxel's own); three block sums per workgroup go
//                      to the workspace
//   reg_sum_kernel     ONE workgroup: per volume, in order, the lanes add the chunks' partial sums strided, the workgroup adds
//                      the lanes (per_volume), then lane 0 adds the volumes in order and scales (loss)
// A memory-bound stencil: 4 bytes of e and 1 of the mask read, 4 bytes of gradient written per voxel from HBM; no LDS tiling,
// the re-reads hit the caches.  No atomics, no allocation, no synchronisation: every sum has one fixed order.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_reg.h"
#include "side_lib.h"
#include "vol_reg.h"

extern "C" const char *bhn_reg_last_error(void) { return side_last_error(); }

// lanes of a wave by butterfly, the four waves in order: every lane returns the sum.  `red` is free again after the next barrier.
__device__ __forceinline__ float reg_block_sum_256(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// grid: N chunks workgroups, workgroup b = chunk b % chunks of volume b / chunks.  Every voxel index is checked against V before
// any access; part is written at (n, d, chunk) with n < N, chunk < chunks.
__global__ __launch_bounds__(REG_BLOCK) void reg_voxel_kernel(const float *__restrict__ volumes, const uint8_t *__restrict__ mask, RegPlan p,
                                                              RegParams a, float *__restrict__ part, float *__restrict__ dvolumes) {
    __shared__ float red[REG_TERMS][4];
    const int n = blockIdx.x / p.chunks, chunk = blockIdx.x - n * p.chunks;
    const float *e = volumes + (size_t)n * p.V;
    float *grad = dvolumes ? dvolumes + (size_t)n * p.V : nullptr;
    float acc[REG_TERMS] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < REG_TRIPS; ++t) {
        const int64_t v = (int64_t)chunk * REG_CHUNK + t * REG_BLOCK + threadIdx.x;
        if (v < p.V) {
            float term[REG_TERMS];
            reg_voxel(p, a, e, mask, v, term, grad);
#pragma unroll
            for (int d = 0; d < REG_TERMS; ++d) acc[d] += term[d];
        }
    }
#pragma unroll
    for (int d = 0; d < REG_TERMS; ++d) {
        const float tot = reg_block_sum_256(acc[d], red[d]);
        if (threadIdx.x == 0) part[reg_part_index(p, n, d, chunk)] = tot;
    }
}

// one workgroup.  pv[d][n] (workspace) and per_volume[d][n] (when given) = the chunks' sums of volume n; loss by reg_finish
__global__ __launch_bounds__(REG_BLOCK) void reg_sum_kernel(const float *__restrict__ part, RegPlan p, RegParams a, float *__restrict__ pv,
                                                            float *__restrict__ per_volume, float *__restrict__ loss) {
    __shared__ float red[REG_TERMS][4];
    for (int n = 0; n < p.N; ++n) {
#pragma unroll
        for (int d = 0; d < REG_TERMS; ++d) {
            float acc = 0.f;
            for (int c = threadIdx.x; c < p.chunks; c += REG_BLOCK) acc += part[reg_part_index(p, n, d, c)];
            const float tot = reg_block_sum_256(acc, red[d]);
            if (threadIdx.x == 0) {
                pv[(size_t)d * p.N + n] = tot;
                if (per_volume) per_volume[(size_t)d * p.N + n] = tot;
            }
        }
        __syncthreads();              // red is written again for the next volume
    }
    if (threadIdx.x == 0) reg_finish(a, pv, p.N, loss);      // lane 0 reads what lane 0 wrote
}

extern "C" size_t bhn_reg_ws_bytes(int32_t N, int32_t nx, int32_t ny, int32_t nz) {
    RegPlan p;
    return reg_make_plan(N, nx, ny, nz, &p) ? p.bytes : 0;
}

extern "C" int bhn_reg_loss(const float *volumes, int32_t N, int32_t nx, int32_t ny, int32_t nz, const uint8_t *mask, const float spacing[3],
                            const float weights[3], float eps, float scale, float *loss, float *per_volume, float *dvolumes, void *ws,
                            size_t ws_bytes, void *stream) {
    RegPlan p;
    BHN_CHECK_ARG(volumes && spacing && weights && loss && ws, "null pointer");
    BHN_CHECK_ARG(N >= 1 && nx >= 1 && ny >= 1 && nz >= 1, "sizes must be at least 1 (N %d, dims %d x %d x %d)", N, nx, ny, nz);
    BHN_CHECK_ARG(reg_make_plan(N, nx, ny, nz, &p), "sizes too large for one call (N %d, dims %d x %d x %d)", N, nx, ny, nz);
    const char *why = reg_params_error(spacing, weights, eps, scale);
    BHN_CHECK_ARG(!why, "%s (spacing %g %g %g, weights %g %g %g, eps %g, scale %g)", why, spacing[0], spacing[1], spacing[2], weights[0],
                  weights[1], weights[2], eps, scale);
    BHN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "ws must be 4-byte aligned");
    if (ws_bytes < p.bytes)
        return side_fail(BHN_EWORKSPACE, "workspace of %zu bytes, bhn_reg_ws_bytes(%d, %d, %d, %d) = %zu", ws_bytes, N, nx, ny, nz, p.bytes);

    const RegParams a = reg_make_params(spacing, weights, eps, scale);
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    float *part = reinterpret_cast<float *>(w + p.off_part), *pv = reinterpret_cast<float *>(w + p.off_pv);
    hipLaunchKernelGGL(reg_voxel_kernel, dim3((unsigned)((int64_t)p.chunks * N)), dim3(REG_BLOCK), 0, st, volumes, mask, p, a, part, dvolumes);
    if (int rc = side_launched("reg_voxel_kernel")) return rc;
    hipLaunchKernelGGL(reg_sum_kernel, dim3(1), dim3(REG_BLOCK), 0, st, part, p, a, pv, per_volume, loss);
    return side_launched("reg_sum_kernel");
}
