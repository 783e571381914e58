// libbhnerf_jnt.so (include/bhnerf_jnt.h): the fan-in of a joint training step -- up to eight float32 vectors added left to right,
// the terms' losses gathered with their sum.
//
// csrc/joint_sum.h holds the argument checks, the plan and the per-element arithmetic, shared with the CPU build of
// tools/joint_sum_host.cpp.  ONE launch on the caller's stream:
//   jnt_sum_kernel     workgroups of JNT_BLOCK lanes, grid-stride, at most BHN_JNT_MAX_BLOCKS of them: a lane adds the K sources of
//                      its unit (four elements by 16-byte loads when every pointer allows it, else one) and writes dst; lane 0 of
//                      workgroup 0 reads the K losses, then writes their sum and them
// Memory-bound: 4 K bytes read and 4 written per element, no LDS, no reduction across lanes.  The pointers travel by value in the
// kernel arguments.  No atomics, no allocation, no synchronisation: every sum has one fixed order.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_jnt.h"
#include "side_lib.h"
#include "joint_sum.h"

extern "C" const char *bhn_jnt_last_error(void) { return side_last_error(); }

// dst may be one of the sources: no __restrict__ anywhere.  Every index is checked against the plan's sizes in jnt_lane.
__global__ __launch_bounds__(JNT_BLOCK) void jnt_sum_kernel(bhn_jnt_ptrs src, int K, JntPlan p, float *dst, bhn_jnt_ptrs loss_in, float *loss_out) {
    jnt_lane(p, src, K, dst, (int)blockIdx.x, (int)threadIdx.x);
    if (loss_out && blockIdx.x == 0 && threadIdx.x == 0) jnt_losses(loss_in, K, loss_out);
}

extern "C" int bhn_jnt_sum(const bhn_jnt_ptrs *src, int32_t K, int64_t n, float *dst, const bhn_jnt_ptrs *loss_in, float *loss_out,
                           void *stream) {
    const char *why = jnt_args_error(src, K, n, dst, loss_in, loss_out);
    BHN_CHECK_ARG(!why, "%s (K %d, n %lld)", why, K, (long long)n);
    const JntPlan p = jnt_make_plan(src, K, n, dst, loss_out != nullptr);
    if (p.blocks == 0) return BHN_OK;
    bhn_jnt_ptrs none = {};
    hipLaunchKernelGGL(jnt_sum_kernel, dim3((unsigned)p.blocks), dim3(JNT_BLOCK), 0, (hipStream_t)stream, *src, (int)K, p, dst,
                       loss_out ? *loss_in : none, loss_out);
    return side_launched("jnt_sum_kernel");
}
