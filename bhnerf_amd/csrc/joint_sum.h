// The fan-in of a joint training step (libbhnerf_jnt.so, include/bhnerf_jnt.h): the argument checks, the plan of the launch and
// the per-element arithmetic, without HIP dependencies.  csrc/joint_sum.hip runs this code on the device; tools/joint_sum_host.cpp
// compiles the same header with a plain C++ compiler and walks the same plan one lane after the other (tests/test_joint_cpu.py).
//
// dst[i] = ((src[0][i] + src[1][i]) + ... + src[K-1][i]) in float32, left to right; loss_out = {sum of the K losses, left to
// right, then the K losses}.  An element is read from every src before it is written to dst and no other lane touches it, so dst
// may be one of the src.
#ifndef BHNERF_JOINT_SUM_H
#define BHNERF_JOINT_SUM_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bhnerf_jnt.h"

#if defined(__HIPCC__)
#define JNT_HD __host__ __device__ inline
#else
#define JNT_HD inline
#endif

#define JNT_BLOCK 256             // lanes per workgroup
#define JNT_VEC 4                 // elements of a 16-byte load
#define JNT_MAX_N ((int64_t)1 << 40)

// four elements as one 16-byte unit, for the host walk and the device alike (the device reads it with one 16-byte load)
struct alignas(16) JntVec {
    float v[JNT_VEC];
};

// ---------------------------------------------------------------------------------------------------------------------------
// The argument checks of bhn_jnt_sum: NULL, or the message of BHN_EINVAL.  Nothing is dereferenced but the two host structs.
// ---------------------------------------------------------------------------------------------------------------------------
inline bool jnt_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [a, a + na) and [b, b + nb) bytes share a byte
inline bool jnt_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

inline const char *jnt_args_error(const bhn_jnt_ptrs *src, int32_t K, int64_t n, const float *dst, const bhn_jnt_ptrs *loss_in,
                                  const float *loss_out) {
    if (K < 1 || K > BHN_JNT_MAX_TERMS) return "K must be in [1, BHN_JNT_MAX_TERMS]";
    if (n < 0 || n > JNT_MAX_N) return "n must be in [0, 2^40]";
    if (!src) return "null src";
    for (int k = 0; k < K; ++k) {
        if (!src->p[k]) return "null src pointer";
        if (!jnt_aligned(src->p[k], 4)) return "src pointer not 4-byte aligned";
    }
    if (n > 0 && !dst) return "null dst";
    if (!jnt_aligned(dst, 4)) return "dst not 4-byte aligned";
    const uint64_t bytes = (uint64_t)n * sizeof(float);
    for (int k = 0; k < K; ++k)
        if (src->p[k] != dst && jnt_overlap(dst, bytes, src->p[k], bytes)) return "dst overlaps a src pointer partially";
    if (loss_out) {
        if (!jnt_aligned(loss_out, 4)) return "loss_out not 4-byte aligned";
        if (!loss_in) return "null loss_in";
        for (int k = 0; k < K; ++k) {
            if (!loss_in->p[k]) return "null loss_in pointer";
            if (!jnt_aligned(loss_in->p[k], 4)) return "loss_in pointer not 4-byte aligned";
        }
        if (jnt_overlap(dst, bytes, loss_out, sizeof(float) * (uint64_t)(K + 1))) return "loss_out overlaps dst";
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The plan of the launch.  Lane t of workgroup b starts at unit b JNT_BLOCK + t and strides by blocks JNT_BLOCK units; a unit
// is four elements on the 16-byte path (units = n / 4, the n % 4 tail elements go to the first lanes of workgroup 0), one
// element otherwise.  Every index is below n.
// ---------------------------------------------------------------------------------------------------------------------------
struct JntPlan {
    int32_t vec;                  // 1: the 16-byte path
    int32_t blocks;               // workgroups: 0 when there is nothing to do
    int64_t units;                // float4 units (vec) or elements
    int64_t tail0;                // first element of the scalar tail (vec), n otherwise
    int64_t n;
};

inline JntPlan jnt_make_plan(const bhn_jnt_ptrs *src, int32_t K, int64_t n, const float *dst, bool losses) {
    JntPlan p;
    bool vec = jnt_aligned(dst, 16);
    for (int k = 0; k < K; ++k) vec = vec && jnt_aligned(src->p[k], 16);
    p.vec = vec ? 1 : 0;
    p.n = n;
    p.units = vec ? n / JNT_VEC : n;
    p.tail0 = vec ? p.units * JNT_VEC : n;
    int64_t blocks = (p.units + JNT_BLOCK - 1) / JNT_BLOCK;
    if (blocks > BHN_JNT_MAX_BLOCKS) blocks = BHN_JNT_MAX_BLOCKS;
    if (blocks == 0 && (losses || p.tail0 < n)) blocks = 1;
    p.blocks = (int32_t)blocks;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The arithmetic.  K is at most BHN_JNT_MAX_TERMS; the loops have that fixed bound so that the by-value pointers stay in
// registers on the device.
// ---------------------------------------------------------------------------------------------------------------------------
JNT_HD float jnt_sum1(const bhn_jnt_ptrs &src, int K, int64_t i) {
    float acc = src.p[0][i];
#pragma unroll
    for (int k = 1; k < BHN_JNT_MAX_TERMS; ++k)
        if (k < K) acc += src.p[k][i];
    return acc;
}

JNT_HD JntVec jnt_sum4(const bhn_jnt_ptrs &src, int K, int64_t u) {
    JntVec acc = reinterpret_cast<const JntVec *>(src.p[0])[u];
#pragma unroll
    for (int k = 1; k < BHN_JNT_MAX_TERMS; ++k)
        if (k < K) {
            const JntVec x = reinterpret_cast<const JntVec *>(src.p[k])[u];
#pragma unroll
            for (int j = 0; j < JNT_VEC; ++j) acc.v[j] += x.v[j];
        }
    return acc;
}

// what one lane (workgroup `block`, lane `lane`) of the launch does to dst
JNT_HD void jnt_lane(const JntPlan &p, const bhn_jnt_ptrs &src, int K, float *dst, int block, int lane) {
    const int64_t stride = (int64_t)p.blocks * JNT_BLOCK;
    for (int64_t u = (int64_t)block * JNT_BLOCK + lane; u < p.units; u += stride) {
        if (p.vec)
            reinterpret_cast<JntVec *>(dst)[u] = jnt_sum4(src, K, u);
        else
            dst[u] = jnt_sum1(src, K, u);
    }
    if (block == 0 && p.tail0 + lane < p.n) dst[p.tail0 + lane] = jnt_sum1(src, K, p.tail0 + lane);
}

// what lane 0 of workgroup 0 does to loss_out: the K values are read before anything is written
JNT_HD void jnt_losses(const bhn_jnt_ptrs &loss_in, int K, float *loss_out) {
    float v[BHN_JNT_MAX_TERMS];
#pragma unroll
    for (int k = 0; k < BHN_JNT_MAX_TERMS; ++k) v[k] = k < K ? *loss_in.p[k] : 0.f;
    float total = v[0];
#pragma unroll
    for (int k = 1; k < BHN_JNT_MAX_TERMS; ++k)
        if (k < K) total += v[k];
    loss_out[0] = total;
#pragma unroll
    for (int k = 0; k < BHN_JNT_MAX_TERMS; ++k)
        if (k < K) loss_out[1 + k] = v[k];
}

#endif
