// CPU build of the argument checks, the plan and the per-element arithmetic of libbhnerf_jnt.so (bhnerf_amd/csrc/joint_sum.h): the
// launch of bhn_jnt_sum walked one workgroup and one lane after the other, for tests/test_joint_cpu.py to compare with NumPy's
// float32 left-to-right sum bit for bit and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/joint_sum_host.cpp -o joint_sum_host
//   joint_sum_host IN OUT
//
// IN:  int64 [K, n, offset, alias, want_losses, bad], float32 src[K][n], float32 losses[K]
//      offset: every vector starts `offset` floats behind a 16-byte boundary (0: the 16-byte path, 1: the element path)
//      alias:  -1, or k: dst IS src[k]
//      bad:    0, or an argument to spoil: 1 a null src[0], 2 a null dst, 3 src[K-1] two bytes off, 4 dst two bytes off,
//              5 a null loss_in[K-1], 6 dst = src[0] + 1 (a partial overlap), 7 loss_out inside dst
// OUT: float32 dst[n], float32 loss_out[K + 1] (when want_losses)
// Exit status 1 with the message on stderr for arguments that bhn_jnt_sum refuses with BHN_EINVAL (K and n are passed as they are).
// Every vector is a heap block of exactly offset + n floats (at least one) and loss_out one of exactly K + 1, the outputs filled with
// NaN bytes first, so that an index outside them is caught and an element left unwritten shows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "joint_sum.h"

static float *block16(size_t floats) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, sizeof(float) * (floats ? floats : 1)) != 0) return nullptr;
    return static_cast<float *>(p);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[6];
    if (fread(head, sizeof(int64_t), 6, f) != 6) { fprintf(stderr, "short header\n"); return 2; }
    const int64_t K64 = head[0], n = head[1], offset = head[2], alias = head[3], bad = head[5];
    const bool want_losses = head[4] != 0;
    const int32_t K = (int32_t)K64;
    bhn_jnt_ptrs src = {}, loss_in = {};
    if (K < 1 || K > BHN_JNT_MAX_TERMS || n < 0 || n > JNT_MAX_N) {             // refused before anything is allocated
        const char *why = jnt_args_error(&src, K, n, nullptr, &loss_in, nullptr);
        fprintf(stderr, "%s\n", why ? why : "sizes accepted?");
        return 1;
    }
    if (offset < 0 || offset > 3 || alias >= K) { fprintf(stderr, "bad header\n"); return 2; }

    float *base[BHN_JNT_MAX_TERMS] = {nullptr};
    float losses[BHN_JNT_MAX_TERMS] = {0.f};
    const size_t N = (size_t)n;
    for (int k = 0; k < K; ++k) {
        base[k] = block16((size_t)offset + N);
        if (!base[k]) return 2;
        if (fread(base[k] + offset, sizeof(float), N, f) != N) { fprintf(stderr, "short input\n"); return 2; }
        src.p[k] = base[k] + offset;
    }
    if (fread(losses, sizeof(float), (size_t)K, f) != (size_t)K) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    for (int k = 0; k < K; ++k) loss_in.p[k] = &losses[k];

    float *dst_base = nullptr, *dst;
    if (alias >= 0) {
        dst = base[alias] + offset;
    } else {
        dst_base = block16((size_t)offset + N);
        if (!dst_base) return 2;
        memset(dst_base, 0xFF, sizeof(float) * ((size_t)offset + N));
        dst = dst_base + offset;
    }
    float *loss_out = want_losses ? (float *)malloc(sizeof(float) * (size_t)(K + 1)) : nullptr;
    if (want_losses && !loss_out) return 2;
    if (loss_out) memset(loss_out, 0xFF, sizeof(float) * (size_t)(K + 1));

    float *dst_arg = dst, *loss_out_arg = loss_out;        // (the spoilt pointers are checked, never dereferenced)
    switch (bad) {
    case 0: break;
    case 1: src.p[0] = nullptr; break;
    case 2: dst_arg = nullptr; break;
    case 3: src.p[K - 1] = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(src.p[K - 1]) + 2); break;
    case 4: dst_arg = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(dst) + 2); break;
    case 5: loss_in.p[K - 1] = nullptr; break;
    case 6: dst_arg = const_cast<float *>(src.p[0]) + 1; break;
    case 7: loss_out_arg = dst; break;
    default: fprintf(stderr, "bad header\n"); return 2;
    }
    const char *why = jnt_args_error(&src, K, n, dst_arg, &loss_in, loss_out_arg);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    if (bad) { fprintf(stderr, "spoilt argument %d accepted\n", (int)bad); return 2; }

    const JntPlan p = jnt_make_plan(&src, K, n, dst, loss_out != nullptr);
    for (int b = 0; b < p.blocks; ++b)                                          // jnt_sum_kernel: workgroup after workgroup
        for (int lane = 0; lane < JNT_BLOCK; ++lane) {
            jnt_lane(p, src, K, dst, b, lane);
            if (loss_out && b == 0 && lane == 0) jnt_losses(loss_in, K, loss_out);
        }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(dst, sizeof(float), N, o) == N;
    if (loss_out) ok = ok && fwrite(loss_out, sizeof(float), (size_t)(K + 1), o) == (size_t)(K + 1);
    const int32_t path[2] = {p.vec, p.blocks};                                  // the path the plan took, for the test to see
    ok = ok && fwrite(path, sizeof(int32_t), 2, o) == 2;
    ok = (fclose(o) == 0) && ok;
    for (int k = 0; k < K; ++k) free(base[k]);
    free(dst_base);
    free(loss_out);
    return ok ? 0 : 2;
}
