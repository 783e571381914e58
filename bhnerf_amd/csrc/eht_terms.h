// The term layer of the weighted-term losses from (u, v) coordinates -- loss = scale sum_d w_d chi^2_d over NT terms in a canonical
// order, each optional -- shared by libbhnerf_cls.so (csrc/eht_closure.hip, NT 3) and libbhnerf_pol.so (csrc/eht_pol.hip, NT 2):
// the effective scale of a term, the terms of a call as the kernels take them, their argument check, and the kernel that adds the
// planes' sums of each term and forms the total.  Outside the __HIPCC__ block a plain C++ compiler takes it: tools/eht_closure_host.cpp
// and tools/eht_pol_host.cpp form their scales with the same functions.
//
// A new term supplies: its index in the canonical order (and NT + 1), its arithmetic in the library's loss kernel, and one more
// term-struct argument of the entry point.
#ifndef BHNERF_EHT_TERMS_H
#define BHNERF_EHT_TERMS_H

#include "eht_uv.h"
#include "side_lib.h"

// The effective scale of a term: scale w_d, formed once on the host and rounded once to float32 (weight 1 changes no bit).
EHT_HD float eht_term_scale(float scale, double weight) { return (float)((double)scale * weight); }

EHT_HD bool eht_weight_ok(double w) { return w >= 0.0 && w < 1e300; }      // false for a negative, infinite or NaN weight

// the terms of a call as the kernels take them: device pointers and effective scales, 0 / NULL for an absent term
template <int NT>
struct EhtTerms {
    const float *target[NT];
    const float *sigma[NT];
    float scale[NT];
    int present[NT];
};

// `in`: the entry point's term arguments (bhn_cls_term or bhn_pol_term: one layout, two types), NULL for an absent term.  A present
// term must have its arrays and a finite weight >= 0; nothing else can fail, so `a` is filled in the same pass.
template <int NT, typename Term>
static int eht_terms_take(const Term *const (&in)[NT], const char *const (&names)[NT], float scale, EhtTerms<NT> *a) {
    for (int d = 0; d < NT; ++d) {
        const Term *t = in[d];
        if (t) {
            BHN_CHECK_ARG(t->target && t->sigma, "term '%s' with a null target or sigma", names[d]);
            BHN_CHECK_ARG(eht_weight_ok(t->weight), "term '%s': weight %g must be finite and >= 0", names[d], t->weight);
        }
        a->present[d] = t ? 1 : 0;
        a->target[d] = t ? t->target : nullptr;
        a->sigma[d] = t ? t->sigma : nullptr;
        a->scale[d] = t ? eht_term_scale(scale, t->weight) : 0.f;
    }
    return BHN_OK;
}

#if defined(__HIPCC__)
#include "eht_uv_kernels.h"

// loss[1 + d] = the sum of terms[d * stride + i], i < count, in the order of eht_loss_sum_kernel (lane-strided, xor butterfly,
// the waves in order); loss[0] = ((t_0 + t_1) + t_2 ...) in the canonical order
template <int NT>
__global__ __launch_bounds__(256) void eht_terms_sum_kernel(float *__restrict__ loss, const float *__restrict__ terms, int stride, int count) {
    __shared__ float red[NT][4];
    float tot[NT];
#pragma unroll
    for (int d = 0; d < NT; ++d) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < count; i += 256) acc += terms[(size_t)d * stride + i];
        tot[d] = eht_block_sum_256(acc, red[d]);
    }
    if (threadIdx.x == 0) {
        float total = tot[0];
#pragma unroll
        for (int d = 0; d < NT; ++d) {
            loss[1 + d] = tot[d];
            if (d) total += tot[d];
        }
        loss[0] = total;
    }
}
#endif

#endif /* BHNERF_EHT_TERMS_H */
