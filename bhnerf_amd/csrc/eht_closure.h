// The combined closure loss from (u, v) coordinates (libbhnerf_cls.so, include/bhnerf_cls.h): the plan and the per-element
// arithmetic it adds to csrc/eht_uv.h, without HIP dependencies.  csrc/eht_closure.hip runs this code on the device;
// tools/eht_closure_host.cpp compiles the same header with a plain C++ compiler and walks the same plan (tests/test_closure_cpu.py).
//
// One visibility pass serves up to three real-valued terms, in the canonical order amp, cphase, logcamp:
//     loss = scale (w_amp chi^2_amp + w_cphase chi^2_cphase + w_logcamp chi^2_logcamp).
// 'amp' and 'cphase' are eht_term_amp / eht_term_cphase / eht_gather_weight / eht_gather_gv of eht_uv.h unchanged, handed the
// term's effective scale (eht_term_scale, csrc/eht_terms.h).  'logcamp' is the log closure amplitude of a quadrangle of baselines (legs 0, 1 over legs 2, 3):
//     y = 1/2 (log m_0 + log m_1 - log m_2 - log m_3),  m_l = |V_l|^2,   term ((y - target) / sigma)^2.
// |V_ab| = |V_ba|: the table needs no signs.
#ifndef BHNERF_EHT_CLOSURE_H
#define BHNERF_EHT_CLOSURE_H

#include "eht_uv.h"

#define CLS_AMP 0                 // the canonical order of the terms: loss[1 + d], the order gv and the total are added in
#define CLS_CPHASE 1
#define CLS_LOGCAMP 2
#define CLS_TERMS 3

// ---------------------------------------------------------------------------------------------------------------------------
// The plan: the (u, v) library's (twiddle tables, partial sums, V at off_vis, dphi at off_dphi -- its row split, so V is bitwise
// bhn_eht_vis') and behind it the buffers of this library.  Like EhtPlan it never makes a plane's arithmetic depend on the batch.
// ---------------------------------------------------------------------------------------------------------------------------
struct ClsPlan {
    EhtPlan e;
    int32_t nca;
    // workspace offsets in bytes, each a multiple of 256
    size_t off_gva;               // (N, nvis) complex64: gv of the 'amp' term (V itself is kept: the closure terms read it)
    size_t off_gv;                // (N, nvis) complex64: gv_amp + gv_cphase + gv_logcamp, what the adjoint reads
    size_t off_dy;                // (N, nca) float32: dL/dy of each quadrangle
    size_t off_terms;             // (CLS_TERMS, N) float32: the planes' scaled sums of each term
    size_t bytes;
};

// false when a size is below 1 (ncp and nca may be 0: no table) or the sizes do not fit the 32-bit launch geometry
EHT_HD bool cls_make_plan(int32_t N, int32_t nvis, int32_t ncp, int32_t nca, int32_t H, int32_t W, ClsPlan *p) {
    if (nca < 0 || !eht_make_plan(N, nvis, ncp, H, W, &p->e)) return false;
    if ((int64_t)N * nca > 0x3fffffff || nca > 0x1fffffff) return false;
    p->nca = nca;
    size_t o = p->e.bytes;
    p->off_gva = o;   o += eht_align256(sizeof(EhtC) * (size_t)N * nvis);
    p->off_gv = o;    o += eht_align256(sizeof(EhtC) * (size_t)N * nvis);
    p->off_dy = o;    o += eht_align256(sizeof(float) * (size_t)N * nca);
    p->off_terms = o; o += eht_align256(sizeof(float) * (size_t)CLS_TERMS * N);
    p->bytes = o;
    return true;
}

// Log closure amplitude of quadrangle q of plane n from the table; *dy = dL/dy = 2 scale d / sigma.  A leg of zero amplitude
// takes the quadrangle out of the loss and of the gradient (the rule of the zero gradient at |vis| = 0, extended: frames before
// the injection render exactly zero images).  A table index outside [0, nvis) is clamped as in eht_term_cphase.
EHT_HD float cls_term_logcamp(const EhtC *vis_n, int nvis, const int32_t *quad, int q, float target, float s, float scale, float *dy) {
    float m[4];
    bool zero = false;
    for (int l = 0; l < 4; ++l) {
        const int32_t k = quad[4 * q + l];
        const EhtC v = vis_n[k < 0 ? 0 : (k >= nvis ? nvis - 1 : k)];
        m[l] = v.x * v.x + v.y * v.y;
        zero = zero || m[l] == 0.f;
    }
    if (zero) {
        *dy = 0.f;
        return 0.f;
    }
    const float y = 0.5f * (logf(m[0]) + logf(m[1]) - logf(m[2]) - logf(m[3]));
    const float d = (y - target) / s;
    *dy = 2.f * scale * d / s;
    return d * d;
}

// Gradient of baseline k of one plane from the quadrangles it sits in, GATHERED in table order like eht_gather_weight:
// w_k = sum_{legs (q, l) on k} s_l dy_q with s = +1 for the numerator (legs 0, 1) and -1 for the denominator; the table entries
// j0, j0 + stride, ...  Then gv_k = w_k (Re V_k, Im V_k) / |V_k|^2, zero at |V_k| = 0.
EHT_HD float cls_gather_weight(int k, const int32_t *quad, const float *dy_n, int nca, int j0, int stride) {
    float w = 0.f;
    for (int j = j0; j < 4 * nca; j += stride)
        if (quad[j] == k) w += ((j & 3) < 2 ? 1.f : -1.f) * dy_n[j >> 2];
    return w;
}

EHT_HD EhtC cls_gather_gv(EhtC v, float w) {
    const float m2 = v.x * v.x + v.y * v.y;
    EhtC g = {0.f, 0.f};
    if (m2 > 0.f) {
        g.x = w * v.x / m2;
        g.y = w * v.y / m2;
    }
    return g;
}

// gv_k = gv_amp + gv_cphase + gv_logcamp, the present terms in that order
EHT_HD EhtC cls_add_gv(bool first, EhtC sum, EhtC g) {
    if (first) return g;
    sum.x += g.x;
    sum.y += g.y;
    return sum;
}

#endif /* BHNERF_EHT_CLOSURE_H */
