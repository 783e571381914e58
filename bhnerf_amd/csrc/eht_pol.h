// The polarimetric EHT losses from (u, v) coordinates (libbhnerf_pol.so, include/bhnerf_pol.h): the plan and the per-element
// arithmetic they add to csrc/eht_uv.h, without HIP dependencies.  csrc/eht_pol.hip runs this code on the device;
// tools/eht_pol_host.cpp compiles the same header with a plain C++ compiler and walks the same plan (tests/test_pol_cpu.py).
//
// The terms couple the Stokes planes of a frame.  With V_s = V[b Sx + s, k] the visibility of plane s (I, Q, U[, V]) of frame b
// on baseline k and P = V_1 + i V_2 the polarised visibility, in the canonical order pvis, m:
//     pvis   |P - target|^2 / sigma^2               the calibrated term
//     m      |P / V_0 - target|^2 / sigma^2         the visibility-domain fractional polarisation: a complex gain common to the
//                                                   planes of a baseline multiplies P and V_0 alike and cancels
//     loss = scale (w_pvis chi^2_pvis + w_m chi^2_m).
// P and P / V_0 are holomorphic in the visibilities, so with g_f = dL/dRe f + i dL/dIm f (the adjoint's convention):
//     g_P = g_pvis + g_m / conj(V_0),   gv_1 = g_P,   gv_2 = -i g_P,   gv_0 = -g_m conj(m) / conj(V_0),   gv_3 = 0.
#ifndef BHNERF_EHT_POL_H
#define BHNERF_EHT_POL_H

#include "eht_uv.h"

#define POL_PVIS 0                // the canonical order of the terms: loss[1 + d], the order gv and the total are added in
#define POL_M 1
#define POL_TERMS 2

// ---------------------------------------------------------------------------------------------------------------------------
// The plan: the (u, v) library's without triangles (twiddle tables, partial sums, V at off_vis -- its row split, so V is bitwise
// bhn_eht_vis') and behind it the buffers of this library.  A frame's arithmetic never depends on the frames computed with it.
// ---------------------------------------------------------------------------------------------------------------------------
struct PolPlan {
    EhtPlan e;
    // workspace offsets in bytes, each a multiple of 256
    size_t off_gv;                // (N, nvis) complex64: gv of every plane, what the adjoint reads
    size_t off_terms;             // (POL_TERMS, N) float32: the frames' scaled sums of each term in the first B of each row
    size_t bytes;
};

// false when a size is below 1 or the sizes do not fit the 32-bit launch geometry
EHT_HD bool pol_make_plan(int32_t N, int32_t nvis, int32_t H, int32_t W, PolPlan *p) {
    if (!eht_make_plan(N, nvis, 0, H, W, &p->e)) return false;
    size_t o = p->e.bytes;
    p->off_gv = o;    o += eht_align256(sizeof(EhtC) * (size_t)N * nvis);
    p->off_terms = o; o += eht_align256(sizeof(float) * (size_t)POL_TERMS * N);
    p->bytes = o;
    return true;
}

EHT_HD bool pol_stokes_ok(int32_t Sx) { return Sx == 3 || Sx == 4; }

// P = Q + i U of the complex visibilities of the Q and the U plane
EHT_HD EhtC pol_p(EhtC q, EhtC u) {
    EhtC p;
    p.x = q.x - u.y;
    p.y = q.y + u.x;
    return p;
}

// One baseline of one frame: both terms from the visibilities (v0, v1, v2) of the planes I, Q, U.  target: a complex64 as a float
// pair.  *term_d is unscaled (the caller multiplies the block sum by the effective scale); the derivatives carry it.  An absent
// term (has_d false) leaves *term_d = 0 and adds nothing; 'm' on a baseline with V_0 == 0 adds 0 to the loss and nothing to the
// gradient (the rule of a zero leg of cls_term_logcamp).  gv[0..2]: the gradient of the planes I, Q, U.
EHT_HD void pol_baseline(EhtC v0, EhtC v1, EhtC v2, bool has_p, const float *tp, float sp, float scale_p, bool has_m, const float *tm,
                         float sm, float scale_m, float *term_p, float *term_m, EhtC gv[3]) {
    const EhtC P = pol_p(v1, v2);
    EhtC gP = {0.f, 0.f}, g0 = {0.f, 0.f};
    *term_p = *term_m = 0.f;
    if (has_p) *term_p = eht_term_vis(P, tp[0], tp[1], sp, scale_p, &gP);
    const float a2 = v0.x * v0.x + v0.y * v0.y;
    if (has_m && a2 > 0.f) {
        EhtC m, gm, gPm;
        m.x = (P.x * v0.x + P.y * v0.y) / a2;             // P conj(V_0) / |V_0|^2
        m.y = (P.y * v0.x - P.x * v0.y) / a2;
        *term_m = eht_term_vis(m, tm[0], tm[1], sm, scale_m, &gm);
        gPm.x = (gm.x * v0.x - gm.y * v0.y) / a2;         // g_m / conj(V_0) = g_m V_0 / |V_0|^2
        gPm.y = (gm.x * v0.y + gm.y * v0.x) / a2;
        g0.x = -(gPm.x * m.x + gPm.y * m.y);              // -g_P conj(m)
        g0.y = -(gPm.y * m.x - gPm.x * m.y);
        if (has_p) {
            gP.x += gPm.x;
            gP.y += gPm.y;
        } else {
            gP = gPm;
        }
    }
    gv[0] = g0;
    gv[1] = gP;
    gv[2].x = gP.y;                                       // -i g_P
    gv[2].y = -gP.x;
}

#endif /* BHNERF_EHT_POL_H */
