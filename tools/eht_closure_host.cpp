// CPU build of the plan and the per-element arithmetic of libbhnerf_cls.so (bhnerf_amd/csrc/eht_closure.h on top of eht_uv.h):
// the launches of bhn_cls_chi2 walked one workgroup after the other, as tools/eht_uv_host.cpp walks bhn_eht_chi2_uv's, for
// tests/test_closure_cpu.py to compare with a float64 reference and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/eht_closure_host.cpp -o eht_closure_host
//   eht_closure_host IN OUT
//
// IN:  float64 [N, Sx, nvis, ncp, nca, H, W, present (bit 0 amp, 1 cphase, 2 logcamp), want_grad, psize_x, psize_y, scale,
//               w_amp, w_cphase, w_logcamp], float64 uv[B nvis 2], float32 images[N H W], for each PRESENT term in the canonical
//      order float32 target[N n_d] and sigma[N n_d] (n_d = nvis | ncp | nca), int32 tri[3 ncp], int8 tri_sign[3 ncp], int32 quad[4 nca]
// OUT: float32 vis[2 N nvis] (the visibilities the terms were computed from), float32 loss[4], float32 dimages[N H W] (when want_grad)
// The workspace is one heap block of exactly bhn_cls_ws_bytes' size and every output a block of exactly its documented size, all
// filled with NaN bytes first, so that an index outside them is caught and an element left unwritten shows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "eht_closure.h"
#include "eht_terms.h"

template <typename T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static void forward(const EhtPlan &p, int Sx, const float *images, const double *uv, double psx, double psy, char *ws) {
    EhtC *Eu = reinterpret_cast<EhtC *>(ws + p.off_eu), *Ev = reinterpret_cast<EhtC *>(ws + p.off_ev);
    EhtC *part = reinterpret_cast<EhtC *>(ws + p.off_part);
    const int B = p.N / Sx;
    for (long long bk = 0; bk < (long long)B * p.nvis; ++bk) {                         // eht_twiddle_kernel
        for (int i = 0; i < p.W; ++i) Eu[bk * p.W + i] = eht_twiddle(uv[2 * bk], i, p.W, psx);
        for (int i = 0; i < p.H; ++i) Ev[bk * p.H + i] = eht_twiddle(uv[2 * bk + 1], i, p.H, psy);
    }
    for (int n = 0; n < p.N; ++n)                                                       // eht_fwd_kernel: grid (kblocks, RS, N)
        for (int s = 0; s < p.RS; ++s)
            for (int kb = 0; kb < p.kblocks; ++kb) {
                EhtC acc[EHT_KB];
                for (int j = 0; j < EHT_KB; ++j) acc[j].x = acc[j].y = 0.f;
                for (int x = 0; x < p.W; ++x) {
                    EhtC col[EHT_KB];
                    eht_columns(p, images, Eu, Ev, n, n / Sx, kb * EHT_KB, s, x, col);
                    for (int j = 0; j < EHT_KB; ++j) { acc[j].x += col[j].x; acc[j].y += col[j].y; }
                }
                for (int j = 0; j < EHT_KB && kb * EHT_KB + j < p.nvis; ++j) part[eht_part_index(p, n, kb * EHT_KB + j, s)] = acc[j];
            }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double head[15];
    if (fread(head, sizeof(double), 15, f) != 15) { fprintf(stderr, "short header\n"); return 2; }
    const int32_t N = (int32_t)head[0], Sx = (int32_t)head[1], nvis = (int32_t)head[2], ncp = (int32_t)head[3], nca = (int32_t)head[4],
                  H = (int32_t)head[5], W = (int32_t)head[6], present = (int32_t)head[7], want_grad = (int32_t)head[8];
    const double psx = head[9], psy = head[10];
    const float scale = (float)head[11];
    const bool has[CLS_TERMS] = {(present & 1) != 0, (present & 2) != 0, (present & 4) != 0};
    const char *why = eht_sizes_error(N, Sx, nvis, ncp, H, W, psx, psy);
    ClsPlan p;
    if (why || !cls_make_plan(N, nvis, ncp, nca, H, W, &p) || !(present & 7) || (has[CLS_CPHASE] && ncp < 1) || (has[CLS_LOGCAMP] && nca < 1)) {
        fprintf(stderr, "%s\n", why ? why : "bad sizes or terms");
        return 1;
    }
    float eff[CLS_TERMS];
    for (int d = 0; d < CLS_TERMS; ++d) {
        if (has[d] && !eht_weight_ok(head[12 + d])) { fprintf(stderr, "bad weight\n"); return 1; }
        eff[d] = has[d] ? eht_term_scale(scale, head[12 + d]) : 0.f;
    }
    const size_t count[CLS_TERMS] = {(size_t)N * nvis, (size_t)N * ncp, (size_t)N * nca}, npix = (size_t)N * H * W;
    std::vector<double> uv;
    std::vector<float> images, target[CLS_TERMS], sigma[CLS_TERMS];
    std::vector<int32_t> tri, quad;
    std::vector<int8_t> sign;
    bool ok = read_n(f, uv, (size_t)(N / Sx) * nvis * 2) && read_n(f, images, npix);
    for (int d = 0; d < CLS_TERMS; ++d)
        if (has[d]) ok = ok && read_n(f, target[d], count[d]) && read_n(f, sigma[d], count[d]);
    ok = ok && read_n(f, tri, (size_t)3 * ncp) && read_n(f, sign, (size_t)3 * ncp) && read_n(f, quad, (size_t)4 * nca);
    if (!ok) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    char *ws = (char *)malloc(p.bytes);
    float *loss = (float *)malloc(4 * sizeof(float));
    float *dimages = want_grad ? (float *)malloc(sizeof(float) * npix) : nullptr;
    if (!ws || !loss || (want_grad && !dimages)) return 2;
    memset(ws, 0xFF, p.bytes);
    memset(loss, 0xFF, 4 * sizeof(float));
    if (dimages) memset(dimages, 0xFF, sizeof(float) * npix);

    EhtC *vis = reinterpret_cast<EhtC *>(ws + p.e.off_vis), *gva = reinterpret_cast<EhtC *>(ws + p.off_gva);
    EhtC *gv = reinterpret_cast<EhtC *>(ws + p.off_gv);
    float *dphi = reinterpret_cast<float *>(ws + p.e.off_dphi), *dy = reinterpret_cast<float *>(ws + p.off_dy);
    float *terms = reinterpret_cast<float *>(ws + p.off_terms);
    forward(p.e, Sx, images.data(), uv.data(), psx, psy, ws);
    const EhtC *part = reinterpret_cast<const EhtC *>(ws + p.e.off_part);
    const bool amp_only = has[CLS_AMP] && !has[CLS_CPHASE] && !has[CLS_LOGCAMP];
    for (int n = 0; n < N; ++n) {                                                       // cls_loss_kernel: one workgroup per plane
        float tot[CLS_TERMS] = {0.f, 0.f, 0.f};
        const EhtC *vis_n = vis + (size_t)n * nvis;
        for (int k = 0; k < nvis; ++k) {
            const size_t t = (size_t)n * nvis + k;
            const EhtC v = eht_combine(p.e, part, n, k);
            vis[t] = v;
            if (has[CLS_AMP]) {
                EhtC g;
                tot[CLS_AMP] += eht_term_amp(v, target[CLS_AMP][t], sigma[CLS_AMP][t], eff[CLS_AMP], &g);
                if (want_grad) (amp_only ? gv : gva)[t] = g;
            }
        }
        if (has[CLS_CPHASE])
            for (int c = 0; c < ncp; ++c) {
                const size_t t = (size_t)n * ncp + c;
                tot[CLS_CPHASE] += eht_term_cphase(vis_n, nvis, tri.data(), sign.data(), c, target[CLS_CPHASE][t], sigma[CLS_CPHASE][t],
                                                   eff[CLS_CPHASE], &dphi[t]);
            }
        if (has[CLS_LOGCAMP])
            for (int q = 0; q < nca; ++q) {
                const size_t t = (size_t)n * nca + q;
                tot[CLS_LOGCAMP] += cls_term_logcamp(vis_n, nvis, quad.data(), q, target[CLS_LOGCAMP][t], sigma[CLS_LOGCAMP][t], eff[CLS_LOGCAMP],
                                                     &dy[t]);
            }
        for (int d = 0; d < CLS_TERMS; ++d) terms[(size_t)d * N + n] = eff[d] * tot[d];
    }
    for (int d = 0; d < CLS_TERMS; ++d) {                                               // eht_terms_sum_kernel
        float tot = 0.f;
        for (int n = 0; n < N; ++n) tot += terms[(size_t)d * N + n];
        loss[1 + d] = tot;
    }
    loss[0] = (loss[1] + loss[2]) + loss[3];
    if (want_grad) {
        if (!amp_only)
            for (int t = 0; t < N * nvis; ++t) {                                        // cls_gather_kernel
                const int n = t / nvis, k = t % nvis;
                EhtC g = {0.f, 0.f};
                bool first = true;
                if (has[CLS_AMP]) { g = gva[t]; first = false; }
                if (has[CLS_CPHASE]) {
                    g = cls_add_gv(first, g, eht_gather_gv(vis[t], eht_gather_weight(k, tri.data(), sign.data(), dphi + (size_t)n * ncp, ncp, 0, 1)));
                    first = false;
                }
                if (has[CLS_LOGCAMP])
                    g = cls_add_gv(first, g, cls_gather_gv(vis[t], cls_gather_weight(k, quad.data(), dy + (size_t)n * nca, nca, 0, 1)));
                gv[t] = g;
            }
        const EhtC *Eu = reinterpret_cast<const EhtC *>(ws + p.e.off_eu), *Ev = reinterpret_cast<const EhtC *>(ws + p.e.off_ev);
        for (int n = 0; n < N; ++n)                                                     // eht_adjoint_kernel: grid (., strips, N)
            for (int y0 = 0; y0 < H; y0 += EHT_ADJ_ROWS)
                for (int x = 0; x < W; ++x) {
                    float acc[EHT_ADJ_ROWS] = {0.f};
                    for (int k = 0; k < nvis; ++k) {
                        const EhtC z = eht_adjoint_z(gv[(size_t)n * nvis + k], Eu[eht_eu_index(p.e, n / Sx, k, x)]);
                        for (int r = 0; r < EHT_ADJ_ROWS; ++r) {
                            const int y = y0 + r < H ? y0 + r : H - 1;
                            acc[r] = eht_adjoint_mac(acc[r], z, Ev[eht_ev_index(p.e, n / Sx, k, y)]);
                        }
                    }
                    for (int r = 0; r < EHT_ADJ_ROWS && y0 + r < H; ++r) dimages[((size_t)n * H + y0 + r) * W + x] = acc[r];
                }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = fwrite(vis, sizeof(EhtC), (size_t)N * nvis, o) == (size_t)N * nvis && fwrite(loss, sizeof(float), 4, o) == 4;
    if (want_grad) ok = ok && fwrite(dimages, sizeof(float), npix, o) == npix;
    ok = (fclose(o) == 0) && ok;
    free(ws); free(loss); free(dimages);
    return ok ? 0 : 2;
}
