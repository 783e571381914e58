// CPU build of the plan and the per-element arithmetic of libbhnerf_pol.so (bhnerf_amd/csrc/eht_pol.h on top of eht_uv.h): the
// launches of bhn_pol_chi2 walked one workgroup after the other, as tools/eht_closure_host.cpp walks bhn_cls_chi2's, for
// tests/test_pol_cpu.py to compare with a float64 reference and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/eht_pol_host.cpp -o eht_pol_host
//   eht_pol_host IN OUT
//
// IN:  float64 [N, Sx, nvis, H, W, present (bit 0 pvis, 1 m), want_grad, psize_x, psize_y, scale, w_pvis, w_m], float64 uv[B nvis 2],
//      float32 images[N H W], for each PRESENT term in the canonical order float32 target[2 B nvis] (re, im pairs) and sigma[B nvis]
// OUT: float32 vis[2 N nvis] (the visibilities the terms were computed from), float32 loss[3], float32 dimages[N H W] (when want_grad)
// The workspace is one heap block of exactly bhn_pol_ws_bytes' size and every output a block of exactly its documented size, all
// filled with NaN bytes first, so that an index outside them is caught and an element left unwritten shows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "eht_pol.h"
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
    double head[12];
    if (fread(head, sizeof(double), 12, f) != 12) { fprintf(stderr, "short header\n"); return 2; }
    const int32_t N = (int32_t)head[0], Sx = (int32_t)head[1], nvis = (int32_t)head[2], H = (int32_t)head[3], W = (int32_t)head[4],
                  present = (int32_t)head[5], want_grad = (int32_t)head[6];
    const double psx = head[7], psy = head[8];
    const float scale = (float)head[9];
    const bool has[POL_TERMS] = {(present & 1) != 0, (present & 2) != 0};
    const char *why = eht_sizes_error(N, Sx, nvis, 0, H, W, psx, psy);
    PolPlan p;
    if (why || !pol_stokes_ok(Sx) || !pol_make_plan(N, nvis, H, W, &p) || !(present & 3)) {
        fprintf(stderr, "%s\n", why ? why : "bad sizes, Sx or terms");
        return 1;
    }
    float eff[POL_TERMS];
    for (int d = 0; d < POL_TERMS; ++d) {
        if (has[d] && !eht_weight_ok(head[10 + d])) { fprintf(stderr, "bad weight\n"); return 1; }
        eff[d] = has[d] ? eht_term_scale(scale, head[10 + d]) : 0.f;
    }
    const int B = N / Sx;
    const size_t count = (size_t)B * nvis, npix = (size_t)N * H * W;
    std::vector<double> uv;
    std::vector<float> images, target[POL_TERMS], sigma[POL_TERMS];
    bool ok = read_n(f, uv, count * 2) && read_n(f, images, npix);
    for (int d = 0; d < POL_TERMS; ++d)
        if (has[d]) ok = ok && read_n(f, target[d], 2 * count) && read_n(f, sigma[d], count);
    if (!ok) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    char *ws = (char *)malloc(p.bytes);
    float *loss = (float *)malloc(3 * sizeof(float));
    float *dimages = want_grad ? (float *)malloc(sizeof(float) * npix) : nullptr;
    if (!ws || !loss || (want_grad && !dimages)) return 2;
    memset(ws, 0xFF, p.bytes);
    memset(loss, 0xFF, 3 * sizeof(float));
    if (dimages) memset(dimages, 0xFF, sizeof(float) * npix);

    EhtC *vis = reinterpret_cast<EhtC *>(ws + p.e.off_vis), *gv = reinterpret_cast<EhtC *>(ws + p.off_gv);
    float *terms = reinterpret_cast<float *>(ws + p.off_terms);
    forward(p.e, Sx, images.data(), uv.data(), psx, psy, ws);
    const EhtC *part = reinterpret_cast<const EhtC *>(ws + p.e.off_part);
    for (int b = 0; b < B; ++b) {                                                       // pol_loss_kernel: one workgroup per frame
        float tot[POL_TERMS] = {0.f, 0.f};
        const int n0 = b * Sx;
        for (int k = 0; k < nvis; ++k) {
            EhtC v[4];
            for (int s = 0; s < Sx; ++s) {
                v[s] = eht_combine(p.e, part, n0 + s, k);
                vis[(size_t)(n0 + s) * nvis + k] = v[s];
            }
            const size_t t = (size_t)b * nvis + k;
            float tp, tm;
            EhtC g[3];
            pol_baseline(v[0], v[1], v[2], has[POL_PVIS], has[POL_PVIS] ? target[POL_PVIS].data() + 2 * t : nullptr,
                         has[POL_PVIS] ? sigma[POL_PVIS][t] : 1.f, eff[POL_PVIS], has[POL_M], has[POL_M] ? target[POL_M].data() + 2 * t : nullptr,
                         has[POL_M] ? sigma[POL_M][t] : 1.f, eff[POL_M], &tp, &tm, g);
            tot[POL_PVIS] += tp;
            tot[POL_M] += tm;
            if (want_grad) {
                for (int s = 0; s < 3; ++s) gv[(size_t)(n0 + s) * nvis + k] = g[s];
                if (Sx == 4) gv[(size_t)(n0 + 3) * nvis + k] = EhtC{0.f, 0.f};
            }
        }
        for (int d = 0; d < POL_TERMS; ++d) terms[(size_t)d * N + b] = eff[d] * tot[d];
    }
    for (int d = 0; d < POL_TERMS; ++d) {                                               // eht_terms_sum_kernel
        float tot = 0.f;
        for (int b = 0; b < B; ++b) tot += terms[(size_t)d * N + b];
        loss[1 + d] = tot;
    }
    loss[0] = loss[1] + loss[2];
    if (want_grad) {
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
    ok = fwrite(vis, sizeof(EhtC), (size_t)N * nvis, o) == (size_t)N * nvis && fwrite(loss, sizeof(float), 3, o) == 3;
    if (want_grad) ok = ok && fwrite(dimages, sizeof(float), npix, o) == npix;
    ok = (fclose(o) == 0) && ok;
    free(ws); free(loss); free(dimages);
    return ok ? 0 : 2;
}
