// CPU build of the plan and the per-element arithmetic of libbhnerf_eht.so (bhnerf_amd/csrc/eht_uv.h): the launches of
// bhn_eht_vis / bhn_eht_chi2_uv walked one workgroup after the other, for tests/test_eht_uv_cpu.py to compare with a float64
// reference and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/eht_uv_host.cpp -o eht_uv_host
//   eht_uv_host IN OUT
//
// IN:  float64 [N, Sx, nvis, ncp, H, W, dtype, want_grad, psize_x, psize_y, scale], float64 uv[B nvis 2], float32 images[N H W],
//      float32 target[2 N nvis | N nvis | N ncp], float32 sigma[N nvis | N ncp], int32 tri[3 ncp], int8 tri_sign[3 ncp]
// OUT: float32 vis[2 N nvis] (what bhn_eht_vis writes), float32 loss[1], float32 dimages[N H W] (when want_grad)
// The workspace is one heap block of exactly bhn_eht_ws_bytes' size and every output a block of exactly its documented size, all
// filled with NaN bytes first, so that an index outside them is caught and an element left unwritten shows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "eht_uv.h"

template <typename T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static void forward(const EhtPlan &p, int Sx, const float *images, const double *uv, double psx, double psy, char *ws, EhtC *vis) {
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
    if (!vis) return;
    for (int t = 0; t < p.N * p.nvis; ++t) vis[t] = eht_combine(p, part, t / p.nvis, t % p.nvis);      // eht_combine_kernel
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double head[11];
    if (fread(head, sizeof(double), 11, f) != 11) { fprintf(stderr, "short header\n"); return 2; }
    const int32_t N = (int32_t)head[0], Sx = (int32_t)head[1], nvis = (int32_t)head[2], ncp = (int32_t)head[3], H = (int32_t)head[4],
                  W = (int32_t)head[5], dtype = (int32_t)head[6], want_grad = (int32_t)head[7];
    const double psx = head[8], psy = head[9];
    const float scale = (float)head[10];
    const char *why = eht_sizes_error(N, Sx, nvis, ncp, H, W, psx, psy);
    EhtPlan p;
    if (why || !eht_make_plan(N, nvis, ncp, H, W, &p) || dtype < 0 || dtype > 2 || (dtype == EHT_DTYPE_CPHASE && ncp < 1)) {
        fprintf(stderr, "%s\n", why ? why : "bad sizes or dtype");
        return 1;
    }
    const size_t nterm = (size_t)N * (dtype == EHT_DTYPE_CPHASE ? ncp : nvis), npix = (size_t)N * H * W;
    std::vector<double> uv;
    std::vector<float> images, target, sigma;
    std::vector<int32_t> tri;
    std::vector<int8_t> sign;
    if (!read_n(f, uv, (size_t)(N / Sx) * nvis * 2) || !read_n(f, images, npix) || !read_n(f, target, nterm * (dtype == EHT_DTYPE_VIS ? 2 : 1)) ||
        !read_n(f, sigma, nterm) || !read_n(f, tri, (size_t)3 * ncp) || !read_n(f, sign, (size_t)3 * ncp)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    char *ws = (char *)malloc(p.bytes);
    EhtC *vis_out = (EhtC *)malloc(sizeof(EhtC) * (size_t)N * nvis);
    float *loss = (float *)malloc(sizeof(float));
    float *dimages = want_grad ? (float *)malloc(sizeof(float) * npix) : nullptr;
    if (!ws || !vis_out || !loss || (want_grad && !dimages)) return 2;
    memset(ws, 0xFF, p.bytes);
    memset(vis_out, 0xFF, sizeof(EhtC) * (size_t)N * nvis);
    memset(loss, 0xFF, sizeof(float));
    if (dimages) memset(dimages, 0xFF, sizeof(float) * npix);

    forward(p, Sx, images.data(), uv.data(), psx, psy, ws, vis_out);                    // bhn_eht_vis
    memset(ws, 0xFF, p.bytes);                                                          // bhn_eht_chi2_uv relies on nothing left there
    EhtC *vis = reinterpret_cast<EhtC *>(ws + p.off_vis);
    float *dphi = reinterpret_cast<float *>(ws + p.off_dphi), *loss_part = reinterpret_cast<float *>(ws + p.off_loss);
    forward(p, Sx, images.data(), uv.data(), psx, psy, ws, nullptr);
    const EhtC *part = reinterpret_cast<const EhtC *>(ws + p.off_part);
    for (int n = 0; n < N; ++n) {                                                       // eht_loss_kernel: one workgroup per plane
        float tot = 0.f;
        for (int k = 0; k < nvis; ++k) {
            const size_t t = (size_t)n * nvis + k;
            const EhtC v = eht_combine(p, part, n, k);
            EhtC gv = v;
            if (dtype == EHT_DTYPE_VIS) tot += eht_term_vis(v, target[2 * t], target[2 * t + 1], sigma[t], scale, &gv);
            else if (dtype == EHT_DTYPE_AMP) tot += eht_term_amp(v, target[t], sigma[t], scale, &gv);
            vis[t] = (want_grad || dtype == EHT_DTYPE_CPHASE) ? gv : v;
        }
        if (dtype == EHT_DTYPE_CPHASE)
            for (int c = 0; c < ncp; ++c) {
                const size_t t = (size_t)n * ncp + c;
                tot += eht_term_cphase(vis + (size_t)n * nvis, nvis, tri.data(), sign.data(), c, target[t], sigma[t], scale, &dphi[t]);
            }
        loss_part[n] = scale * tot;
    }
    float tot = 0.f;
    for (int n = 0; n < N; ++n) tot += loss_part[n];                                    // eht_loss_sum_kernel
    loss[0] = tot;
    if (want_grad) {
        if (dtype == EHT_DTYPE_CPHASE)                                                  // eht_gather_kernel
            for (int t = 0; t < N * nvis; ++t)
                vis[t] = eht_gather_gv(vis[t], eht_gather_weight(t % nvis, tri.data(), sign.data(), dphi + (size_t)(t / nvis) * ncp, ncp, 0, 1));
        const EhtC *Eu = reinterpret_cast<const EhtC *>(ws + p.off_eu), *Ev = reinterpret_cast<const EhtC *>(ws + p.off_ev);
        for (int n = 0; n < N; ++n)                                                     // eht_adjoint_kernel: grid (., strips, N)
            for (int y0 = 0; y0 < H; y0 += EHT_ADJ_ROWS)
                for (int x = 0; x < W; ++x) {
                    float acc[EHT_ADJ_ROWS] = {0.f};
                    for (int k = 0; k < nvis; ++k) {
                        const EhtC z = eht_adjoint_z(vis[(size_t)n * nvis + k], Eu[eht_eu_index(p, n / Sx, k, x)]);
                        for (int r = 0; r < EHT_ADJ_ROWS; ++r) {
                            const int y = y0 + r < H ? y0 + r : H - 1;
                            acc[r] = eht_adjoint_mac(acc[r], z, Ev[eht_ev_index(p, n / Sx, k, y)]);
                        }
                    }
                    for (int r = 0; r < EHT_ADJ_ROWS && y0 + r < H; ++r) dimages[((size_t)n * H + y0 + r) * W + x] = acc[r];
                }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(vis_out, sizeof(EhtC), (size_t)N * nvis, o) == (size_t)N * nvis && fwrite(loss, sizeof(float), 1, o) == 1;
    if (want_grad) ok = ok && fwrite(dimages, sizeof(float), npix, o) == npix;
    ok = (fclose(o) == 0) && ok;
    free(ws); free(vis_out); free(loss); free(dimages);
    return ok ? 0 : 2;
}
