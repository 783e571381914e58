// CPU build of the per-point code of libbhnerf_grf.so (bhnerf_amd/csrc/gr_factors.h): the arithmetic the device runs, walked launch by
// launch and workgroup by workgroup (the two stages of the domain mean included), for tests/test_gr_factors_cpu.py to compare with
// the NumPy functions of bhnerf_amd/kgeo.py and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/gr_factors_host.cpp -o gr_factors_host
//   gr_factors_host IN OUT
//
// IN:  float64 [n, ngeo, spin, M, E, inc, fillna, fill, arad, avert, ator, z_width, rmin, rmax, normalise, Q_frac, V_frac, spectral_index],
//      then r, theta, affine, Delta, Sigma, Xi, R, Theta, Omega (n ngeo each), then lam, alpha, beta (n each)
// OUT: float64 g[n ngeo], b[n ngeo 3], mean[1], J[S n ngeo] with S = 3, or 4 when V_frac != 0  (the layouts of include/bhnerf_grf.h);
//      with normalise = 0 the mean is still computed and written, but b is not divided by it
// Inputs, outputs and the workspace are separate heap blocks of exactly the documented size, so that an index outside them is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gr_factors.h"

#define HEAD 18

static double *block(size_t count, int fill) {
    double *p = (double *)malloc(sizeof(double) * (count ? count : 1));
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, fill, sizeof(double) * count);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double head[HEAD];
    if (fread(head, sizeof(double), HEAD, f) != HEAD) { fprintf(stderr, "short header\n"); return 2; }
    const long long n = (long long)head[0];
    const int ngeo = (int)head[1];
    if (n < 1 || n > (1LL << 24) || ngeo < 0 || ngeo > (1 << 16)) { fprintf(stderr, "bad sizes\n"); return 2; }
    const size_t total = (size_t)n * ngeo;
    double *pt[9], *ray[3];
    for (int i = 0; i < 9; ++i) {
        pt[i] = block(total, 0);
        if (fread(pt[i], sizeof(double), total, f) != total) { fprintf(stderr, "short point field %d\n", i); return 2; }
    }
    for (int i = 0; i < 3; ++i) {
        ray[i] = block((size_t)n, 0);
        if (fread(ray[i], sizeof(double), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short ray field %d\n", i); return 2; }
    }
    fclose(f);
    GrfGeos g;
    g.n = n; g.ngeo = ngeo;
    g.r = pt[0]; g.theta = pt[1]; g.affine = pt[2]; g.Delta = pt[3]; g.Sigma = pt[4]; g.Xi = pt[5]; g.R = pt[6]; g.Theta = pt[7];
    const double *Omega = pt[8];
    g.lam = ray[0]; g.alpha = ray[1]; g.beta = ray[2];
    g.a = head[2]; g.M = head[3]; g.E = head[4]; g.sin_inc = sin(head[5]);
    const double fillna = head[6];
    const int fill = head[7] != 0.0;
    const double arad = head[8], avert = head[9], ator = head[10], z_width = head[11], rmin = head[12], rmax = head[13];
    const int normalise = head[14] != 0.0;
    const double Q_frac = head[15], V_frac = head[16], spectral_index = head[17];
    const char *why = grf_geos_error(g);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    if (Q_frac > 1.0 || Q_frac < 0.0) { fprintf(stderr, "Q_frac should be in [0,1]\n"); return 1; }
    const int with_v = V_frac != 0.0, S = with_v ? 4 : 3;
    const long long blocks = ((long long)total + GRF_BLOCK - 1) / GRF_BLOCK;

    double *gfac = block(total, 0xFF), *b = block(3 * total, 0xFF), *mean = block(1, 0xFF), *J = block((size_t)S * total, 0xFF);
    double *ws = block((size_t)blocks * 2, 0xFF);            // bhn_grf_ws_bytes(n, ngeo)
    double *partial = ws, *count = ws + blocks;

    // bhn_grf_doppler, bhn_grf_fluid_field
    for (long long blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < GRF_BLOCK; ++t) {
            const long long p = blk * GRF_BLOCK + t;
            if (p >= (long long)total) continue;
            gfac[p] = grf_point_doppler(g, p, Omega[p], fillna, fill);
        }
    for (long long blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < GRF_BLOCK; ++t) {
            const long long p = blk * GRF_BLOCK + t;
            if (p >= (long long)total) continue;
            grf_point_fluid_field(g, p, Omega[p], arad, avert, ator, b + 3 * p);
        }
    // bhn_grf_domain_mean: stage 1 per workgroup, stage 2 in one workgroup
    for (long long blk = 0; blk < blocks; ++blk) {
        double s_sum[GRF_BLOCK], s_cnt[GRF_BLOCK];
        for (int t = 0; t < GRF_BLOCK; ++t) {
            const long long p = blk * GRF_BLOCK + t;
            const bool in = p < (long long)total && grf_in_domain(g, p, z_width, rmin, rmax);
            s_sum[t] = in ? grf_field_magnitude(b + 3 * p) : 0.0;
            s_cnt[t] = in ? 1.0 : 0.0;
        }
        partial[blk] = grf_tree_sum_host(s_sum);
        count[blk] = grf_tree_sum_host(s_cnt);
    }
    {
        double s_sum[GRF_BLOCK], s_cnt[GRF_BLOCK];
        for (int t = 0; t < GRF_BLOCK; ++t) {
            double s = 0.0, c = 0.0;
            for (long long i = t; i < blocks; i += GRF_BLOCK) {
                s += partial[i];
                c += count[i];
            }
            s_sum[t] = s;
            s_cnt[t] = c;
        }
        const double s = grf_tree_sum_host(s_sum), c = grf_tree_sum_host(s_cnt);
        mean[0] = s / c;
    }
    // bhn_grf_transport
    for (long long blk = 0; blk < blocks; ++blk)
        for (int t = 0; t < GRF_BLOCK; ++t) {
            const long long p = blk * GRF_BLOCK + t;
            if (p >= (long long)total) continue;
            double v[3] = {b[3 * p], b[3 * p + 1], b[3 * p + 2]}, out[4];
            if (normalise)
                for (int i = 0; i < 3; ++i) v[i] = v[i] / mean[0];
            grf_point_transport(g, p, Omega[p], gfac[p], v, Q_frac, V_frac, spectral_index, with_v, out);
            for (int s = 0; s < S; ++s) J[(size_t)s * total + p] = out[s];
        }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(gfac, sizeof(double), total, o) == total && fwrite(b, sizeof(double), 3 * total, o) == 3 * total &&
              fwrite(mean, sizeof(double), 1, o) == 1 && fwrite(J, sizeof(double), (size_t)S * total, o) == (size_t)S * total;
    ok = (fclose(o) == 0) && ok;
    for (int i = 0; i < 9; ++i) free(pt[i]);
    for (int i = 0; i < 3; ++i) free(ray[i]);
    free(gfac); free(b); free(mean); free(J); free(ws);
    return ok ? 0 : 2;
}
