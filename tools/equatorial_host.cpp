// CPU build of the per-ray code of bhn_eql_crossings (bhnerf_amd/csrc/equatorial.h): the arithmetic the device runs, one ray after
// the other, for tests/test_equatorial_cpu.py to compare with geodesics._integrate_crossings and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/equatorial_host.cpp -o equatorial_host
//   equatorial_host IN OUT
//
// IN:  float64 [n, nmax, max_steps, spin, inclination, distance, M, h, r_c, alpha[n], beta[n]]
// OUT: float64 cross[7 n nmax], int32 count[n], int32 status[n]  (the layouts of include/bhnerf_eql.h)
// The three outputs are separate heap blocks of exactly the documented size, so that an index outside them is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "equatorial.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double head[9];
    if (fread(head, sizeof(double), 9, f) != 9) { fprintf(stderr, "short header\n"); return 2; }
    const int64_t n = (int64_t)head[0];
    const int32_t nmax = (int32_t)head[1], max_steps = (int32_t)head[2];
    if (n < 1 || n > (int64_t)1 << 24 || nmax > 1 << 16) { fprintf(stderr, "bad ray or crossing count\n"); return 2; }
    std::vector<double> alpha(n), beta(n);
    if (fread(alpha.data(), sizeof(double), n, f) != (size_t)n || fread(beta.data(), sizeof(double), n, f) != (size_t)n) {
        fprintf(stderr, "short ray list\n");
        return 2;
    }
    fclose(f);
    const char *why = eq_params_error(head[3], head[4], head[5], head[6], head[7], head[8], max_steps, nmax);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    const KtParams p = kt_make_params(head[3], head[4], head[5], head[6], head[7], head[8], max_steps, 0);
    const size_t nc = (size_t)EQ_ROWS * n * nmax;
    double *cross = (double *)malloc(sizeof(double) * nc);
    int32_t *count = (int32_t *)malloc(sizeof(int32_t) * n);
    int32_t *status = (int32_t *)malloc(sizeof(int32_t) * n);
    if (!cross || !count || !status) return 2;
    memset(cross, 0x7F, sizeof(double) * nc);                 // 1.4e306 / 0x7F7F7F7F where an element is left unwritten
    memset(count, 0x7F, sizeof(int32_t) * n);
    memset(status, 0x7F, sizeof(int32_t) * n);
    for (int64_t i = 0; i < n; ++i) eq_trace_ray(p, nmax, alpha[i], beta[i], i, n, cross, count, status);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(cross, sizeof(double), nc, o) == nc && fwrite(count, sizeof(int32_t), n, o) == (size_t)n &&
              fwrite(status, sizeof(int32_t), n, o) == (size_t)n;
    ok = (fclose(o) == 0) && ok;
    free(cross); free(count); free(status);
    return ok ? 0 : 2;
}
