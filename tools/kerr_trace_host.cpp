// CPU build of the stepping code of bhn_kerr_trace (bhnerf_amd/csrc/kerr_trace.h): the arithmetic the device runs, one ray after
// the other, for tests/test_kerr_trace_cpu.py to compare with geodesics._integrate and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/kerr_trace_host.cpp -o kerr_trace_host
//   kerr_trace_host IN OUT
//
// IN:  float64 [n, ngeo, max_steps, spin, inclination, distance, M, h, r_c, alpha[n], beta[n]]
// OUT: float64 end[7 n], int32 status[n], float64 samples[7 n ngeo]  (the layouts of include/bhnerf_kerr.h)
// The three outputs are separate heap blocks of exactly the documented size, so that an index outside them is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kerr_trace.h"

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
    const int32_t ngeo = (int32_t)head[1], max_steps = (int32_t)head[2];
    if (n < 1 || (ngeo > 0 && n > (int64_t)1 << 24)) { fprintf(stderr, "bad ray count\n"); return 2; }
    std::vector<double> alpha(n), beta(n);
    if (fread(alpha.data(), sizeof(double), n, f) != (size_t)n || fread(beta.data(), sizeof(double), n, f) != (size_t)n) {
        fprintf(stderr, "short ray list\n");
        return 2;
    }
    fclose(f);
    const char *why = kt_params_error(head[3], head[4], head[5], head[6], head[7], head[8], max_steps, ngeo);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    const KtParams p = kt_make_params(head[3], head[4], head[5], head[6], head[7], head[8], max_steps, ngeo);
    const size_t ns = (size_t)KT_ROWS * n * ngeo;
    double *end = (double *)malloc(sizeof(double) * KT_ROWS * n);
    int32_t *status = (int32_t *)malloc(sizeof(int32_t) * n);
    double *samples = ngeo > 0 ? (double *)malloc(sizeof(double) * ns) : nullptr;
    if (!end || !status || (ngeo > 0 && !samples)) return 2;
    memset(end, 0xFF, sizeof(double) * KT_ROWS * n);          // NaN / 0x7F7F7F7F where the tracer leaves an element unwritten
    memset(status, 0x7F, sizeof(int32_t) * n);
    if (samples) memset(samples, 0xFF, sizeof(double) * ns);
    for (int64_t i = 0; i < n; ++i) kt_trace_ray(p, alpha[i], beta[i], i, n, samples, end, status);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(end, sizeof(double), KT_ROWS * n, o) == (size_t)(KT_ROWS * n) && fwrite(status, sizeof(int32_t), n, o) == (size_t)n;
    if (ngeo > 0) ok = ok && fwrite(samples, sizeof(double), ns, o) == ns;
    ok = (fclose(o) == 0) && ok;
    free(end); free(status); free(samples);
    return ok ? 0 : 2;
}
