// CPU build of the per-point code of libbhnerf_flow.so (bhnerf_amd/csrc/flow_factors.h on gr_factors.h): the arithmetic the device runs,
// walked launch by launch and workgroup by workgroup, for tests/test_flow_factors_cpu.py to compare with the NumPy functions of
// bhnerf_amd/kgeo.py and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/flow_factors_host.cpp -o flow_factors_host
//   flow_factors_host IN OUT
//
// IN:  float64 [n, ngeo, spin, M, E, inc, fillna, fill, given_umu, beta, chi, given_b, arad, avert, ator, divisor, Q_frac, V_frac,
//      spectral_index, zamo_frame], then r, theta, affine, Delta, Sigma, Xi, R, Theta, omega (n ngeo each), then lam, alpha, beta (n each),
//      then umu (n ngeo 4) when given_umu != 0, then b (n ngeo 3) when given_b != 0
// OUT: float64 umu[n ngeo 4] when given_umu = 0 (bhn_flow_zamo_velocity), g[n ngeo] (bhn_flow_doppler), b[n ngeo 3] when given_b = 0
//      (bhn_flow_fluid_field), J[S n ngeo] (bhn_flow_transport, S = 3, or 4 when V_frac != 0; bhn_flow_transport_zamo with zamo_frame != 0,
//      S = 3): the layouts of include/bhnerf_flow.h.  b is divided by `divisor` in the transport unless divisor = 0 (a NULL divisor).
// Inputs and outputs are separate heap blocks of exactly the documented size, so that an index outside them is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flow_factors.h"

#define HEAD 20

static double *block(size_t count, int fill) {
    double *p = (double *)malloc(sizeof(double) * (count ? count : 1));
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, fill, sizeof(double) * count);
    return p;
}

static double *read_block(FILE *f, size_t count, const char *what) {
    double *p = block(count, 0);
    if (fread(p, sizeof(double), count, f) != count) { fprintf(stderr, "short %s\n", what); exit(2); }
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
    const double fillna = head[6];
    const int fill = head[7] != 0.0, given_umu = head[8] != 0.0, given_b = head[11] != 0.0, zamo_frame = head[19] != 0.0;
    const double beta = head[9], chi = head[10], arad = head[12], avert = head[13], ator = head[14], divisor = head[15];
    const double Q_frac = head[16], V_frac = zamo_frame ? 0.0 : head[17], spectral_index = head[18];
    double *pt[9], *ray[3];
    for (int i = 0; i < 9; ++i) pt[i] = read_block(f, total, "point field");
    for (int i = 0; i < 3; ++i) ray[i] = read_block(f, (size_t)n, "ray field");
    double *umu = given_umu ? read_block(f, 4 * total, "umu") : block(4 * total, 0xFF);
    double *b = given_b ? read_block(f, 3 * total, "b") : block(3 * total, 0xFF);
    fclose(f);
    FlowGeos g;
    g.n = n; g.ngeo = ngeo;
    g.r = pt[0]; g.theta = pt[1]; g.affine = pt[2]; g.Delta = pt[3]; g.Sigma = pt[4]; g.Xi = pt[5]; g.R = pt[6]; g.Theta = pt[7];
    g.omega = pt[8];
    g.lam = ray[0]; g.alpha = ray[1]; g.beta = ray[2];
    g.a = head[2]; g.M = head[3]; g.E = head[4]; g.sin_inc = sin(head[5]);
    const char *why = flow_geos_error(g);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    if (Q_frac > 1.0 || Q_frac < 0.0) { fprintf(stderr, "Q_frac should be in [0,1]\n"); return 1; }
    if (zamo_frame && given_umu) { fprintf(stderr, "the ZAMO frame needs beta and chi\n"); return 1; }
    const int with_v = V_frac != 0.0, S = with_v ? 4 : 3;
    const long long blocks = ((long long)total + GRF_BLOCK - 1) / GRF_BLOCK;
    double *gfac = block(total, 0xFF), *J = block((size_t)S * total, 0xFF);

#define FOR_EACH_POINT                                   \
    for (long long blk = 0; blk < blocks; ++blk)         \
        for (int t = 0; t < GRF_BLOCK; ++t)              \
            if (const long long p = blk * GRF_BLOCK + t; p < (long long)total)

    if (!given_umu)                                      // bhn_flow_zamo_velocity
        FOR_EACH_POINT flow_zamo_frame_velocity(g, p, beta, chi, umu + 4 * p);
    FOR_EACH_POINT gfac[p] = flow_point_doppler(g, p, umu + 4 * p, fillna, fill);          // bhn_flow_doppler
    if (!given_b)                                        // bhn_flow_fluid_field
        FOR_EACH_POINT flow_point_fluid_field(g, p, umu + 4 * p, arad, avert, ator, b + 3 * p);
    FOR_EACH_POINT {                                     // bhn_flow_transport / bhn_flow_transport_zamo
        double v[3] = {b[3 * p], b[3 * p + 1], b[3 * p + 2]}, out[4];
        if (divisor != 0.0)
            for (int i = 0; i < 3; ++i) v[i] = v[i] / divisor;
        if (zamo_frame)
            flow_point_transport_zamo(g, p, beta, chi, gfac[p], v, Q_frac, spectral_index, out);
        else
            flow_point_transport(g, p, umu + 4 * p, gfac[p], v, Q_frac, V_frac, spectral_index, with_v, out);
        for (int s = 0; s < S; ++s) J[(size_t)s * total + p] = out[s];
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = true;
    if (!given_umu) ok = fwrite(umu, sizeof(double), 4 * total, o) == 4 * total && ok;
    ok = fwrite(gfac, sizeof(double), total, o) == total && ok;
    if (!given_b) ok = fwrite(b, sizeof(double), 3 * total, o) == 3 * total && ok;
    ok = fwrite(J, sizeof(double), (size_t)S * total, o) == (size_t)S * total && ok;
    ok = (fclose(o) == 0) && ok;
    for (int i = 0; i < 9; ++i) free(pt[i]);
    for (int i = 0; i < 3; ++i) free(ray[i]);
    free(umu); free(b); free(gfac); free(J);
    return ok ? 0 : 2;
}
