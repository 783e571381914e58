// CPU build of the per-point code of bhn_rec_build and bhn_rec_kepler (bhnerf_amd/csrc/geo_record.h): the arithmetic the device runs,
// in the order of its two launches (every point, then every ray's cumulative sum), for tests/test_geo_record_cpu.py to compare with
// geodesics._build_record and to run under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/geo_record_host.cpp -o geo_record_host
//   geo_record_host IN OUT
//
// IN:  float64 [n, ngeo, spin, M, factor, nk, samples[7 n ngeo], lam[n], eta[n], rk[nk]]
// OUT: float64 the 18 fields of include/bhnerf_rec.h in its order, n ngeo each, then Omega[nk] of the radii rk
// Every output is a separate heap block of exactly the documented size, so that an index outside it is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "geo_record.h"

static bool read_all(FILE *f, std::vector<double> &v) { return v.empty() || fread(v.data(), sizeof(double), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    double head[6];
    if (fread(head, sizeof(double), 6, f) != 6) { fprintf(stderr, "short header\n"); return 2; }
    const long long n = (long long)head[0], nk = (long long)head[5];
    const int ngeo = (int)head[1];
    const double spin = head[2], M = head[3], factor = head[4];
    const char *why = rec_sizes_error(n, ngeo);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    if (n > (1LL << 24) / ngeo || nk < 0 || nk > (1LL << 24)) { fprintf(stderr, "bad sizes\n"); return 2; }
    const long long total = n * ngeo;
    std::vector<double> samples((size_t)REC_SAMPLE_ROWS * total), lam((size_t)n), eta((size_t)n), rk((size_t)nk);
    if (!read_all(f, samples) || !read_all(f, lam) || !read_all(f, eta) || !read_all(f, rk)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);

    double *blocks[REC_FIELDS];
    for (int i = 0; i < REC_FIELDS; ++i) {
        blocks[i] = (double *)malloc(sizeof(double) * total);
        if (!blocks[i]) return 2;
        memset(blocks[i], 0xFF, sizeof(double) * total);          // NaN where the code leaves an element unwritten
    }
    RecFields o;
    o.r = blocks[0]; o.theta = blocks[1]; o.phi = blocks[2]; o.t = blocks[3]; o.mino = blocks[4]; o.Delta = blocks[5]; o.Sigma = blocks[6];
    o.Xi = blocks[7]; o.omega = blocks[8]; o.x = blocks[9]; o.y = blocks[10]; o.z = blocks[11]; o.R = blocks[12]; o.Theta = blocks[13];
    o.vr = blocks[14]; o.vth = blocks[15]; o.dtau = blocks[16]; o.affine = blocks[17];
    for (long long p = 0; p < total; ++p) rec_build_point(samples.data(), lam.data(), eta.data(), p, ngeo, total, spin, M, o);
    for (long long ray = 0; ray < n; ++ray) rec_affine_ray(o.Sigma, o.dtau, o.affine, ray, ngeo);

    double *Omega = (double *)malloc(sizeof(double) * (nk > 0 ? nk : 1));
    if (!Omega) return 2;
    const double sqrt_M = sqrt(M);
    for (long long p = 0; p < nk; ++p) Omega[p] = rec_kepler(rk[p], factor * sqrt_M, spin * sqrt_M);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    bool ok = true;
    for (int i = 0; i < REC_FIELDS; ++i) ok = ok && fwrite(blocks[i], sizeof(double), total, out) == (size_t)total;
    if (nk > 0) ok = ok && fwrite(Omega, sizeof(double), nk, out) == (size_t)nk;
    ok = (fclose(out) == 0) && ok;
    for (int i = 0; i < REC_FIELDS; ++i) free(blocks[i]);
    free(Omega);
    return ok ? 0 : 2;
}
