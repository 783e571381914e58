// CPU build of the plan and the per-voxel arithmetic of libbhnerf_reg.so (bhnerf_amd/csrc/vol_reg.h): the launches of
// bhn_reg_loss walked one workgroup after the other, for tests/test_vol_reg_cpu.py to compare with a float64 reference and to run
// under a sanitizer.
//
//   g++ -O2 -ffp-contract=off [-fsanitize=address,undefined] -I bhnerf_amd/csrc tools/vol_reg_host.cpp -o vol_reg_host
//   vol_reg_host IN OUT
//
// IN:  float64 [N, nx, ny, nz, has_mask, want_grad, want_per_volume, hx, hy, hz, w_tv, w_tsv, w_l1, eps, scale],
//      float32 volumes[N nx ny nz], uint8 mask[nx ny nz] (when has_mask)
// OUT: float32 loss[4], float32 per_volume[3 N] (when want_per_volume), float32 dvolumes[N nx ny nz] (when want_grad)
// Exit status 1 with the message on stderr for arguments that bhn_reg_loss refuses with BHN_EINVAL.
// The workspace is one heap block of exactly bhn_reg_ws_bytes' size and every output a block of exactly its documented size, all
// filled with NaN bytes first, so that an index outside them is caught and an element left unwritten shows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vol_reg.h"

// reg_block_sum_256: the lanes of each wave by butterfly (lane 0's value), then the four waves in order
static float block_sum(const float *lane) {
    float red[4];
    for (int w = 0; w < 4; ++w) {
        float v[64], t[64];
        memcpy(v, lane + 64 * w, sizeof(v));
        for (int o = 32; o > 0; o >>= 1) {
            for (int i = 0; i < 64; ++i) t[i] = v[i] + v[i ^ o];
            memcpy(v, t, sizeof(v));
        }
        red[w] = v[0];
    }
    return red[0] + red[1] + red[2] + red[3];
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
    const int32_t N = (int32_t)head[0], nx = (int32_t)head[1], ny = (int32_t)head[2], nz = (int32_t)head[3];
    const bool has_mask = head[4] != 0, want_grad = head[5] != 0, want_pv = head[6] != 0;
    const float spacing[3] = {(float)head[7], (float)head[8], (float)head[9]}, weights[3] = {(float)head[10], (float)head[11], (float)head[12]};
    const float eps = (float)head[13], scale = (float)head[14];
    RegPlan p;
    if (!reg_make_plan(N, nx, ny, nz, &p)) { fprintf(stderr, "bad sizes\n"); return 1; }
    const char *why = reg_params_error(spacing, weights, eps, scale);
    if (why) { fprintf(stderr, "%s\n", why); return 1; }
    const RegParams a = reg_make_params(spacing, weights, eps, scale);
    const size_t V = (size_t)p.V, total = V * N;

    // the inputs too are heap blocks of exactly their sizes
    float *volumes = (float *)malloc(sizeof(float) * total);
    uint8_t *mask = has_mask ? (uint8_t *)malloc(V) : nullptr;
    if (!volumes || (has_mask && !mask)) return 2;
    if (fread(volumes, sizeof(float), total, f) != total || (has_mask && fread(mask, 1, V, f) != V)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);

    char *ws = (char *)malloc(p.bytes);
    float *loss = (float *)malloc(4 * sizeof(float));
    float *per_volume = want_pv ? (float *)malloc(sizeof(float) * 3 * N) : nullptr;
    float *dvolumes = want_grad ? (float *)malloc(sizeof(float) * total) : nullptr;
    if (!ws || !loss || (want_pv && !per_volume) || (want_grad && !dvolumes)) return 2;
    memset(ws, 0xFF, p.bytes);
    memset(loss, 0xFF, 4 * sizeof(float));
    if (per_volume) memset(per_volume, 0xFF, sizeof(float) * 3 * N);
    if (dvolumes) memset(dvolumes, 0xFF, sizeof(float) * total);
    float *part = reinterpret_cast<float *>(ws + p.off_part), *pv = reinterpret_cast<float *>(ws + p.off_pv);

    for (long long b = 0; b < (long long)p.chunks * N; ++b) {                           // reg_voxel_kernel: one workgroup per chunk
        const int n = (int)(b / p.chunks), chunk = (int)(b - (long long)n * p.chunks);
        const float *e = volumes + (size_t)n * V;
        float *grad = dvolumes ? dvolumes + (size_t)n * V : nullptr;
        std::vector<float> acc(REG_TERMS * REG_BLOCK, 0.f);
        for (int lane = 0; lane < REG_BLOCK; ++lane)
            for (int t = 0; t < REG_TRIPS; ++t) {
                const int64_t v = (int64_t)chunk * REG_CHUNK + t * REG_BLOCK + lane;
                if (v >= p.V) continue;
                float term[REG_TERMS];
                reg_voxel(p, a, e, mask, v, term, grad);
                for (int d = 0; d < REG_TERMS; ++d) acc[d * REG_BLOCK + lane] += term[d];
            }
        for (int d = 0; d < REG_TERMS; ++d) part[reg_part_index(p, n, d, chunk)] = block_sum(&acc[d * REG_BLOCK]);
    }
    for (int n = 0; n < N; ++n)                                                         // reg_sum_kernel: one workgroup
        for (int d = 0; d < REG_TERMS; ++d) {
            float acc[REG_BLOCK] = {0.f};
            for (int lane = 0; lane < REG_BLOCK; ++lane)
                for (int c = lane; c < p.chunks; c += REG_BLOCK) acc[lane] += part[reg_part_index(p, n, d, c)];
            const float tot = block_sum(acc);
            pv[(size_t)d * N + n] = tot;
            if (per_volume) per_volume[(size_t)d * N + n] = tot;
        }
    reg_finish(a, pv, N, loss);

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    bool ok = fwrite(loss, sizeof(float), 4, o) == 4;
    if (want_pv) ok = ok && fwrite(per_volume, sizeof(float), (size_t)3 * N, o) == (size_t)3 * N;
    if (want_grad) ok = ok && fwrite(dvolumes, sizeof(float), total, o) == total;
    ok = (fclose(o) == 0) && ok;
    free(volumes); free(mask); free(ws); free(loss); free(per_volume); free(dvolumes);
    return ok ? 0 : 2;
}
