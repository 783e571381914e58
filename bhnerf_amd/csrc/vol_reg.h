// Volume priors on the recovered 3-D emission (libbhnerf_reg.so, include/bhnerf_reg.h): the host-side plan and the per-voxel
// arithmetic, without HIP dependencies.  csrc/vol_reg.hip runs this code on the device; tools/vol_reg_host.cpp compiles the same
// header with a plain C++ compiler and walks the same plan one workgroup after the other (tests/test_vol_reg_cpu.py).
//
// A volume e[i, j, k] of dims (nx, ny, nz), k fastest; a mask m in {0, 1} shared by the N volumes of a call (NULL: all ones).
// Forward, masked differences: d_a[v] = (e[v + a] - e[v]) / h_a when v + a is inside the lattice and both voxels are in the mask,
// else exactly 0; q = dx^2 + dy^2 + dz^2.  The terms, in the canonical order:
//     tv  = sum m sqrt(q + eps^2)      tsv = sum m q      l1 = sum m |e|
// and with c[v] = w_tv / sqrt(q[v] + eps^2) + 2 w_tsv, T_a[v] = d_a[v] c[v] / h_a the gradient in its gather form (no atomics):
//     dloss/de[v] = m[v] ( -(T_x + T_y + T_z)[v] + T_x[v - x] + T_y[v - y] + T_z[v - z] + w_l1 sign(e[v]) )
// where w_d is the effective weight scale * weights[d] and a missing predecessor contributes 0.  The gradient of a voxel
// recomputes c of its three predecessors: 13 loads of e per voxel, all but one of them served by the caches.
#ifndef BHNERF_VOL_REG_H
#define BHNERF_VOL_REG_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define REG_HD __host__ __device__ inline
#else
#define REG_HD inline
#endif

#define REG_TERMS 3
#define REG_TV 0
#define REG_TSV 1
#define REG_L1 2
#define REG_BLOCK 256             // lanes per workgroup
#define REG_TRIPS 4               // voxels per lane: trip t of lane l of chunk c is voxel c REG_CHUNK + t REG_BLOCK + l
#define REG_CHUNK (REG_BLOCK * REG_TRIPS)

// ---------------------------------------------------------------------------------------------------------------------------
// The plan: every size and workspace offset a call uses.  The chunks of a volume depend on (nx, ny, nz) only, so a volume's
// partial sums, its per_volume row and its gradient do not depend on N or on where in the batch it stands.
// ---------------------------------------------------------------------------------------------------------------------------
struct RegPlan {
    int32_t N, nx, ny, nz;
    int64_t V;                    // voxels of one volume
    int32_t chunks;               // workgroups per volume: ceil(V / REG_CHUNK)
    // workspace offsets in bytes, each a multiple of 256
    size_t off_part;              // float part[N][REG_TERMS][chunks]: the workgroups' partial sums
    size_t off_pv;                // float pv[REG_TERMS][N]: the unscaled term sums per volume
    size_t bytes;
};

REG_HD size_t reg_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// false: a size below 1, or more than one call takes (a volume beyond 2^31 - 1 voxels, more than 2^31 - 1 workgroups)
REG_HD bool reg_make_plan(int32_t N, int32_t nx, int32_t ny, int32_t nz, RegPlan *p) {
    if (N < 1 || nx < 1 || ny < 1 || nz < 1) return false;
    if ((int64_t)nx * ny > 0x7fffffffLL) return false;     // (checked before the third factor: nothing below overflows 64 bits)
    const int64_t V = (int64_t)nx * ny * nz;
    if (V > 0x7fffffffLL - REG_CHUNK) return false;
    const int64_t chunks = (V + REG_CHUNK - 1) / REG_CHUNK;
    if (chunks * N > 0x7fffffffLL) return false;
    p->N = N; p->nx = nx; p->ny = ny; p->nz = nz;
    p->V = V;
    p->chunks = (int32_t)chunks;
    p->off_part = 0;
    p->off_pv = reg_align256(sizeof(float) * (size_t)N * REG_TERMS * (size_t)chunks);
    p->bytes = p->off_pv + reg_align256(sizeof(float) * (size_t)N * REG_TERMS);
    return true;
}

REG_HD size_t reg_part_index(const RegPlan &p, int n, int d, int chunk) { return ((size_t)n * REG_TERMS + d) * p.chunks + chunk; }

// The parameters of a call as the kernels take them.  w[d] = scale * weights[d], the product formed once in float64 on the host
// and rounded once to float32; a term is present when its w is not 0.
struct RegParams {
    float inv_h[3];               // 1 / spacing, rounded once from float64
    float w[REG_TERMS];
    float eps2;                   // eps^2; 0 when tv is absent (never used then)
};

REG_HD bool reg_finite(double v) { return v == v && v - v == 0.0; }

// NULL, or what is wrong with the parameters (the message of BHN_EINVAL)
REG_HD const char *reg_params_error(const float spacing[3], const float weights[3], float eps, float scale) {
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.f) || !reg_finite(spacing[a])) return "spacing must be positive and finite";
    for (int d = 0; d < REG_TERMS; ++d)
        if (!(weights[d] >= 0.f) || !reg_finite(weights[d])) return "weights must be finite and >= 0";
    if (!reg_finite(scale)) return "scale must be finite";
    if (weights[REG_TV] != 0.f && (!(eps > 0.f) || !reg_finite(eps))) return "eps must be positive and finite when the tv weight is not 0";
    return nullptr;
}

REG_HD RegParams reg_make_params(const float spacing[3], const float weights[3], float eps, float scale) {
    RegParams a;
    for (int i = 0; i < 3; ++i) a.inv_h[i] = (float)(1.0 / (double)spacing[i]);
    for (int d = 0; d < REG_TERMS; ++d) a.w[d] = (float)((double)scale * (double)weights[d]);
    a.eps2 = weights[REG_TV] != 0.f ? eps * eps : 0.f;
    return a;
}

REG_HD bool reg_in(const uint8_t *mask, int64_t v) { return mask ? mask[v] != 0 : true; }

// The forward differences of voxel v = (i, j, k), which must be in the mask: what stands in a masked-out neighbour is not read.
// Every index is v or v + a stride with the neighbour's coordinate checked against its dim: inside [0, V).
REG_HD void reg_diffs(const RegPlan &p, const RegParams &a, const float *e, const uint8_t *mask, int64_t v, int i, int j, int k, float ev,
                      float d[3]) {
    const int64_t sx = (int64_t)p.ny * p.nz, sy = p.nz;
    d[0] = (i + 1 < p.nx && reg_in(mask, v + sx)) ? (e[v + sx] - ev) * a.inv_h[0] : 0.f;
    d[1] = (j + 1 < p.ny && reg_in(mask, v + sy)) ? (e[v + sy] - ev) * a.inv_h[1] : 0.f;
    d[2] = (k + 1 < p.nz && reg_in(mask, v + 1)) ? (e[v + 1] - ev) * a.inv_h[2] : 0.f;
}

// c[v] of the header comment from q[v]
REG_HD float reg_c(const RegParams &a, float q) {
    float c = 2.f * a.w[REG_TSV];
    if (a.w[REG_TV] != 0.f) c += a.w[REG_TV] / sqrtf(q + a.eps2);
    return c;
}

// T_axis of the voxel u = (i, j, k), a predecessor of the voxel whose gradient is computed; 0 when u is masked out.  u's
// successor along `axis` is that voxel: inside the lattice.
REG_HD float reg_T_of(const RegPlan &p, const RegParams &a, const float *e, const uint8_t *mask, int64_t u, int i, int j, int k, int axis) {
    if (!reg_in(mask, u)) return 0.f;
    float d[3];
    reg_diffs(p, a, e, mask, u, i, j, k, e[u], d);
    const float q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    return d[axis] * reg_c(a, q) * a.inv_h[axis];
}

// One voxel v < V of volume e: its three unscaled terms (an absent term: 0) and, when grad is not NULL, grad[v].
REG_HD void reg_voxel(const RegPlan &p, const RegParams &a, const float *e, const uint8_t *mask, int64_t v, float term[REG_TERMS], float *grad) {
    term[REG_TV] = term[REG_TSV] = term[REG_L1] = 0.f;
    if (!reg_in(mask, v)) {
        if (grad) grad[v] = 0.f;
        return;
    }
    const int64_t sx = (int64_t)p.ny * p.nz, sy = p.nz;
    const int64_t ij = v / p.nz;
    const int k = (int)(v - ij * p.nz), i = (int)(ij / p.ny), j = (int)(ij - (int64_t)i * p.ny);
    const float ev = e[v];
    float d[3];
    reg_diffs(p, a, e, mask, v, i, j, k, ev, d);
    const float q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (a.w[REG_TV] != 0.f) term[REG_TV] = sqrtf(q + a.eps2);
    if (a.w[REG_TSV] != 0.f) term[REG_TSV] = q;
    if (a.w[REG_L1] != 0.f) term[REG_L1] = fabsf(ev);
    if (!grad) return;
    const float c = reg_c(a, q);
    float g = -(d[0] * c * a.inv_h[0] + d[1] * c * a.inv_h[1] + d[2] * c * a.inv_h[2]);
    if (i > 0) g += reg_T_of(p, a, e, mask, v - sx, i - 1, j, k, 0);
    if (j > 0) g += reg_T_of(p, a, e, mask, v - sy, i, j - 1, k, 1);
    if (k > 0) g += reg_T_of(p, a, e, mask, v - 1, i, j, k - 1, 2);
    g += a.w[REG_L1] * (ev > 0.f ? 1.f : (ev < 0.f ? -1.f : 0.f));
    grad[v] = g;
}

// loss[4] = {total, tv, tsv, l1} from the volumes' sums pv[REG_TERMS][N], added in the order of the volumes
REG_HD void reg_finish(const RegParams &a, const float *pv, int N, float *loss) {
    float total = 0.f;
    for (int d = 0; d < REG_TERMS; ++d) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += pv[(size_t)d * N + n];
        loss[1 + d] = a.w[d] != 0.f ? a.w[d] * s : 0.f;
        total += loss[1 + d];
    }
    loss[0] = total;
}

#endif
