// The EHT chi-square from (u, v) coordinates (libbhnerf_eht.so, include/bhnerf_eht.h): the host-side plan and the per-element
// arithmetic, without HIP dependencies.  csrc/eht_uv.hip runs this code on the device; tools/eht_uv_host.cpp compiles the same
// header with a plain C++ compiler and walks the same plan one block after the other (tests/test_eht_uv_cpu.py).
//
// A[k, (y, x)] = exp(-2 pi i (u_k x_x + v_k y_y)) = Eu[k, x] Ev[k, y] is separable, so the visibilities of a plane are
//     V_k = sum_x Eu[k, x] sum_y I[y, x] Ev[k, y]
// and the adjoint is dI[y, x] = Re sum_k conj(gv_k) Eu[k, x] Ev[k, y] with gv_k = dL/dRe V_k + i dL/dIm V_k.  Nothing of size
// nvis x H x W exists anywhere: the operator is the float64 (u, v) list and two complex64 tables of nvis (W + H) entries per frame.
#ifndef BHNERF_EHT_UV_H
#define BHNERF_EHT_UV_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EHT_HD __host__ __device__ inline
#else
#define EHT_HD inline
#endif

struct alignas(8) EhtC {          // complex64, interleaved (re, im)
    float x, y;
};

#define EHT_KB 8                  // baselines per workgroup of the forward pass: an image value in a register serves all of them
#define EHT_MIN_ROWS 8            // a row split of the forward pass holds at least this many image rows
#define EHT_MAX_SPLITS 64
#define EHT_ADJ_ROWS 4            // image rows per workgroup of the adjoint
#define EHT_DTYPE_VIS 0
#define EHT_DTYPE_AMP 1
#define EHT_DTYPE_CPHASE 2

// ---------------------------------------------------------------------------------------------------------------------------
// The plan: every size and workspace offset a call uses.  It depends on (N, nvis, ncp, H, W) only -- never on the number of
// frames per call in a way that changes a frame's arithmetic: the row split is a function of (nvis, H), so one frame's
// visibilities and gradient do not depend on the batch it is computed in.
// ---------------------------------------------------------------------------------------------------------------------------
struct EhtPlan {
    int32_t N, nvis, ncp, H, W;
    int32_t kblocks;              // ceil(nvis / EHT_KB)
    int32_t RS, rows_per;         // row splits of the forward pass; split s covers rows [s rows_per, min(H, (s + 1) rows_per))
    int32_t block;                // threads per workgroup of the forward pass and the adjoint: W rounded up to waves, 64..256
    int32_t loss_blocks;          // workgroups of the loss stage, one per plane = partial loss sums
    // workspace offsets in bytes, each a multiple of 256
    size_t off_eu, off_ev, off_part, off_vis, off_dphi, off_loss, bytes;
};

EHT_HD size_t eht_align256(size_t v) { return (v + 255) & ~(size_t)255; }

EHT_HD int eht_row_splits(int32_t nvis, int32_t H) {
    const int kblocks = (nvis + EHT_KB - 1) / EHT_KB;
    int rs = (256 + kblocks - 1) / kblocks;                // one frame alone should put a workgroup on every CU
    const int most = (H + EHT_MIN_ROWS - 1) / EHT_MIN_ROWS;
    if (rs > most) rs = most;
    if (rs > EHT_MAX_SPLITS) rs = EHT_MAX_SPLITS;
    if (rs < 1) rs = 1;
    const int rows_per = (H + rs - 1) / rs;
    return (H + rows_per - 1) / rows_per;                  // no empty split
}

// false when a size is below 1 (ncp may be 0: no closure phases) or the sizes do not fit the 32-bit launch geometry
EHT_HD bool eht_make_plan(int32_t N, int32_t nvis, int32_t ncp, int32_t H, int32_t W, EhtPlan *p) {
    if (N < 1 || nvis < 1 || ncp < 0 || H < 1 || W < 1) return false;
    if (N > 65535 || (int64_t)N * nvis > 0x3fffffff || (int64_t)N * ncp > 0x3fffffff || (int64_t)H * W > 0x3fffffff || H > 65535 * EHT_ADJ_ROWS)
        return false;
    p->N = N; p->nvis = nvis; p->ncp = ncp; p->H = H; p->W = W;
    p->kblocks = (nvis + EHT_KB - 1) / EHT_KB;
    p->RS = eht_row_splits(nvis, H);
    p->rows_per = (H + p->RS - 1) / p->RS;
    const int wv = (W + 63) / 64;
    p->block = 64 * (wv < 1 ? 1 : (wv > 4 ? 4 : wv));
    p->loss_blocks = N;
    size_t o = 0;
    p->off_eu = o;   o += eht_align256(sizeof(EhtC) * (size_t)N * nvis * W);          // frames <= planes: sized for Sx = 1
    p->off_ev = o;   o += eht_align256(sizeof(EhtC) * (size_t)N * nvis * H);
    p->off_part = o; o += eht_align256(sizeof(EhtC) * (size_t)N * nvis * p->RS);
    p->off_vis = o;  o += eht_align256(sizeof(EhtC) * (size_t)N * nvis);
    p->off_dphi = o; o += eht_align256(sizeof(float) * (size_t)N * ncp);
    p->off_loss = o; o += eht_align256(sizeof(float) * (size_t)p->loss_blocks);
    p->bytes = o;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Twiddle tables.  Pixel centres are observation.dft_matrix's: (i - (n - 1) / 2) psize.  The phase is formed in float64, reduced
// to turns (the part of u x beyond whole turns: |t| <= 1/2) before the sine and cosine, and rounded to complex64 last.
// ---------------------------------------------------------------------------------------------------------------------------
EHT_HD EhtC eht_twiddle(double u, int i, int n, double psize) {
    const double x = ((double)i - 0.5 * (double)(n - 1)) * psize;
    double t = u * x;                                      // turns; exp(-2 pi i t)
    t -= rint(t);
    const double a = -6.283185307179586476925286766559 * t;
    EhtC e;
    e.x = (float)cos(a);
    e.y = (float)sin(a);
    return e;
}

EHT_HD EhtC eht_cmul(EhtC a, EhtC b) {
    EhtC r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

// index helpers shared by the device kernels and the host walk
EHT_HD size_t eht_eu_index(const EhtPlan &p, int b, int k, int x) { return ((size_t)b * p.nvis + k) * p.W + x; }
EHT_HD size_t eht_ev_index(const EhtPlan &p, int b, int k, int y) { return ((size_t)b * p.nvis + k) * p.H + y; }
EHT_HD size_t eht_part_index(const EhtPlan &p, int n, int k, int s) { return ((size_t)n * p.nvis + k) * p.RS + s; }

// One image column x of row split s for the EHT_KB baselines from k0 (the unit of work of a forward lane): an image value is
// loaded once and serves all of them.  out[j] = Eu[k0 + j, x] sum_y I[y, x] Ev[k0 + j, y].  Baselines past nvis repeat the last
// one (their results are never stored), so the loop has no tail.
EHT_HD void eht_columns(const EhtPlan &p, const float *images, const EhtC *Eu, const EhtC *Ev, int n, int b, int k0, int s, int x,
                        EhtC out[EHT_KB]) {
    const int r0 = s * p.rows_per, r1 = r0 + p.rows_per < p.H ? r0 + p.rows_per : p.H;
    EhtC c[EHT_KB];
    size_t ev[EHT_KB];
    for (int j = 0; j < EHT_KB; ++j) {
        const int k = k0 + j < p.nvis ? k0 + j : p.nvis - 1;
        c[j].x = c[j].y = 0.f;
        ev[j] = eht_ev_index(p, b, k, 0);
    }
    for (int y = r0; y < r1; ++y) {
        const float v = images[((size_t)n * p.H + y) * p.W + x];
        for (int j = 0; j < EHT_KB; ++j) {
            const EhtC e = Ev[ev[j] + y];
            c[j].x += v * e.x;
            c[j].y += v * e.y;
        }
    }
    for (int j = 0; j < EHT_KB; ++j) {
        const int k = k0 + j < p.nvis ? k0 + j : p.nvis - 1;
        out[j] = eht_cmul(c[j], Eu[eht_eu_index(p, b, k, x)]);
    }
}

// Stage 2: a visibility is the sum of its RS partial sums, in order.
EHT_HD EhtC eht_combine(const EhtPlan &p, const EhtC *part, int n, int k) {
    EhtC v = {0.f, 0.f};
    for (int s = 0; s < p.RS; ++s) {
        const EhtC q = part[eht_part_index(p, n, k, s)];
        v.x += q.x;
        v.y += q.y;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// chi^2 terms and their derivatives: the arithmetic of eht_loss_kernel (csrc/simple_kernels.hip), the zero gradient at |vis| = 0
// included.  `term` is unscaled (the caller multiplies the block sum by scale); the derivative carries the scale.
// ---------------------------------------------------------------------------------------------------------------------------
EHT_HD float eht_term_vis(EhtC v, float tre, float tim, float s, float scale, EhtC *gv) {
    const float dr = v.x - tre, di = v.y - tim;
    gv->x = 2.f * scale * dr / (s * s);
    gv->y = 2.f * scale * di / (s * s);
    return (dr * dr + di * di) / (s * s);
}

EHT_HD float eht_term_amp(EhtC v, float target, float s, float scale, EhtC *gv) {
    const float amp = sqrtf(v.x * v.x + v.y * v.y);
    const float d = (amp - target) / s;
    const float g = amp > 0.f ? 2.f * scale * d / (s * amp) : 0.f;
    gv->x = g * v.x;
    gv->y = g * v.y;
    return d * d;
}

// closure phase of triangle c of plane n from the table: phi = sum_legs sign atan2; *dphi = dL/dphi
// (a table index outside [0, nvis) is the caller's error; it is clamped so that it cannot read outside the plane's visibilities)
EHT_HD float eht_term_cphase(const EhtC *vis_n, int nvis, const int32_t *tri, const int8_t *tri_sign, int c, float target, float s,
                             float scale, float *dphi) {
    float phi = 0.f;
    for (int l = 0; l < 3; ++l) {
        const int32_t k = tri[3 * c + l];
        const EhtC v = vis_n[k < 0 ? 0 : (k >= nvis ? nvis - 1 : k)];
        phi += (float)tri_sign[3 * c + l] * atan2f(v.y, v.x);
    }
    const float d = target - phi;
    *dphi = -scale * sinf(d) / (s * s);
    return (1.f - cosf(d)) / (s * s);
}

// Gradient of baseline k of one plane: the triangles it sits in are GATHERED in table order (a fixed order, no atomics):
// gv_k = w_k (-Im V_k, Re V_k) / |V_k|^2 with w_k = sum_{legs (c, l) on k} sign dphi_c, zero at |V_k| = 0.  eht_gather_weight sums
// the table entries j0, j0 + stride, ...: a device wave gives each lane one such slice and adds the 64 slices in a butterfly.
EHT_HD float eht_gather_weight(int k, const int32_t *tri, const int8_t *tri_sign, const float *dphi_n, int ncp, int j0, int stride) {
    float w = 0.f;
    for (int j = j0; j < 3 * ncp; j += stride)
        if (tri[j] == k) w += (float)tri_sign[j] * dphi_n[j / 3];
    return w;
}

EHT_HD EhtC eht_gather_gv(EhtC v, float w) {
    const float m2 = v.x * v.x + v.y * v.y;
    EhtC g = {0.f, 0.f};
    if (m2 > 0.f) {
        g.x = -w * v.y / m2;
        g.y = w * v.x / m2;
    }
    return g;
}

// Adjoint of one pixel given z_k = conj(gv_k) Eu[k, x]: the contribution of baseline k is Re(z_k Ev[k, y]).
EHT_HD EhtC eht_adjoint_z(EhtC gv, EhtC eu) {
    EhtC z;
    z.x = gv.x * eu.x + gv.y * eu.y;
    z.y = gv.x * eu.y - gv.y * eu.x;
    return z;
}
EHT_HD float eht_adjoint_mac(float acc, EhtC z, EhtC ev) { return acc + (z.x * ev.x - z.y * ev.y); }

// argument check shared by the entry points and the host program; NULL when the table is usable
EHT_HD const char *eht_sizes_error(int32_t N, int32_t Sx, int32_t nvis, int32_t ncp, int32_t H, int32_t W, double psize_x, double psize_y) {
    if (N < 1 || Sx < 1 || nvis < 1 || H < 1 || W < 1) return "sizes below 1";
    if (ncp < 0) return "ncp must be >= 0";
    if (N % Sx != 0) return "N must be a multiple of Sx";
    if (!(psize_x > 0.0) || !(psize_y > 0.0) || !(psize_x < 1e300) || !(psize_y < 1e300)) return "pixel sizes must be positive and finite";
    return (const char *)0;
}

#endif /* BHNERF_EHT_UV_H */
