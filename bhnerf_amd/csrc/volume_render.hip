// VolumeVisualizer.render (visualization.py:545-591) fused: colour map and alpha (render) -> wireframe cube (draw_cube,
// visualization.py:702-736) -> black-hole sphere (draw_bh, :748-755) -> alpha_composite (:628-663).  One launch renders all N
// frames over the shared sample points.
//
// Mapping.  A group of LPR lanes (16, 32 or 64) owns one ray (h, w); samples lie across the lanes, 64-sample chunks follow each
// other for longer rays, so the emission reads of a group are consecutive floats.  Everything that depends on the point alone --
// the wireframe sum, the masks, the step length, the black-hole shade -- is computed once per chunk and used by up to VOL_NF frames
// (blockIdx.y walks the frames in groups of VOL_NF).  The back-to-front recurrence of alpha_composite
//     R <- (R + m c)(1 - oa) + c oa,  acc <- a + (1 - a) acc,  R += 1 - acc           (m in {0, 1}, oa = a (1 - m))
// is evaluated in its closed form  R = sum_s c_s (m_s + oa_s) prod_{s' < s} (1 - oa_s') + prod_s (1 - a_s):  per chunk an
// exclusive prefix product (shuffle scan over the group) and four butterfly reductions, carried from chunk to chunk in a fixed
// order.  No atomics: two runs are bitwise equal, and a frame's image does not depend on the frames rendered with it.
//
// The wireframe sum  1e6 sum_q exp(-|p - q| / lw^2)  over the 3072 points q = v_i + t_k d_j is the whole cost of the reference.
// Here
//   * points that draw_cube zeroes (max|p_c| > fw/2 + lw) and points inside the black hole (alpha := 1) skip it: exact;
//   * it stops once alpha >= 1 for every frame of the group (terms are >= 0, alpha is clipped to [0, 1]): exact;
//   * terms with |p - q| > CUT = 39 lw^2 are dropped.  BOUND: such a term is < 1e6 exp(-39) = 1.155e-11, and there are at most
//     3072 of them, so what any point's alpha loses is < 3.55e-8 < 2^-24 = 5.96e-8.  (The least multiple that would do is
//     ln(1e6 * 3072 * 2^24) = 38.48: the tests below are 1.3 % of CUT away from it, their rounding errors are ~1e-7.)
//     Every q has two coordinates equal to +-fw/2 (it lies on the line of a cube edge, or on its continuation for the 24 outward
//     stubs), and |p - q| >= |p_a - q_a| >= ||p_a| - fw/2| for each of them:
//       - a point with fewer than two axes a with ||p_a| - fw/2| <= CUT is farther than CUT from every q (pre-test: no term kept);
//       - a segment (i, j) whose two fixed coordinates are farther than CUT from p in the plane across it is dropped whole (64 terms);
//       - on a kept segment only the k with |along - t_k| <= CUT can be within CUT; the range of k is widened to the next integers
//         outward.  Keeping a term that could have been dropped is always right: only dropping needs the bound.
//   The differences p - q are formed in double (p, fw/2 and t_k = k fw / 63 are then exact to 1e-16): in float the cancellation
//   of coordinates of size fw/2 would put ~fw 2^-24 / lw^2 of relative error on every term near a line.
//
// Parity notes: the step length is that of image row 0 for every row (alpha_composite takes dists[0, ...]); thresholds are
// compared in double against the float coordinates, as the reference evaluated on the same float inputs does.
#include <math.h>

#include "common.h"

#define VOL_NF 4        // frames that share one pass over the points

struct VolView {
    double half, zero_above, inside_below, bh2, step, inv_step, cut, cut2, fw;
    float neg_log2e_over_lw2, alb[3];
    int bh;
};

// 1e6 sum_q exp(-|p - q| / lw^2) in the reference's order (vertex i, direction j, sample k), or any value >= stop once reached
__device__ __forceinline__ float volume_wire_sum(float px, float py, float pz, const VolView &v, float stop) {
    const double x = px, y = py, z = pz;
    const int near = (fabs(fabs(x) - v.half) <= v.cut) + (fabs(fabs(y) - v.half) <= v.cut) + (fabs(fabs(z) - v.half) <= v.cut);
    if (near < 2) return 0.f;
    float sum = 0.f;
    for (int i = 0; i < 8; ++i) {
        double u[3];                                       // p - v_i; vertex i has bit c of i set where coordinate c is +fw/2
        u[0] = x - ((i & 1) ? v.half : -v.half);
        u[1] = y - ((i & 2) ? v.half : -v.half);
        u[2] = z - ((i & 4) ? v.half : -v.half);
#pragma unroll
        for (int j = 0; j < 6; ++j) {                      // d_j = -x, +x, -y, +y, -z, +z
            const int c = j >> 1, a = (c + 1) % 3, b = (c + 2) % 3;
            const double r2 = u[a] * u[a] + u[b] * u[b];
            if (r2 > v.cut2) continue;
            const double along = (j & 1) ? u[c] : -u[c];   // (p - v_i) . d_j
            const double lo = fmax((along - v.cut) * v.inv_step, 0.0), hi = fmin((along + v.cut) * v.inv_step, 63.0);
            if (!(lo <= hi)) continue;
            const int k1 = (int)ceil(hi);
            for (int k = (int)lo; k <= k1; ++k) {
                const double t = k == 63 ? v.fw : (double)k * v.step;          // np.linspace(0, fw, 64)
                const double d = along - t;
                const float dist = sqrtf((float)(r2 + d * d));
                sum += 1e6f * __builtin_amdgcn_exp2f(dist * v.neg_log2e_over_lw2);
            }
            if (sum >= stop) return sum;
        }
    }
    return sum;
}

template <int LPR>
__global__ __launch_bounds__(256) void volume_render_kernel(const float *__restrict__ pts, const float *__restrict__ emission,
                                                            const float *__restrict__ alpha_scale, int N, long long HW, int W, int S,
                                                            long long frame_stride, const float *__restrict__ lut, int lut_n, VolView v,
                                                            float *__restrict__ images) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const long long ray = (long long)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool ok = ray < HW;
    const int n0 = blockIdx.y * VOL_NF;
    const int nf = N - n0 < VOL_NF ? N - n0 : VOL_NF;
    const long long row0 = ok ? (ray % W) * (long long)S : 0;       // the ray of image row 0 in the same column
    float scale[VOL_NF], T[VOL_NF], A[VOL_NF], R[VOL_NF][3];
#pragma unroll
    for (int f = 0; f < VOL_NF; ++f) {
        scale[f] = f < nf ? alpha_scale[n0 + f] : 0.f;
        T[f] = 1.f; A[f] = 1.f;
        R[f][0] = R[f][1] = R[f][2] = 0.f;
    }
    for (int s0 = 0; s0 < S; s0 += LPR) {
        const int s = s0 + sub;
        const bool live = ok && s < S;
        float e[VOL_NF];
        float px = 0.f, py = 0.f, pz = 0.f, step = 0.f, wire = 0.f, shade = 0.f;
        bool zeroed = false, hole = false, inside = false;
        if (live) {
            const long long pi = ray * S + s;
            float amin = 0.f;
#pragma unroll
            for (int f = 0; f < VOL_NF; ++f) {
                e[f] = f < nf ? emission[(long long)(n0 + f) * frame_stride + pi] : 0.f;
                amin = fminf(amin, e[f] * scale[f]);
            }
            px = pts[3 * pi]; py = pts[3 * pi + 1]; pz = pts[3 * pi + 2];
            if (s + 1 < S) {
                const float *q = pts + 3 * (row0 + s);
                const float dx = q[3] - q[0], dy = q[4] - q[1], dz = q[5] - q[2];
                step = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
            }
            const double amax = (double)fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
            const double r2 = (double)px * px + (double)py * py + (double)pz * pz;
            zeroed = amax > v.zero_above;
            hole = v.bh && r2 < v.bh2;
            inside = amax < v.inside_below && r2 > v.bh2;
            if (hole) shade = (float)((-(double)px - (double)py + (double)pz) * 0.57735026918962576451);    // l . p, l = (-1, -1, 1) / sqrt 3
            // alpha = e scale + wire >= 1 in every frame of the group once wire >= 1 - min(0, min_f e_f scale_f) (+ rounding room)
            else if (!zeroed) wire = volume_wire_sum(px, py, pz, v, (1.f - amin) * 1.00001f);
        }
#pragma unroll
        for (int f = 0; f < VOL_NF; ++f) {
            if (f >= nf) break;                            // (block-uniform)
            float c0 = 0.f, c1 = 0.f, c2 = 0.f, a = 0.f;
            if (live) {
                if (hole) {
                    c0 = shade * v.alb[0]; c1 = shade * v.alb[1]; c2 = shade * v.alb[2];
                    a = 1.f;
                } else if (!zeroed) {
                    // matplotlib's Colormap.__call__ on floats: int(e N), e N == N -> N - 1, below / above -> first / last entry
                    const float t = fminf(fmaxf(e[f] * (float)lut_n, -1.f), (float)lut_n);
                    int i = t == (float)lut_n ? lut_n - 1 : (int)t;
                    i = i < 0 ? 0 : (i > lut_n - 1 ? lut_n - 1 : i);
                    c0 = lut[3 * i] - 0.05f; c1 = lut[3 * i + 1] - 0.05f; c2 = lut[3 * i + 2] - 0.05f;
                    a = e[f] * scale[f] + wire;
                }
                c0 = fminf(fmaxf(c0, 0.f), 1.f) * step; c1 = fminf(fmaxf(c1, 0.f), 1.f) * step; c2 = fminf(fmaxf(c2, 0.f), 1.f) * step;
                a = fminf(fmaxf(a, 0.f), 1.f);
            }
            const float oa = inside ? 0.f : a;
            // inclusive prefix product of (1 - oa) over the group, then the exclusive one
            float incl = 1.f - oa;
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) {
                const float up = __shfl_up(incl, o, LPR);
                if (sub >= o) incl *= up;
            }
            float excl = __shfl_up(incl, 1, LPR);
            if (sub == 0) excl = 1.f;
            const float wgt = (inside ? 1.f : oa) * (T[f] * excl);
            float r0 = c0 * wgt, r1 = c1 * wgt, r2 = c2 * wgt, g = 1.f - a;
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) {
                r0 += __shfl_xor(r0, o, LPR);
                r1 += __shfl_xor(r1, o, LPR);
                r2 += __shfl_xor(r2, o, LPR);
                g *= __shfl_xor(g, o, LPR);
            }
            R[f][0] += r0; R[f][1] += r1; R[f][2] += r2;
            A[f] *= g;
            T[f] *= __shfl(incl, LPR - 1, LPR);
        }
    }
    if (ok && sub == 0) {
#pragma unroll
        for (int f = 0; f < VOL_NF; ++f) {
            if (f >= nf) break;
            float *o = images + ((long long)(n0 + f) * HW + ray) * 3;
            o[0] = R[f][0] + A[f]; o[1] = R[f][1] + A[f]; o[2] = R[f][2] + A[f];
        }
    }
}

extern "C" int bhn_volume_render(const float *pts, const float *emission, const float *alpha_scale, int32_t N, int32_t H, int32_t W,
                                 int32_t S, int64_t frame_stride, const float *lut, int32_t lut_n, const bhn_volume_view *view,
                                 float *images, void *stream) {
    BHN_CHECK_ARG(pts && emission && alpha_scale && lut && view && images, "null pointer");
    BHN_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && S >= 1, "bad sizes N=%d H=%d W=%d S=%d", N, H, W, S);
    BHN_CHECK_ARG(lut_n >= 2, "colour table of %d entries (at least 2)", lut_n);
    BHN_CHECK_ARG(view->facewidth > 0.0 && view->linewidth > 0.0, "facewidth %g and linewidth %g must be positive", view->facewidth, view->linewidth);
    BHN_CHECK_ARG(view->bh_radius >= 0.0, "bh_radius %g is negative", view->bh_radius);
    BHN_CHECK_ARG(isfinite(view->facewidth) && isfinite(view->linewidth) && isfinite(view->bh_radius), "non-finite view");
    BHN_CHECK_ARG(frame_stride >= 0, "negative frame_stride");
    const long long HW = (long long)H * W;
    const int lpr = S <= 16 ? 16 : (S <= 32 ? 32 : 64);
    const long long blocks = (HW + 256 / lpr - 1) / (256 / lpr), groups = ((long long)N + VOL_NF - 1) / VOL_NF;
    BHN_CHECK_ARG(blocks <= 0x7fffffffLL && groups <= 65535, "too many rays (%lld) or frames (%d) for one launch", HW, N);
    VolView v;
    const double fw = view->facewidth, lw = view->linewidth, bh = view->bh_radius;
    v.fw = fw;
    v.half = 0.5 * fw;
    v.zero_above = 0.5 * fw + lw;          // draw_cube: greater(amax|p|, facewidth / 2 + linewidth)
    v.inside_below = 0.5 * fw - lw;        // alpha_composite: less(amax|p|, facewidth / 2 - linewidth)
    v.bh2 = bh * bh;
    v.bh = bh > 0.0 ? 1 : 0;
    v.step = fw / 63.0;
    v.inv_step = 63.0 / fw;
    v.cut = 39.0 * lw * lw;
    v.cut2 = v.cut * v.cut;
    v.neg_log2e_over_lw2 = (float)(-1.4426950408889634074 / (lw * lw));
    for (int c = 0; c < 3; ++c) v.alb[c] = (float)view->bh_albedo[c];
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)groups);
    if (lpr == 16) hipLaunchKernelGGL((volume_render_kernel<16>), grid, dim3(256), 0, st, pts, emission, alpha_scale, N, HW, W, S, (long long)frame_stride, lut, lut_n, v, images);
    else if (lpr == 32) hipLaunchKernelGGL((volume_render_kernel<32>), grid, dim3(256), 0, st, pts, emission, alpha_scale, N, HW, W, S, (long long)frame_stride, lut, lut_n, v, images);
    else hipLaunchKernelGGL((volume_render_kernel<64>), grid, dim3(256), 0, st, pts, emission, alpha_scale, N, HW, W, S, (long long)frame_stride, lut, lut_n, v, images);
    BHN_HIP(hipGetLastError());
    return BHN_OK;
}
