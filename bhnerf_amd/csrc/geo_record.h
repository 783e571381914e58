// Per-point arithmetic of libbhnerf_rec.so: the geodesic record of bhnerf_amd/geodesics.py (`_build_record` with kerr_functions,
// radial_potential and angular_potential) restated for one sample point of one ray, and alma.image_plane_model's Keplerian Omega.
//
// No HIP dependency: geo_record.hip compiles it for the device, tools/geo_record_host.cpp for the CPU with a plain C++ compiler, so
// that the same arithmetic can be run under a sanitizer and compared with the NumPy code.  A restatement, not a new method: every
// expression keeps NumPy's order of operations (x ** 2 is x * x there, ** 1.5 is the maths library's pow), all arithmetic is float64 and
// floating-point contraction is switched off.  Host and device then differ from NumPy by their maths library's sin / cos / tan / pow
// only; r, theta, phi, t, mino, vr, vth and dtau are copies or sign flips of the tracer's samples and carry its bits.  Nothing is
// clamped: NaN and inf are written where NumPy produces them.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define REC_HD __host__ __device__ __forceinline__
#else
#define REC_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define REC_BLOCK 256        // sample points per workgroup of the pointwise pass
#define REC_RAY_BLOCK 64     // rays per workgroup of the cumulative sum: one lane per ray
#define REC_SAMPLE_ROWS 7    // rows of the tracer's samples: mino, r, theta, phi, t, vr, vth (geodesics.SAMPLE_ROWS)
#define REC_FIELDS 18        // per-point outputs

// The 18 per-point outputs, (n, ngeo) row-major each, in the order of include/bhnerf_rec.h.
struct RecFields {
    double *r, *theta, *phi, *t, *mino, *Delta, *Sigma, *Xi, *omega, *x, *y, *z, *R, *Theta, *vr, *vth, *dtau, *affine;
};

// What one point holds apart from dtau and affine, which are its ray's
struct RecPoint {
    double r, theta, phi, t, mino, Delta, Sigma, Xi, omega, x, y, z, R, Theta, vr, vth;
};

// radial_potential(r, a, lam, eta, M)
REC_HD double rec_radial_potential(double r, double a, double lam, double eta, double M) {
    const double Delta = r * r - 2.0 * M * r + a * a;
    const double P = r * r + a * a - a * lam;
    const double d = lam - a;
    return P * P - Delta * (eta + d * d);
}

// angular_potential(theta, a, lam, eta)
REC_HD double rec_angular_potential(double theta, double a, double lam, double eta) {
    const double c = cos(theta), tn = tan(theta);
    return eta + a * a * (c * c) - lam * lam / (tn * tn);
}

// _build_record at one point: s_* are the tracer's sample rows there (forward equations: mino, phi and t are negated here)
REC_HD RecPoint rec_point(double s_mino, double s_r, double s_theta, double s_phi, double s_t, double s_vr, double s_vth, double lam,
                          double eta, double spin, double M) {
    RecPoint p;
    const double a = spin * M;
    const double r = s_r, th = s_theta;
    p.r = r;
    p.theta = th;
    p.phi = -s_phi;
    p.t = -s_t;
    p.mino = -s_mino;
    // kerr_functions(r, theta, spin, M)
    const double a2 = a * a;
    const double c = cos(th), s = sin(th);
    p.Delta = r * r - 2.0 * M * r + a2;
    p.Sigma = r * r + a2 * (c * c);
    const double q = r * r + a2;
    p.Xi = q * q - p.Delta * a2 * (s * s);
    p.omega = 2.0 * a * M * r / p.Xi;
    p.x = r * s * cos(p.phi);
    p.y = r * s * sin(p.phi);
    p.z = r * c;
    p.R = rec_radial_potential(r, a, lam, eta, M);
    p.Theta = rec_angular_potential(th, a, lam, eta);
    p.vr = s_vr;
    p.vth = s_vth;
    return p;
}

// dtau of a ray from the first sample's record value mino[.., 0]:  -mino[..., :1] * ones
REC_HD double rec_dtau(double mino0) { return -mino0 * 1.0; }

// Point p = ray * ngeo + k of a (7, n, ngeo) sample buffer -> every output but affine.  total = n * ngeo.
REC_HD void rec_build_point(const double *samples, const double *lam, const double *eta, long long p, int ngeo, long long total, double spin,
                            double M, const RecFields &o) {
    const long long ray = p / ngeo;
    const RecPoint v = rec_point(samples[p], samples[total + p], samples[2 * total + p], samples[3 * total + p], samples[4 * total + p],
                                 samples[5 * total + p], samples[6 * total + p], lam[ray], eta[ray], spin, M);
    o.r[p] = v.r; o.theta[p] = v.theta; o.phi[p] = v.phi; o.t[p] = v.t; o.mino[p] = v.mino;
    o.Delta[p] = v.Delta; o.Sigma[p] = v.Sigma; o.Xi[p] = v.Xi; o.omega[p] = v.omega;
    o.x[p] = v.x; o.y[p] = v.y; o.z[p] = v.z;
    o.R[p] = v.R; o.Theta[p] = v.Theta; o.vr[p] = v.vr; o.vth[p] = v.vth;
    o.dtau[p] = rec_dtau(-samples[ray * ngeo]);
}

// affine = -np.cumsum(Sigma * dtau, axis=-1) of one ray, in np.cumsum's order: sample 0 first, one product then one add per sample
REC_HD void rec_affine_ray(const double *Sigma, const double *dtau, double *affine, long long ray, int ngeo) {
    const long long row = ray * ngeo;
    double acc = 0.0;
    for (int k = 0; k < ngeo; ++k) {
        const double term = Sigma[row + k] * dtau[row + k];
        acc = k == 0 ? term : acc + term;
        affine[row + k] = -acc;
    }
}

// alma.image_plane_model's Omega at one point:  (factor * sqrt_M) / (r ** 1.5 + spin * sqrt_M); the two products are the caller's
REC_HD double rec_kepler(double r, double factor_sqrt_M, double spin_sqrt_M) { return factor_sqrt_M / (pow(r, 1.5) + spin_sqrt_M); }

// Why the sizes are outside the contract, or NULL.  Host only.
inline const char *rec_sizes_error(long long n, int ngeo) {
    if (n < 1) return "ray count n must be at least 1";
    if (ngeo < 1) return "ngeo must be at least 1";
    return nullptr;
}
