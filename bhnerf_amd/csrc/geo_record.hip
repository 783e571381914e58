// libbhnerf_rec.so: the geodesic record of geodesics._build_record from the tracer's samples, and the Keplerian Omega of
// alma.image_plane_model, on the device -- what lets a record be created where the tracer left its samples and stay there.
//
// bhn_rec_build is two launches on the caller's stream (geo_record.h holds the per-point arithmetic, shared with the CPU build of
// tools/geo_record_host.cpp):
//   rec_point_kernel   one lane per sample point, workgroups of REC_BLOCK = 256 lanes over the n * ngeo points.  Point p reads the seven
//                      sample rows at p (consecutive lanes, consecutive doubles) and its ray's lam, eta and first Mino sample, and writes
//                      every output but affine at p.
//   rec_affine_kernel  one lane per ray, workgroups of REC_RAY_BLOCK = 64 lanes: the lane walks its ray from sample 0 and writes
//                      affine = -cumsum(Sigma * dtau) in np.cumsum's order, reading the Sigma and dtau the first launch wrote.  A lane's
//                      consecutive samples share cache lines; the pass moves 3 of the record's 25 doubles per point.
// bhn_rec_kepler is one lane per point.  No LDS, no atomics, no cross-lane operation.  All arithmetic is float64.
//
// Built into a library of its own (include/bhnerf_rec.h): the ABIs of the other six libraries are not touched.
#include <hip/hip_runtime.h>

#include "../../include/bhnerf_rec.h"
#include "geo_record.h"
#include "side_lib.h"

extern "C" const char *bhn_rec_last_error(void) { return side_last_error(); }

__global__ __launch_bounds__(REC_BLOCK) void rec_point_kernel(const double *__restrict__ samples, const double *__restrict__ lam,
                                                              const double *__restrict__ eta, int ngeo, long long total, double spin, double M,
                                                              RecFields out) {
    const long long p = (long long)blockIdx.x * REC_BLOCK + threadIdx.x;
    if (p >= total) return;
    rec_build_point(samples, lam, eta, p, ngeo, total, spin, M, out);
}

__global__ __launch_bounds__(REC_RAY_BLOCK) void rec_affine_kernel(const double *__restrict__ Sigma, const double *__restrict__ dtau,
                                                                   double *__restrict__ affine, long long n, int ngeo) {
    const long long ray = (long long)blockIdx.x * REC_RAY_BLOCK + threadIdx.x;
    if (ray >= n) return;
    rec_affine_ray(Sigma, dtau, affine, ray, ngeo);
}

__global__ __launch_bounds__(REC_BLOCK) void rec_kepler_kernel(const double *__restrict__ r, long long count, double factor_sqrt_M,
                                                               double spin_sqrt_M, double *__restrict__ Omega) {
    const long long p = (long long)blockIdx.x * REC_BLOCK + threadIdx.x;
    if (p >= count) return;
    Omega[p] = rec_kepler(r[p], factor_sqrt_M, spin_sqrt_M);
}

extern "C" int bhn_rec_build(const double *samples, const double *lam, const double *eta, int64_t n, int32_t ngeo, double spin, double M,
                             const bhn_rec_fields *out, void *stream) {
    BHN_CHECK_ARG(samples, "null samples");
    BHN_CHECK_ARG(lam && eta, "null lam or eta");
    BHN_CHECK_ARG(out, "null out");
    double *const fields[REC_FIELDS] = {out->r, out->theta, out->phi, out->t, out->mino, out->Delta, out->Sigma, out->Xi, out->omega,
                                        out->x, out->y, out->z, out->R, out->Theta, out->vr, out->vth, out->dtau, out->affine};
    for (int i = 0; i < REC_FIELDS; ++i) BHN_CHECK_ARG(fields[i], "null output field %d of out", i);
    const char *why = rec_sizes_error((long long)n, ngeo);
    BHN_CHECK_ARG(!why, "%s (n %lld, ngeo %d)", why, (long long)n, ngeo);
    // 7 n ngeo doubles of samples stay far inside 2^63 bytes
    const long long blocks = n > ((int64_t)1 << 40) / ngeo ? 0 : side_blocks((long long)n * ngeo, REC_BLOCK);
    BHN_CHECK_ARG(blocks > 0, "too many points (n %lld, ngeo %d) for one launch", (long long)n, ngeo);
    const long long ray_blocks = side_blocks((long long)n, REC_RAY_BLOCK);
    BHN_CHECK_ARG(ray_blocks > 0, "too many rays (n %lld) for one launch", (long long)n);
    RecFields o;
    o.r = out->r; o.theta = out->theta; o.phi = out->phi; o.t = out->t; o.mino = out->mino; o.Delta = out->Delta; o.Sigma = out->Sigma;
    o.Xi = out->Xi; o.omega = out->omega; o.x = out->x; o.y = out->y; o.z = out->z; o.R = out->R; o.Theta = out->Theta; o.vr = out->vr;
    o.vth = out->vth; o.dtau = out->dtau; o.affine = out->affine;
    const long long total = (long long)n * ngeo;
    hipLaunchKernelGGL(rec_point_kernel, dim3((unsigned)blocks), dim3(REC_BLOCK), 0, (hipStream_t)stream, samples, lam, eta, (int)ngeo, total,
                       spin, M, o);
    if (int rc = side_launched("rec_point_kernel")) return rc;
    hipLaunchKernelGGL(rec_affine_kernel, dim3((unsigned)ray_blocks), dim3(REC_RAY_BLOCK), 0, (hipStream_t)stream, (const double *)o.Sigma,
                       (const double *)o.dtau, o.affine, (long long)n, (int)ngeo);
    return side_launched("rec_affine_kernel");
}

extern "C" int bhn_rec_kepler(const double *r, int64_t count, double spin, double M, double factor, double *Omega, void *stream) {
    BHN_CHECK_ARG(r, "null r");
    BHN_CHECK_ARG(Omega, "null output Omega");
    BHN_CHECK_ARG(count >= 1, "count must be at least 1, not %lld", (long long)count);
    const long long blocks = side_blocks((long long)count, REC_BLOCK);
    BHN_CHECK_ARG(blocks > 0, "too many points (%lld) for one launch", (long long)count);
    const double sqrt_M = sqrt(M);
    hipLaunchKernelGGL(rec_kepler_kernel, dim3((unsigned)blocks), dim3(REC_BLOCK), 0, (hipStream_t)stream, r, (long long)count, factor * sqrt_M,
                       spin * sqrt_M, Omega);
    return side_launched("rec_kepler_kernel");
}
