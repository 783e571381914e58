/*
 * bhnerf_reg.h -- C ABI of libbhnerf_reg.so: priors on a 3-D emission volume, on the MI355X (gfx950): the smoothed isotropic
 * total variation ('tv'), the total squared variation ('tsv') and the l1 norm ('l1') of N volumes on one regular lattice, with
 * the gradient in the volumes.
 *
 * A library of its own, beside the other side libraries: their ABIs stay exactly what they are.  The conventions are those of
 * include/bhnerf_pol.h: 0 on success or a BHN_E* code (the last-error call of this header gives a thread-local message; nothing
 * aborts, nothing prints); the CALLER owns every buffer, what an output or the workspace holds on entry is irrelevant, every
 * element of an output is written and nothing outside the sizes named here is; no allocation, no synchronisation, no
 * environment reads, no state but the error string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the
 * calling thread's current device and can be captured into a graph.
 *
 * The volumes.  e[n, i, j, k], n < N, dims (nx, ny, nz) in C order, k fastest: the order of np.meshgrid(.., indexing='ij')
 * coordinates flattened.  mask[i, j, k] in {0, 1} is shared by the N volumes, NULL means all ones.  spacing = (hx, hy, hz) > 0.
 *
 * The terms.  Differences are forward and masked: dx[v] = (e[i+1, j, k] - e[i, j, k]) / hx when i + 1 < nx and both voxels are
 * in the mask, else exactly 0 (a difference across the boundary of the domain is not counted); dy, dz alike; q = dx^2 + dy^2 +
 * dz^2.  In the canonical order tv, tsv, l1:
 *   tv   = sum_n sum_v m[v] sqrt(q[v] + eps^2)
 *   tsv  = sum_n sum_v m[v] q[v]
 *   l1   = sum_n sum_v m[v] |e[v]|
 *   loss = scale (w_tv tv + w_tsv tsv + w_l1 l1)
 * A term with weight 0 is absent: its loss slot and its per_volume row are exactly 0 and it puts no requirement on eps.  The
 * gradient in a masked-out voxel is exactly 0, sign(0) = 0, and what stands in the masked-out voxels of `volumes` is never read.
 * The effective weight of a term is scale * w_d, the product formed once in float64 on the host and rounded once to float32.
 * Every sum has one fixed order and there are no atomics: the result is bitwise reproducible, and the gradient of a volume and
 * its per_volume row do not depend on N or on where in the batch the volume stands.
 */
#ifndef BHNERF_REG_H
#define BHNERF_REG_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP / BHN_EWORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

BHN_API const char *bhn_reg_last_error(void);

/* Bytes of workspace a call with these sizes needs; 0 when a size is below 1 or too large for one call (a volume of more than
 * 2^31 - 1025 voxels).  The workspace must be 4-byte aligned. */
BHN_API size_t bhn_reg_ws_bytes(int32_t N, int32_t nx, int32_t ny, int32_t nz);

/* volumes (N, nx ny nz) float32 and mask (nx ny nz) uint8 are DEVICE pointers, spacing and weights HOST arrays of 3 floats.
 * loss[4] = {total, tv, tsv, l1} (device), each term scale w_d term_d with the volumes' sums added in order, total = tv + tsv +
 * l1; per_volume (3, N) (device, or NULL) the unscaled sums of each term per volume; dvolumes (N, nx ny nz) (device, or NULL:
 * no gradient is computed) = d total / d volumes.  workspace: bhn_reg_ws_bytes(N, nx, ny, nz) bytes.
 * BHN_EINVAL before any launch: a null volumes / spacing / weights / loss / workspace, a size below 1 or too large, a spacing that
 * is not positive and finite, a weight that is negative or not finite, a scale that is not finite, eps not positive and finite
 * while w_tv is not 0, a misaligned workspace.  BHN_EWORKSPACE before any launch: workspace_bytes too small. */
BHN_API int bhn_reg_loss(const float *volumes, int32_t N, int32_t nx, int32_t ny, int32_t nz,
                 const uint8_t *mask,            /* (nx ny nz) or NULL                                   */
                 const float spacing[3], const float weights[3], float eps, float scale,
                 float *loss,                    /* 4 floats: total, tv, tsv, l1 (each scale w_d term_d) */
                 float *per_volume,              /* (3, N) unscaled term sums per volume, or NULL        */
                 float *dvolumes,                /* (N, nx ny nz), or NULL: no gradient                  */
                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_REG_H */
