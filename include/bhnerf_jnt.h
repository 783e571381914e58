/*
 * bhnerf_jnt.h -- C ABI of libbhnerf_jnt.so: the fan-in of a joint training step (optimization.TrainStep.joint), on the MI355X
 * (gfx950): up to eight float32 vectors of one length added element by element in ONE launch and in one defined order, and the
 * terms' device-resident losses gathered into one vector with their sum.
 *
 * A library of its own, beside the other side libraries: their ABIs stay exactly what they are.  The conventions are those of
 * include/bhnerf_reg.h: 0 on success or a BHN_E* code (the last-error call of this header gives a thread-local message; nothing
 * aborts, nothing prints); the CALLER owns every buffer, what an output holds on entry is irrelevant, every element of an output
 * is written and nothing outside the sizes named here is; no allocation, no synchronisation, no environment reads, no state but
 * the error string; all work is enqueued on `stream` (a hipStream_t passed as void*) of the calling thread's current device and
 * can be captured into a graph.
 *
 * The sum.  dst[i] = ((src[0][i] + src[1][i]) + ... + src[K-1][i]) for i < n, in float32, left to right: one correctly rounded
 * IEEE addition after the other, subnormals kept, nothing fused or reassociated; K = 1 copies.  The K pointers travel BY VALUE in
 * the struct: there is no pointer table in device memory.  dst may be equal to any src[k] (an element is read before it is
 * written, by the same lane); a dst that overlaps a src[k] without being equal to it is refused.
 *
 * The losses.  With loss_out not NULL: loss_out[1 + k] = *loss_in->p[k] for k < K, and loss_out[0] their sum, left to right from
 * loss_in->p[0].  One lane of workgroup 0 reads the K values, then writes the K + 1 floats with ordinary stores; loss_in->p[k]
 * may therefore point into loss_out.  loss_out must not overlap dst.  n == 0 with losses only is allowed: the src pointers must
 * still be non-null and aligned (they are not read), dst may be NULL.
 *
 * The launch.  Workgroups of 256 lanes, grid-stride, at most BHN_JNT_MAX_BLOCKS workgroups.  When dst and every src[k] are
 * 16-byte aligned a lane moves four elements per trip with 16-byte loads and stores and workgroup 0 takes the n % 4 elements of
 * the tail one by one; otherwise (a slice such as buf + 1) every element goes one by one.  The result does not depend on the
 * path: an element's sum is the same K - 1 additions in either.
 */
#ifndef BHNERF_JNT_H
#define BHNERF_JNT_H

#include "bhnerf_hip.h"        /* BHN_API, BHN_OK / BHN_EINVAL / BHN_EHIP */

#ifdef __cplusplus
extern "C" {
#endif

#define BHN_JNT_MAX_TERMS 8
#define BHN_JNT_MAX_BLOCKS 1024        /* the cap of the grid: 4 workgroups of 256 lanes per compute unit of an MI355X */

/* K device pointers, the entries from K on are ignored */
typedef struct bhn_jnt_ptrs {
    const float *p[BHN_JNT_MAX_TERMS];
} bhn_jnt_ptrs;

BHN_API const char *bhn_jnt_last_error(void);

/* src->p[k] (n floats each), dst (n floats) and, with loss_out (K + 1 floats), loss_in->p[k] (one float each) are DEVICE
 * pointers; src and loss_in themselves are HOST structs, read before the call returns.
 * BHN_EINVAL before any device call: K outside [1, BHN_JNT_MAX_TERMS]; n < 0 or beyond 2^40; a null src or src->p[k]; a null dst
 * with n > 0; with loss_out set a null loss_in or loss_in->p[k]; a pointer that is not 4-byte aligned; a dst that overlaps a
 * src->p[k] partially; a loss_out that overlaps dst.  n == 0 without loss_out does nothing and succeeds. */
BHN_API int bhn_jnt_sum(const bhn_jnt_ptrs *src, int32_t K, int64_t n, float *dst,
                const bhn_jnt_ptrs *loss_in,    /* K pointers to one float each, or NULL when loss_out is NULL */
                float *loss_out,                /* K + 1 floats: total, then the terms; or NULL: no losses     */
                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BHNERF_JNT_H */
