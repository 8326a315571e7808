/*
 * mckpp_hip_put.h - the prognostic state set or incremented in place from arrays in device (or host) memory.
 *
 * A companion of mckpp_hip_device.h and the inverse of mckpp_hip_fetch_dev: that call takes fields out on the device,
 * this one writes U, V, T and S of a resident run between two launches - a learned correction every coupling interval,
 * an analysis increment, SST and SSS overwritten under ice, a few columns re-seeded - without the download, host edit
 * and mckpp_hip_upload that the edit otherwise costs, and without what the upload cancels:
 *
 *     for every coupling interval w:
 *       mckpp_hip_step(h, 1 + w * K, K);                       K steps, one launch
 *       ... the caller's kernels on s: the increment dT(npts, nzp1) from the state the partner holds ...
 *       mckpp_hip_put_dev(h, 1, &plane_T_add, s);              T = T + dT, behind those kernels, on the device
 *       mckpp_hip_dev_fence(h, s);                             s may rewrite dT once the library has read it
 *
 * Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued, streams passed as
 * void *, no host wait apart from the turn of the pinned image of the plane table.
 *
 * What a put leaves alone: the output schedules and their bookkeeping, exports, the restart schedule and its snapshots,
 * the step log, the flux ring or series, the ancillary series and schedules, a resident bottom temperature, the column
 * map and the diagnostics - these stay those of the last step, as in the reference after a host edit of U / X.  A put
 * belongs between launches: it is queued on the context's stream, behind every launch already queued there.
 *
 * The contract on the caller's arrays is mckpp_hip_fluxes_dev's: arrays handed to mckpp_hip_put_dev are read by a
 * kernel that runs later and must stay allocated and unchanged until mckpp_hip_dev_fence on the stream that next writes
 * or frees them, or until mckpp_hip_synchronize.  mckpp_hip_put_host returns when the state has been written.
 */
#ifndef MCKPP_HIP_PUT_H
#define MCKPP_HIP_PUT_H

#include "mckpp_hip_device.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MCKPP_PUT_SET = 0, MCKPP_PUT_ADD = 1 };                   /* op */
enum { MCKPP_PUT_SKIP = 1, MCKPP_PUT_TIME_LEVELS = 2 };          /* flags, a bit mask */

/* One plane of a put: in(npts, nlev), points fastest, doubles (dtype MCKPP_EXP_F64) or floats (MCKPP_EXP_F32, widened
 * exactly before anything else), for levels lev0 .. lev0 + nlev - 1 (0-based) of state field `field` on the axis
 * mckpp_hip_window_fetch documents: mckpp_dev_plane_c turned round.  Values at points that are no resident column are
 * never used.
 *
 * Fields: MCKPP_OUT_U, _V, _T, _S_ANOM (X(:,:,2) itself) and _S (X(:,:,2) + Sref).  Every other output field is refused
 * by number: it is an output of the step, not state.
 *
 * Arithmetic, each line one correctly rounded fp64 operation on the element x and the widened value v:
 *     op SET:              x = v            field S:  X2 = v - Sref   (the inverse of the X2 + Sref a fetch forms)
 *     op ADD:              x = x + v        field S:  X2 = X2 + v
 *
 * flags & MCKPP_PUT_SKIP: an element whose widened value compares == to skip_value leaves the state element untouched -
 * a plane mckpp_hip_fetch_dev filled with a land value, the points a partner does not correct.  A NaN skip_value is
 * refused with the flag; without the flag skip_value is not read.
 *
 * flags & MCKPP_PUT_TIME_LEVELS: the operation is also applied to both saved time levels of the field, Us / Xs(:,:,0:1).
 * SET makes both equal to the value written to the profile, which is what mckpp_initialize_ocean_model seeds; ADD adds v
 * to each.  Without the flag only U / X change, and the next step's first guess 2 Xs(new) - Xs(old) is formed from the
 * values before the put: what the reference does when a host edits X alone.
 *
 * Where a plane writes a column's element at level 0 (lev0 == 0, not skipped), the surface reference of the field
 * follows, as the end of the reference's ocnstep states it: uref = U(1,1), vref = U(1,2), Tref = X(1,1) and Ssurf =
 * X(1,2) + Sref - unless L_SSref, where Ssurf stays SSref. */
typedef struct { int32_t field, lev0, nlev, dtype, op, flags; double skip_value; const void *in; } mckpp_put_plane_c;
#define MCKPP_PUT_PLANES_MAX 64

/* Applies nplanes <= MCKPP_PUT_PLANES_MAX planes in one launch on the context's stream: behind everything already
 * queued there and behind what producer_stream had queued at the call.  Behind the launch the event is recorded that
 * mckpp_hip_dev_fence makes a stream wait for.
 * Refused before anything is queued, with the state, the schedules and their bookkeeping untouched, by a message that
 * names this function and planes[k]: no state uploaded; nplanes outside 0 .. MCKPP_PUT_PLANES_MAX or a null table; an
 * unknown or non-state field; a level range outside the axis (nlev < 1 included); an unknown dtype, op or flag bit; a
 * NaN skip value; two planes of the call that touch the same field and overlapping levels (S and S_ANOM are one field
 * here) - the planes of a call have no order -; and an `in` that is null, host memory - pinned or not -, too small for
 * npts * nlev elements, or memory the context's device cannot reach. */
int mckpp_hip_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_put_plane_c *planes, void *producer_stream);

/* The same from arrays in host memory (`in` must not be null): every plane is copied into device staging on the
 * context's stream, the same launch follows, and the call waits for it, as the other host setters do.  The staging is
 * grow-only and goes with the resident state. */
int mckpp_hip_put_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_put_plane_c *planes);

/* All shards with the same table: every plane of every shard is checked before any shard queues; a shard takes the
 * full-size arrays and writes only its own columns, so every state element is written once.  One event on the caller's
 * stream orders every shard.  In the host form each shard stages the whole plane. */
int mckpp_hip_multi_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_put_plane_c *planes, void *producer_stream);
int mckpp_hip_multi_put_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_put_plane_c *planes);

#ifdef __cplusplus
}
#endif
#endif
