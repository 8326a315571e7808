/*
 * mckpp_hip_remap.h - the caller's horizontal grids, second half: interval means out and state increments in on
 * points that are not the model's.
 *
 * A companion of mckpp_hip_hgrid.h, which carries forcing in and the last step's instant out on a caller grid.  A
 * coupler exchanges the mean over the coupling interval, and a partner on its own grid that corrects the ocean (a
 * learned increment, SST and SSS under ice) forms that correction on its own points.  The two calls here are
 * mckpp_hip_records_dev and mckpp_hip_put_dev through the weight tables of mckpp_hip_hgrid_define:
 *
 *     mckpp_hip_hgrid_define(h, 0, n_atm, &atm_to_ocean, &ocean_to_atm);
 *     mckpp_hip_window_schedule_zoom(h, 0, 1, K, 1, {T}, {MEAN}, 1, &level0);        one record: nrec = 1
 *     for every coupling interval w:
 *       mckpp_hip_step(h, 1 + w * K, K);                          record w is complete
 *       mckpp_hip_remap_records_dev(h, 1, &mean_sst_on_atm_grid, s);
 *       mckpp_hip_window_record_release(h, 0, w);                 at once
 *       ... the partner's kernels on s: eight flux fields and an increment dT(n_atm, nzp1) on its grid ...
 *       mckpp_hip_hgrid_fluxes_dev(h, 0, nt, fields, 0, flsn, el, s);
 *       mckpp_hip_remap_put_dev(h, 1, &plane_T_add, s);           T = T + (in table) dT
 *       mckpp_hip_dev_fence(h, s);
 *
 * The arithmetic is the one statement of mckpp_hip_hgrid.h, unchanged: a row's sum starts as a = w * x of its first
 * used entry and adds a = a + w * x for each further used entry in entry order, every * and + one correctly rounded
 * fp64 operation.  What is stated here is which entries are used and what happens to the sum.  The device, the host
 * functions of mckpp_hip_hgrid.h and several shards give the same bits.
 *
 * There is no host form: a host caller remaps with mckpp_host_hgrid_apply and calls mckpp_hip_window_record_fetch or
 * mckpp_hip_put_host.  Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued,
 * streams passed as void *, a refusal leaves state, schedules, records and grids untouched and names the function and
 * planes[k].
 */
#ifndef MCKPP_HIP_REMAP_H
#define MCKPP_HIP_REMAP_H

#include "mckpp_hip_hgrid.h"
#include "mckpp_hip_device_records.h"
#include "mckpp_hip_put.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a completed record's plane on a caller grid ---- */

/* mckpp_dev_record_plane_c's plane - operation `op` (0 mean, 1 min, 2 max, 3 last) of field `field` in record `rec` of
 * schedule `sched`, levels lev0 .. lev0 + nlev - 1 of the levels the schedule keeps - delivered as out(n, nlev) on caller
 * grid `grid`, points fastest, doubles (MCKPP_EXP_F64) or floats (MCKPP_EXP_F32).
 *
 * The source value x at a model point and level is mckpp_hip_records_dev's double for that point, bit for bit; the mean
 * is sum / (double)period.  From there on it is the `out` direction of mckpp_hip_hgrid.h: the row sum a over the used
 * entries, norm MCKPP_HGRID_NORM_NONE (the value is a) or MCKPP_HGRID_NORM_USED (a / d, d the used weights summed in the
 * same order; d == 0.0 counts as no used entry), a caller point with no used entry gets land_value where fill_land != 0
 * and keeps what `out` held otherwise, and a float plane is one final conversion.
 *
 * The USED entries of a row are those whose model point is a ROW OF THE RECORD: for a schedule without a point list the
 * resident columns (mckpp_hip_hgrid_fetch_dev's rule), for a schedule with a zoom point list the listed resident
 * columns - a regional box or a set of moorings remaps from what the record holds and from nothing else.  Under a multi
 * handle: the rows of any shard. */
typedef struct { int32_t sched, field, op, lev0, nlev, dtype, grid, norm, fill_land; int64_t rec; double land_value; void *out; }
    mckpp_remap_record_plane_c;
#define MCKPP_REMAP_PLANES_MAX 64

/* Delivers nplanes <= MCKPP_REMAP_PLANES_MAX planes, of any schedules, records and grids.  Ordering is
 * mckpp_hip_records_dev's: two launches on the context's stream - the records' rows into an internal staging plane
 * (npts, nlev) of doubles, then every caller point's row sum from it - behind the launches that completed the records
 * and behind what consumer_stream had queued at the call; consumer_stream waits for the second.  So
 * mckpp_hip_window_record_release may follow the call at once, and so may the launch that overwrites the ring slot.
 * Refused before anything is queued: everything mckpp_hip_records_dev refuses of the plane (a schedule that is not set,
 * a record that is incomplete or released - its steps are named -, a field or op the schedule does not keep, the level
 * range, the dtype) and everything mckpp_hip_hgrid_fetch_dev refuses (an undefined grid, a missing out table, a grid
 * defined for another npts, an unknown norm, planes whose out arrays overlap, an out that is null, host memory,
 * unreachable or too small for n * nlev elements).
 * The device table of a listed schedule on a grid is built on first use and goes with the schedule and with the grid. */
int mckpp_hip_remap_records_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_remap_record_plane_c *planes, void *consumer_stream);

/* ---- U, V, T, S set or incremented from planes on a caller grid ---- */

/* mckpp_put_plane_c's plane with in(n, nlev) on caller grid `grid`, points fastest; floats are widened exactly before
 * anything else.  For resident column c and level lev the value v is the row sum of the column's `in` row over level lev
 * of the plane: the `in` direction of mckpp_hip_hgrid.h - all entries count, the first assigns, the rest add in entry
 * order.  What then happens to v is mckpp_hip_put.h's, unchanged: op SET or ADD, field S against S_ANOM,
 * MCKPP_PUT_TIME_LEVELS, and the surface references that follow level 0.
 *
 * flags & MCKPP_PUT_SKIP: a state element (column, level) is left untouched if ANY entry of the column's row reads, at
 * that level, a value that compares == to skip_value - mckpp_hip_vaxis_put_dev's rule for the values its branch reads.
 * A plane that mckpp_hip_hgrid_fetch_dev filled with a land value therefore comes back harmless.  The sum itself is
 * never compared.
 *
 * An EMPTY `in` row of a resident column leaves that column untouched, under SET and under ADD, with or without SKIP: a
 * partner corrects the points it covers.  This differs from mckpp_hip_hgrid_fluxes_dev and _flux_ring_put_dev, which
 * refuse an empty row: forcing is required, an increment is not. */
typedef struct { int32_t field, lev0, nlev, dtype, op, flags, grid; double skip_value; const void *in; } mckpp_remap_put_plane_c;

/* Applies nplanes <= MCKPP_REMAP_PLANES_MAX planes in one launch on the context's stream, behind everything queued
 * there and behind what producer_stream had queued at the call; the event mckpp_hip_dev_fence waits on is recorded
 * behind it.  It cancels nothing: what mckpp_hip_put_dev leaves alone, this leaves alone.
 * Refused before anything is queued: what mckpp_hip_put_dev refuses (no state uploaded; nplanes outside
 * 0 .. MCKPP_REMAP_PLANES_MAX or a null table; a non-state field, by number; a level range outside the axis; an unknown
 * dtype, op or flag bit; a NaN skip value with MCKPP_PUT_SKIP; two planes on the same field and overlapping levels, S
 * and S_ANOM being one field; an `in` that is null, host memory or unreachable), an undefined grid, a missing in table,
 * a grid defined for another npts, and an `in` too small for n * nlev elements. */
int mckpp_hip_remap_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_remap_put_plane_c *planes, void *producer_stream);

/* All shards with the same table; every shard is checked before any shard queues.  Records: every shard's first launch
 * writes shard 0's staging and shard 0 alone runs the second, with the rows of all shards as used, as
 * mckpp_hip_multi_hgrid_fetch_dev does - one context and several shards give the same bits.  Puts: every shard sums for
 * its own columns through its own in table. */
int mckpp_hip_multi_remap_records_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_remap_record_plane_c *planes,
                                      void *consumer_stream);
int mckpp_hip_multi_remap_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_remap_put_plane_c *planes,
                                  void *producer_stream);

#ifdef __cplusplus
}
#endif
#endif
