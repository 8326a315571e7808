/*
 * mckpp_hip_vrecords.h - completed records of output schedules on the caller's levels: interval means (and minima,
 * maxima, last steps) out through a vertical axis, at the model's points or on a caller grid.
 *
 * A companion of mckpp_hip_vaxis.h, mckpp_hip_device_records.h and mckpp_hip_remap.h, and the last row of the table:
 *
 *                                                      model points             caller grid
 *     last step's instant, model levels                mckpp_hip_fetch_dev      mckpp_hip_hgrid_fetch_dev
 *     last step's instant, caller levels               mckpp_hip_vaxis_fetch_dev mckpp_hip_hv_fetch_dev
 *     completed record, model levels                   mckpp_hip_records_dev    mckpp_hip_remap_records_dev
 *     completed record, caller levels                  mckpp_hip_vrecords_vaxis_dev / _host   mckpp_hip_vrecords_hv_dev
 *
 * A coupler exchanges the mean over the coupling interval; a partner on its own levels takes it here:
 *
 *     mckpp_hip_vaxis_define(h, 0, n_axis, z);
 *     mckpp_hip_window_schedule_zoom(h, 0, 1, K, 1, {T}, {MEAN}, 1, &top_30_levels);     one record: nrec = 1
 *     for every coupling interval w:
 *       mckpp_hip_step(h, 1 + w * K, K);                          record w is complete
 *       mckpp_hip_vrecords_vaxis_dev(h, 1, &mean_T_on_my_levels, s);
 *       mckpp_hip_window_record_release(h, 0, w);                 at once
 *       ... the partner's kernels on s ...
 *
 * and a host writes daily means on standard depths (XIOS's interpolate_axis in a <file>) with
 * mckpp_hip_vrecords_vaxis_host.
 *
 * No arithmetic is restated here.  The record's value is mckpp_hip_records_dev's, the interpolation is
 * mckpp_hip_vaxis.h's vinterp, the row sum is mckpp_hip_hgrid.h's, every operation one correctly rounded fp64
 * operation.  What is stated here is the ORDER of them and which values each reads.  The device, the host restatement
 * (mckpp_hip_window_record_fetch, mckpp_host_vaxis_map, mckpp_host_hgrid_apply) and several shards give the same bits.
 *
 * The order: RECORD VALUE FIRST, THEN VERTICAL, then - on a caller grid - horizontal.  The source value at a row and a
 * model level is mckpp_hip_records_dev's double for that schedule, record, field and op, bit for bit; a mean is
 * sum / (double)period, formed before anything else.  S is what the record holds - Sref is in it already -, nothing is
 * added a second time.  The caller level's value is vinterp through the entry of the axis's out table: a clamp (ABOVE,
 * BELOW) reads one source level, a bracket reads two and takes the four operations of mckpp_hip_vaxis.h, one rounded
 * operation per line.  A float plane is one final conversion.
 *
 * So interpolating a record of minima (or maxima) gives the interpolation of the minima, NOT the minimum of the
 * interpolated series: the two bracket values may come from different steps.  And the mean of the interpolated steps
 * equals the value delivered here in exact arithmetic only - interpolation is linear, rounding is not.
 *
 * Level zooms.  A schedule with a zoom_axis keeps model levels lev0 .. lev0 + nlev - 1 of a field.  A plane is accepted
 * if and only if every model level that the axis's out table reads, for any caller level, is a kept level
 * (mckpp_host_vrecords_rule); otherwise it is refused before anything is queued, by a message that names planes[k], the
 * first offending caller level, the model level it reads and the kept range.  A partner that lives in the top 300 m
 * keeps a ring of 30 levels; a schedule of one kept level serves an axis whose entries all read that one level.
 *
 * Out of scope: reduced records (mckpp_hip_reduce.h) on a caller grid or axis; mckpp_hip_vaxis_init_profiles from a
 * caller grid; fields on the interface axis 0..nz; a host form on a caller grid - a host caller composes
 * mckpp_hip_vrecords_vaxis_host with mckpp_host_hgrid_apply.
 *
 * Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued, streams passed as
 * void *, a refusal leaves state, schedules, records, grids, axes and arrays untouched and names the function and
 * planes[k].
 */
#ifndef MCKPP_HIP_VRECORDS_H
#define MCKPP_HIP_VRECORDS_H

#include "mckpp_hip_vaxis.h"
#include "mckpp_hip_device_records.h"
#include "mckpp_hip_remap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_VRECORDS_PLANES_MAX 64

/* The level rule, HIP-free.  branch[nt], kin[nt]: the out table of a caller axis of nt levels (mckpp_host_vaxis_map
 * with zm(1:nzp1) as the source); lev0, nlev: the model levels lev0 .. lev0 + nlev - 1 a schedule keeps.  Returns 0 if
 * every level read - kin, and kin + 1 of a bracket - is kept; 1 otherwise, with the first offending caller level in
 * *caller_level and the first model level it reads that is not kept in *model_level (either may be null); -1 for a
 * null table, nt < 1 or nlev < 1. */
int mckpp_host_vrecords_rule(int32_t nt, const int32_t *branch, const int32_t *kin, int32_t lev0, int32_t nlev,
                             int32_t *caller_level, int32_t *model_level);

/* ---- a completed record's plane on a caller axis, at the record's points ---- */

/* Operation `op` (0 mean, 1 min, 2 max, 3 last) of field `field` in record `rec` of schedule `sched`, delivered as
 * out(npoints, n_axis) on caller axis `axis`, points fastest, doubles (MCKPP_EXP_F64) or floats (MCKPP_EXP_F32).  It
 * covers the whole caller axis; its point axis is the schedule's - the grid, or a zoom's point list in list order -
 * exactly as mckpp_hip_records_dev has it, and so are fill_land and land_value: a position that is no row of the record
 * gets land_value at every caller level, or keeps what `out` held.  Fields are mckpp_hip_vaxis_fetch_dev's:
 * three-dimensional fields on the levels axis 1..nzp1 only. */
typedef struct { int32_t sched, field, op, axis, dtype, fill_land; int64_t rec; double land_value; void *out; }
    mckpp_vaxis_record_plane_c;

/* Delivers nplanes <= MCKPP_VRECORDS_PLANES_MAX planes, of any schedules, records and axes, in one launch on the
 * context's stream with mckpp_hip_records_dev's ordering: behind the launches that completed the records and behind what
 * consumer_stream had queued at the call; consumer_stream waits for it.  mckpp_hip_window_record_release, and the launch
 * that overwrites the ring slot, may follow at once.
 * Refused before anything is queued: everything mckpp_hip_records_dev refuses (the count or a null table; a schedule
 * that is unknown or not set; a record that is incomplete or released - its steps are named -; a field or op the
 * schedule does not keep; an unknown dtype; an `out` that is null, host memory, unreachable), an undefined axis, a
 * two-dimensional or interface-axis field, by name, an axis that reads a level the schedule does not keep (above), and
 * an `out` too small for npoints * n_axis elements. */
int mckpp_hip_vrecords_vaxis_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes,
                                 void *consumer_stream);

/* The same planes with `out` in host memory (null is refused; the size is the caller's to get right).  Staged on the
 * device and copied on the context's stream; returns when the arrays are written, like mckpp_hip_records_reduce_host
 * and mckpp_hip_put_host.  With fill_land == 0 the whole array goes up to the staging first, so that the positions
 * without a row come back as they were: such a plane crosses the bus twice.  An array of at least 256 KiB is registered (hipHostRegister) at its first use, like the
 * arrays of mckpp_hip_window_record_fetch, and stays so until mckpp_hip_release_host_arrays: it must not be freed
 * before.  XIOS's interpolate_axis for a host output path. */
int mckpp_hip_vrecords_vaxis_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes);

/* ---- ... and on a caller grid: vertical first, at the record's rows; then horizontal ---- */

/* The plane above with caller grid `grid` and `norm`: out(n_grid, n_axis) on the caller's points.  The value at a row
 * of the record and caller level j is the one stated above; from there on it is mckpp_hip_remap_records_dev's, at caller
 * level j: the row sum over the used entries - those whose model point is a ROW OF THE RECORD, the resident columns or
 * the listed resident columns of a zoomed schedule -, norm, land_value and fill_land as mckpp_hip_hgrid_fetch_dev has
 * them, a float plane one final conversion. */
typedef struct { int32_t sched, field, op, axis, dtype, grid, norm, fill_land; int64_t rec; double land_value; void *out; }
    mckpp_hv_record_plane_c;

/* Two launches on the context's stream, like mckpp_hip_remap_records_dev: the records' rows onto the caller's levels
 * into the internal staging plane (npts, n_axis) of doubles, then every caller point's row sum from it; ordering as
 * above, consumer_stream waits for the second.  The device table of a listed schedule on a grid is built on first use
 * and is mckpp_hip_remap_records_dev's.
 * Refused before anything is queued: what mckpp_hip_vrecords_vaxis_dev refuses of the record, the field and the axis,
 * and what mckpp_hip_remap_records_dev refuses of the grid, the norm and the array (an undefined grid, a missing out
 * table, a grid defined for another npts, an unknown norm, planes whose out arrays overlap, an out that is null, host
 * memory, unreachable or too small for n_grid * n_axis elements). */
int mckpp_hip_vrecords_hv_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_record_plane_c *planes, void *consumer_stream);

/* All shards with the same table; every shard is checked before any shard queues.  vaxis_dev and vaxis_host:
 * mckpp_hip_multi_records_dev's rule - a shard writes its own rows of the full-size array, shard 0 also the positions no
 * shard holds.  hv_dev: mckpp_hip_multi_remap_records_dev's - every shard's first launch writes shard 0's staging and
 * shard 0 alone runs the second over the rows of any shard.  One context and several shards give the same bits. */
int mckpp_hip_multi_vrecords_vaxis_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes,
                                       void *consumer_stream);
int mckpp_hip_multi_vrecords_vaxis_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes);
int mckpp_hip_multi_vrecords_hv_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_record_plane_c *planes,
                                    void *consumer_stream);

#ifdef __cplusplus
}
#endif
#endif
