/*
 * mckpp_hip_hv.h - the caller's horizontal grid and the caller's vertical axis in one call: fields out, state in, on
 * points and levels that are both not the model's.
 *
 * A companion of mckpp_hip_remap.h and mckpp_hip_vaxis.h.  A learned correction, an analysis, an ice or atmosphere
 * model with a column of its own lives on its own points AND its own levels:
 *
 *     mckpp_hip_hgrid_define(h, 0, n_grid, &partner_to_ocean, &ocean_to_partner);
 *     mckpp_hip_vaxis_define(h, 0, n_axis, z);
 *     for every coupling interval:
 *       mckpp_hip_step(h, nt, K);
 *       mckpp_hip_hv_fetch_dev(h, 1, &plane_T_out, s);            T on the partner's points and levels
 *       ... the partner's kernels on s: the increment dT(n_grid, n_axis) ...
 *       mckpp_hip_hv_put_dev(h, 1, &plane_T_add, s);              T = T + vinterp((in table) dT), on the device
 *       mckpp_hip_dev_fence(h, s);
 *
 * No arithmetic is restated here.  The row sum is mckpp_hip_hgrid.h's - a = w * x of the first used entry, a = a + w * x
 * for each further one in entry order -, the interpolation is mckpp_hip_vaxis.h's vinterp, every operation one correctly
 * rounded fp64 operation.  What is stated here is the ORDER of the two and which values each reads.  Grids come from
 * mckpp_hip_hgrid_define and axes from mckpp_hip_vaxis_define, both unchanged.  The device, the host helpers
 * (mckpp_host_hgrid_apply, mckpp_host_vaxis_map) and several shards give the same bits.
 *
 * Out of scope: mckpp_hip_vaxis_init_profiles from a caller grid; a host form - a host caller composes
 * mckpp_host_hgrid_apply, mckpp_host_vaxis_map and mckpp_hip_put_host / mckpp_hip_window_fetch.  Interval means
 * (records) on a caller axis are mckpp_hip_vrecords.h's.
 *
 * Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued, streams passed as
 * void *, a refusal leaves state, schedules, records, grids and axes untouched and names the function and planes[k].
 */
#ifndef MCKPP_HIP_HV_H
#define MCKPP_HIP_HV_H

#include "mckpp_hip_remap.h"
#include "mckpp_hip_vaxis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_HV_PLANES_MAX 64

/* ---- fields out: vertical first, at the model point; then horizontal, at the caller's level ---- */

/* One plane: out(n_grid, n_axis), points fastest, doubles (MCKPP_EXP_F64) or floats (MCKPP_EXP_F32), on caller grid
 * `grid` and caller axis `axis`.
 *
 * The source value x at model point p and caller level j is mckpp_hip_vaxis_fetch_dev's double for that field, point
 * and level, bit for bit: vinterp of the column as it stands from zm(1:nzp1) to the caller's level, S with Sref added
 * to both bracket values first.  From there on it is the `out` direction of mckpp_hip_hgrid.h, unchanged, at caller
 * level j: the row sum a over the used entries - entries whose model point is no resident column of the group are left
 * out -, norm MCKPP_HGRID_NORM_NONE (the value is a) or MCKPP_HGRID_NORM_USED (a / d, d the used weights summed in the
 * same order; d == 0.0 counts as no used entry); a caller point without a used entry gets land_value where
 * fill_land != 0 and keeps what `out` held otherwise; a float plane is one final conversion. */
typedef struct { int32_t field, axis, dtype, grid, norm, fill_land; double land_value; void *out; } mckpp_hv_plane_c;

/* Delivers nplanes <= MCKPP_HV_PLANES_MAX planes, of any fields, grids and axes.  Ordering, events, the growth of the
 * staging block and the multi rule are mckpp_hip_hgrid_fetch_dev's: two launches on the context's stream - every
 * column's profile onto the caller's levels into an internal staging plane (npts, n_axis) of doubles, then every caller
 * point's row sum from it - behind what consumer_stream had queued at the call; consumer_stream waits for the second.
 * Refused before anything is queued: what mckpp_hip_vaxis_fetch_dev refuses of the field and the axis (two-dimensional
 * and interface-axis fields by name, an undefined axis) and what mckpp_hip_hgrid_fetch_dev refuses of the grid, the norm
 * and the array (an undefined grid, a missing out table, a grid defined for another npts, an unknown norm, planes whose
 * out arrays overlap, an out that is null, host memory, unreachable or too small for n_grid * n_axis elements). */
int mckpp_hip_hv_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_plane_c *planes, void *consumer_stream);

/* ---- state in: horizontal first, at the caller's levels; then vertical ---- */

/* One plane: in(n_grid, n_axis), points fastest, doubles or floats widened exactly first.  It holds the whole caller
 * axis `axis` and writes the whole model profile, levels 0 .. nzp1 - 1, of one of the five state fields of
 * mckpp_hip_put.h.
 *
 * For resident column c and caller level k, s(c, k) is the row sum of the column's `in` row over level k of the plane:
 * the `in` direction of mckpp_hip_hgrid.h - all entries count, the first assigns w * x, the rest add in entry order.
 * The value of model level lev is then vinterp through the entry of the axis's in table for lev: s(c, kin) for a clamp
 * (ABOVE, BELOW), va + ((va - vb) * t) / dz with va = s(c, kin), vb = s(c, kin + 1) for a bracket, each operation
 * rounded once.  What then happens to the value is mckpp_hip_put.h's, unchanged: op SET or ADD, S against S_ANOM,
 * MCKPP_PUT_TIME_LEVELS, the surface references after level 0.
 *
 * flags & MCKPP_PUT_SKIP: a state element (c, lev) is left untouched if ANY entry of the column's row reads a value that
 * compares == to skip_value at a caller level the branch of lev reads: kin, and kin + 1 for a bracket.  Neither a sum
 * nor the interpolated value is ever compared.
 *
 * An EMPTY `in` row of a resident column leaves the whole column untouched: mckpp_hip_remap_put_dev's rule. */
typedef struct { int32_t field, axis, dtype, op, flags, grid; double skip_value; const void *in; } mckpp_hv_put_plane_c;

/* Applies nplanes <= MCKPP_HV_PLANES_MAX planes in one launch on the context's stream, behind everything queued there
 * and behind what producer_stream had queued at the call; the event mckpp_hip_dev_fence waits on is recorded behind it.
 * It cancels nothing: what mckpp_hip_put_dev leaves alone, this leaves alone.
 * Refused before anything is queued: what mckpp_hip_remap_put_dev refuses of the grid and the array (an undefined grid,
 * a missing in table, a grid defined for another npts, an `in` that is null, host memory, unreachable or too small for
 * n_grid * n_axis elements) and what mckpp_hip_vaxis_put_dev refuses of the axis and the planes (no state uploaded, the
 * count, a non-state field, an unknown dtype, op or flag bit, a NaN skip value with MCKPP_PUT_SKIP, an undefined axis,
 * two planes of one call on the same field, S and S_ANOM being one). */
int mckpp_hip_hv_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_put_plane_c *planes, void *producer_stream);

/* All shards with the same table; every shard is checked before any shard queues.  Fetch: every shard's first launch
 * writes shard 0's staging and shard 0 alone runs the second over the union, as mckpp_hip_multi_hgrid_fetch_dev does -
 * one context and several shards give the same bits.  Put: every shard puts its own columns through its own in table. */
int mckpp_hip_multi_hv_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_plane_c *planes, void *consumer_stream);
int mckpp_hip_multi_hv_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_put_plane_c *planes, void *producer_stream);

#ifdef __cplusplus
}
#endif
#endif
