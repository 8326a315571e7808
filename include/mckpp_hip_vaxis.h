/*
 * mckpp_hip_vaxis.h - the caller's vertical axes: profiles in, increments in, fields out, on levels that are not the
 * model's.
 *
 * A companion of mckpp_hip_put.h.  Every other call of the device-array interface speaks model levels zm(1:nzp1); none
 * of the partners they were built for lives there.  The reference itself reads its initial profiles on the file's axes
 * zvel, ztemp, zsal and interpolates them onto zm (src/mckpp_initialize_ocean_profiles_mod.F90:55-117, :122-159); an
 * analysis increment or a learned correction arrives on the analysis's or the network's levels; and a partner that
 * forms such an increment wants the state on its own levels first (XIOS's interpolate_axis, next to the zoom_axis and
 * reduce_axis of mckpp_hip_zoom.h and mckpp_hip_reduce.h):
 *
 *     mckpp_hip_vaxis_define(h, 0, n, z);                         the partner's levels, once
 *     mckpp_hip_upload(h, &state);                                column map, f, jerlov, ocdepth
 *     mckpp_hip_vaxis_init_profiles_host(h, &profiles);           the reference's initial profiles
 *     mckpp_hip_init_ocean(h, 0);
 *     for every coupling interval:
 *       mckpp_hip_step(h, nt, K);
 *       mckpp_hip_vaxis_fetch_dev(h, 1, &plane_T_out, s);         T on the partner's levels
 *       ... the partner's kernels on s: the increment dT(npts, n) ...
 *       mckpp_hip_vaxis_put_dev(h, 1, &plane_T_add, s);           T = T + vinterp(dT), on the device
 *       mckpp_hip_dev_fence(h, s);
 *
 * The interpolation, stated once.  vinterp(zs[0..n-1], vs[0..n-1], zt), zs strictly decreasing, is the reference's
 * :138-153, test for test:
 *
 *     if   zt >  zs[0]   : v = vs[0]
 *     elif zt <  zs[n-1] : v = vs[n-1]
 *     else kin = the smallest index with zs[kin+1] <= zt   (what the reference's carried DO WHILE finds, targets descending)
 *          dz = zs[kin] - zs[kin+1];  t = zt - zs[kin]     (axis values only: formed once per axis, on the host)
 *          dv = vs[kin] - vs[kin+1];  p = dv * t;  q = p / dz;  v = vs[kin] + q
 *
 * Each line is one correctly rounded fp64 operation (-ffp-contract=off, IEEE divide); floats are widened exactly first.
 * Equality belongs to the bracket branch, as in the reference: a target equal to zs[0] takes kin = 0 with t = 0, a
 * target equal to zs[n-1] takes the last pair and the formula is evaluated - the result need not be vs[n-1] bit for bit.
 *
 * Conventions are those of mckpp_hip_device.h and mckpp_hip_put.h: device pointers checked before anything is queued,
 * streams passed as void *, a refusal leaves the state, schedules, rings and series untouched and names the function
 * and planes[k].
 */
#ifndef MCKPP_HIP_VAXIS_H
#define MCKPP_HIP_VAXIS_H

#include "mckpp_hip_put.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_VAXES 8              /* caller axes of a context: 0 .. MCKPP_VAXES - 1 */
#define MCKPP_VAXIS_LEVELS_MAX 1024 /* most levels of a caller axis */
#define MCKPP_VAXIS_PLANES_MAX 64

enum { MCKPP_VAXIS_ABOVE = 0, MCKPP_VAXIS_BELOW = 1, MCKPP_VAXIS_BRACKET = 2 };   /* branch of a table entry */

/* The table of vinterp from the source axis zs[ns] onto the targets zt[nt], both strictly decreasing: per target the
 * branch, kin (ABOVE: 0, BELOW: ns - 1: the one source level read; BRACKET: kin and kin + 1 are read), and for a
 * bracket t and dz as above (0.0 and 1.0 otherwise).  HIP-free.  Returns 0, or -1 (nothing written) for a null
 * pointer, ns < 2, nt < 1, a non-finite value or an axis that does not strictly decrease. */
int mckpp_host_vaxis_map(int32_t ns, const double *zs, int32_t nt, const double *zt, int32_t *branch, int32_t *kin,
                         double *t, double *dz);

/* Defines caller axis `axis` (0 .. MCKPP_VAXES - 1): n levels z[0..n-1] in host memory, in the convention of zm (heights,
 * strictly decreasing).  Refused: n < 0, n == 1, n > MCKPP_VAXIS_LEVELS_MAX, a null z, a non-finite value, an axis not
 * strictly decreasing.  n = 0 drops the axis (z is not read).  The axis carries two small device tables built on the
 * host by mckpp_host_vaxis_map: the in table, per model level against zm(1:nzp1) as targets, and the out table, per
 * caller level with zm(1:nzp1) as the source.  It belongs to the context, not to the resident state: mckpp_hip_upload
 * and mckpp_hip_load_restart keep it.  Redefining an axis waits for the context's stream first. */
int mckpp_hip_vaxis_define(mckpp_hip_handle h, int axis, int32_t n, const double *z);

/* One plane of a put on a caller's axis: in(npts, n_axis), points fastest, doubles or floats, holds the whole caller
 * axis `axis`, and the plane writes the whole model profile, levels 0 .. nzp1 - 1, of state field `field` (the five
 * state fields of mckpp_hip_put.h).  The value v of each model level is vinterp of the column's input profile; what
 * then happens to v is mckpp_hip_put.h's, unchanged: op SET and ADD, S against S_ANOM, MCKPP_PUT_TIME_LEVELS, the
 * surface references (level 0 is always written, unless skipped).  flags & MCKPP_PUT_SKIP: a model level is left
 * untouched if any input value its branch reads (one or two of them) compares == to skip_value. */
typedef struct { int32_t field, axis, dtype, op, flags; double skip_value; const void *in; } mckpp_vaxis_put_plane_c;

/* Limit, ordering, event (mckpp_hip_dev_fence), staging and the host form's wait are mckpp_hip_put_dev's and
 * mckpp_hip_put_host's.  Refused, in addition to what those refuse: an undefined axis (or one outside 0 ..
 * MCKPP_VAXES - 1), two planes of one call on the same field (S and S_ANOM are one field), an `in` too small for
 * npts * n_axis elements. */
int mckpp_hip_vaxis_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, void *producer_stream);
int mckpp_hip_vaxis_put_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes);

/* The reference's initial profiles (src/mckpp_initialize_ocean_profiles_mod.F90:55-117): u, v (npts, n of axis_vel),
 * temp (npts, n of axis_temp), sal (npts, n of axis_sal), points fastest, all of `dtype`.  For the resident columns:
 *   1. U, V = vinterp of u, v;  U_init, V_init = U, V
 *   2. T = vinterp of temp
 *   3. the Kelvin rule: if any element satisfies T > 200 && T < 400 (strict on both sides), T = T - tk0 at every element
 *   4. S = vinterp of sal
 *   5. Sref = (S(1) + S(nzp1)) / 2.;  SSref = Sref;  X2 = S - Sref
 *   6. Tref = T(1);  Ssurf = SSref under L_SSref, otherwise X2(1) + Sref
 * Nothing else is written: Us, Xs, hmixd, old / new and hmix remain mckpp_hip_init_ocean's to seed, as in the reference.
 * The rule's ANY runs over the resident columns - over all shards of a multi handle.  The reference's runs over every
 * point, land included; land points are no resident columns here and their values are never read, so a Kelvin value at
 * a land point alone subtracts nothing: the one documented difference.
 * State must have been uploaded: the upload supplies the column map, f, jerlov and ocdepth, and its profile members
 * may hold anything.  This is an initialisation call: it returns when the state is written, like mckpp_hip_upload.
 * Refused: no state, a null member, an undefined axis, an unknown dtype, a non-finite tk0, and in the _dev form what
 * mckpp_hip_put_dev refuses of a device pointer (u, v, temp, sal are named). */
typedef struct { int32_t axis_vel, axis_temp, axis_sal, dtype; double tk0; const void *u, *v, *temp, *sal; } mckpp_vaxis_profiles_c;
int mckpp_hip_vaxis_init_profiles_dev(mckpp_hip_handle h, const mckpp_vaxis_profiles_c *p, void *producer_stream);
int mckpp_hip_vaxis_init_profiles_host(mckpp_hip_handle h, const mckpp_vaxis_profiles_c *p);

/* One plane of a fetch on a caller's axis: out(npts, n_axis), points fastest, doubles or floats (one final
 * conversion).  Each element is vinterp of the field as it stands on the device - mckpp_hip_window_fetch(field, 3)'s
 * value, S with Sref added first - from zm(1:nzp1) to the caller's level.  Only three-dimensional fields on the levels
 * axis 1..nzp1 are taken; two-dimensional fields and interface-axis fields (wu .. wTnt, dif*) are refused by name.
 * Ordering, fill_land and the multi rule (shard 0 writes the points no shard holds) are mckpp_hip_fetch_dev's. */
typedef struct { int32_t field, axis, dtype, fill_land; double land_value; void *out; } mckpp_vaxis_dev_plane_c;
int mckpp_hip_vaxis_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes, void *consumer_stream);

/* All shards: an axis is defined on every shard; puts, profiles and fetches take the full-size arrays, every plane of
 * every shard is checked before any shard queues, and a shard touches only its own columns. */
int mckpp_hip_multi_vaxis_define(mckpp_hip_multi_handle m, int axis, int32_t n, const double *z);
int mckpp_hip_multi_vaxis_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, void *producer_stream);
int mckpp_hip_multi_vaxis_put_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes);
int mckpp_hip_multi_vaxis_init_profiles_dev(mckpp_hip_multi_handle m, const mckpp_vaxis_profiles_c *p, void *producer_stream);
int mckpp_hip_multi_vaxis_init_profiles_host(mckpp_hip_multi_handle m, const mckpp_vaxis_profiles_c *p);
int mckpp_hip_multi_vaxis_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes, void *consumer_stream);

#ifdef __cplusplus
}
#endif
#endif
