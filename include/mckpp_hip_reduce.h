/*
 * mckpp_hip_reduce.h - completed records of output schedules reduced over points and levels on the device.
 *
 * A companion of mckpp_hip_device_records.h: XIOS's reduce_axis and reduce_domain of a <file> in iodef.xml.  Where
 * mckpp_hip_records_dev delivers a plane out(npoints, nlev) of a record, the calls below deliver that plane reduced
 * over its levels (out(npoints)), over its points (out(nlev)), or over both (one double): a domain-mean SST, a column
 * heat content sum_k hm(k) * T(k), a horizontal-mean profile, a domain-integrated salt - 8 bytes to a few hundred,
 * from one pass over a record that is resident already, instead of the plane over the bus and a sum on the host.
 *
 *     mckpp_hip_reduce_weights(h, area, hm, NULL);                        once: point and level weights
 *     mckpp_hip_window_schedule_zoom(h, 0, 1, K, 1, {T}, {MEAN}, 1, &level0);
 *     for every interval w:
 *       mckpp_hip_step(h, 1 + w * K, K);
 *       mckpp_hip_records_reduce_dev(h, 1, {sched 0, rec w, T, mean; axis none, domain average, area-weighted}, s);
 *       mckpp_hip_window_record_release(h, 0, w);                         at once: ordering as in the companion
 *       ... the caller's kernels on s read the one double ...
 *
 * Conventions are those of mckpp_hip_device_records.h: everything is checked before anything is queued, messages name
 * the function and planes[k], streams are void *, at most MCKPP_DEV_PLANES_MAX planes per call.
 *
 * The arithmetic, stated once.  Every *, + and / below is one rounded fp64 operation (no contraction), and the order
 * is part of the interface: the device, the host helper and several shards behind one handle give the same double.
 *
 *  a. A value x(r, l) is what mckpp_hip_records_dev delivers as a double for that plane, row and level: the mean as
 *     sum / (double)period, S with Sref.
 *  b. Axis reduction of a row over the plane's levels l = lev0 .. lev0 + nlev - 1.  The weight wl of a level is
 *     level_w (iface_w for a field on the interface axis: wu, wv, wt, ws, wb, wtnt, difm, dift, difs) at l + the zoom's
 *     lev0, or 1.0 without bit 0 of `weighted`.  Sum: a = wl * x of the first level, then a = a + wl * x for each
 *     further level in ascending order.  Average: that sum divided by W, the weights summed in the same ascending
 *     order - (double)nlev without weights -, and land_value if W == 0.0.  Min and max: of the x alone, m = x of the
 *     first level, then m = x < m ? x : m (max: x > m ? x : m) in ascending order.
 *  c. Domain reduction over the positions p = 0 .. npoints - 1 of the schedule's point axis.  The term of a position
 *     that is a row is t[p] = wp[point(p)] * a[p] - a[p] itself without bit 1 - and of a position that is no row +0.0.
 *     Sum: let N2 be the smallest power of two >= npoints; the terms are padded with +0.0 up to N2; then, while n > 1:
 *     n /= 2; t[i] = t[i] + t[i + n] for i < n.  Average: that sum divided by the same tree over wp[point(p)] at rows
 *     (1.0 without weights) and +0.0 elsewhere, and land_value if that denominator == 0.0.  Min and max: the same
 *     tree with t[i] = t[i + n] < t[i] ? t[i + n] : t[i] (max: >), the term of a position that is no row, and the
 *     padding, +infinity (max: -infinity) - so over rows only.  A plane whose schedule has no row delivers land_value
 *     in every element.
 *  d. Axis-only planes write land_value at positions that are no row (mckpp_hip_records_dev's rule with fill_land).
 *
 * The tree of c decomposes for any power of two M <= N2: the elements j, j + M, j + 2M, ... of each residue j reduced
 * by the same tree, then the M partials reduced by the same tree, give the same bits.  That is how the kernels split
 * a plane over workgroups - no atomics, no dependence on the grid - and how a run with one process per GPU gets the
 * same double: it gathers its axis-reduced planes like any field and calls mckpp_host_reduce_tree on the terms.
 */
#ifndef MCKPP_HIP_REDUCE_H
#define MCKPP_HIP_REDUCE_H

#include "mckpp_hip_device_records.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_RED_NONE 0
#define MCKPP_RED_SUM 1
#define MCKPP_RED_AVERAGE 2
#define MCKPP_RED_MIN 3
#define MCKPP_RED_MAX 4
#define MCKPP_RED_W_LEVELS 1   /* bits of `weighted` */
#define MCKPP_RED_W_POINTS 2

/* One reduced plane: sched, field, op, lev0, nlev and rec name a plane as in mckpp_dev_record_plane_c.
 * axis_op / domain_op: 0 none, 1 sum, 2 average, 3 min, 4 max; not both 0.
 * weighted: bit 0 - level weights in the axis reduction, bit 1 - point weights in the domain reduction
 *           (a bit whose weights are not set, or whose reduction is none/min/max: refused by name).
 * out:  domain_op none -> out(npoints) doubles, the schedule's point axis (grid, or zoom list in list order);
 *       axis_op none   -> out(nlev) doubles; both -> one double. */
typedef struct { int32_t sched, field, op, lev0, nlev, axis_op, domain_op, weighted;
                 int64_t rec; double land_value; void *out; } mckpp_reduce_plane_c;

/* The weights of the reductions: point_w(npts) host doubles by point number of the 3-D ordering (a zoomed schedule
 * looks a listed point up by its number), level_w(nzp1) for fields on the level axis (hm, for a heat content),
 * iface_w(nzp1) for fields on the interface axis.  NULL: not set; a second call replaces all three.  Every weight
 * must be finite and >= 0: otherwise the call is refused, naming the array and the index, and the weights in place
 * stay.  They are the context's own until replaced or finalized: indexed by point and by level, not by resident
 * column, so mckpp_hip_upload and mckpp_hip_load_restart leave them alone.  Needs the grid's size: after the first
 * upload or load_restart.  Waits for the context's stream (a reduction in flight may read the weights in place). */
int mckpp_hip_reduce_weights(mckpp_hip_handle h, const double *point_w, const double *level_w, const double *iface_w);

/* Reduces nplanes <= MCKPP_DEV_PLANES_MAX planes into device memory, stream-ordered exactly like
 * mckpp_hip_records_dev: behind everything queued on the context's stream and behind what consumer_stream had queued
 * at the call; consumer_stream then waits for an event behind the delivery.  No host wait but the turn of the pinned
 * image of the plane table; mckpp_hip_window_record_release and the next launch may follow at once.  Refused before
 * anything is queued, by a message that names this function and planes[k]: everything mckpp_hip_records_dev refuses
 * of sched, rec, field, op, lev0, nlev; both ops none (a plane that is not reduced is mckpp_hip_records_dev's); an op
 * outside 0..4; a `weighted` bit without its weights or on a reduction that takes none; an unknown bit; and an `out`
 * that is null, host memory, too small, or memory the context's device cannot reach.
 * The scratch the terms of c travel through - N2 doubles per level of a domain-reduced plane, one more slab for an
 * average - is the context's, grow-only: the first call of a shape allocates, the steady state does not. */
int mckpp_hip_records_reduce_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_reduce_plane_c *planes, void *consumer_stream);

/* The same launches, then one copy of all results through a pinned block of the context's and a wait for it: `out`
 * is plain host memory, refused only if null. */
int mckpp_hip_records_reduce_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_reduce_plane_c *planes);

/* The tree of c over t[0 .. n-1] on the host, no GPU: +0.0 for n <= 0.  t is not changed. */
double mckpp_host_reduce_tree(const double *t, int64_t n);

/* All shards with the same weights and the same table; every plane of every shard is checked before any shard queues.
 * The results are the single context's bit for bit: every shard writes the terms of its own rows (b, with the point
 * weight applied) into shard 0's scratch, events order them, and shard 0 runs c and delivers.  Axis-only planes are
 * mckpp_hip_multi_records_dev's case: every shard writes its own positions, shard 0 the land_value positions. */
int mckpp_hip_multi_reduce_weights(mckpp_hip_multi_handle m, const double *point_w, const double *level_w, const double *iface_w);
int mckpp_hip_multi_records_reduce_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_reduce_plane_c *planes,
                                       void *consumer_stream);
int mckpp_hip_multi_records_reduce_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_reduce_plane_c *planes);

#ifdef __cplusplus
}
#endif
#endif
