/*
 * mckpp_hip_device_records.h - completed records of output schedules delivered into arrays in device memory.
 *
 * A companion of mckpp_hip_device.h, where the two merged features meet: mckpp_hip_fetch_dev delivers a field as it
 * stands on the device, and a record of an output schedule (mckpp_hip_window_schedule, mckpp_hip_window_schedule_zoom)
 * leaves the device through host pointers.  A coupler exchanges the mean over the coupling interval, so a partner on
 * the GPU takes it with this call, without the bus and without a host wait:
 *
 *     mckpp_hip_window_schedule_zoom(h, 0, 1, K, 1, {T, u, v, hmix}, {MEAN ...}, 4, &level0);   one record: nrec = 1
 *     for every coupling interval w:
 *       mckpp_hip_step(h, 1 + w * K, K);                       K steps, one launch: record w is complete
 *       mckpp_hip_records_dev(h, 4, planes_of_record_w, s);    the four interval means into the caller's arrays
 *       mckpp_hip_window_record_release(h, 0, w);              at once: see "Ordering"
 *       ... the caller's kernels on s: fluxes from the mean SST ...
 *       mckpp_hip_fluxes_dev(h, nt, fields, 0, flsn, el, s);
 *
 * Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued, streams passed as
 * void *, no host wait apart from the turn of the pinned image of the plane table.
 *
 * Ordering.  The delivery is one launch on the context's stream: behind everything already queued there - the launches
 * that completed the records - and behind what consumer_stream had queued at the call; an event recorded behind it is
 * what consumer_stream then waits for.  Because the delivery runs on the context's stream, everything the context
 * queues later runs behind it: mckpp_hip_window_record_release may follow the call at once, and so may the launch that
 * writes the next record into the ring slot just released.  The arrays then still receive the record that was asked
 * for.  A coupler with nrec = 1 relies on exactly this.
 */
#ifndef MCKPP_HIP_DEVICE_RECORDS_H
#define MCKPP_HIP_DEVICE_RECORDS_H

#include "mckpp_hip_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One plane of a delivery: operation `op` (0 mean, 1 min, 2 max, 3 last) of output field `field` in record `rec` of
 * schedule `sched`; levels lev0 .. lev0 + nlev - 1 (0-based) of the levels THE SCHEDULE KEEPS for that field - a
 * two-dimensional field or a one-level zoom takes lev0 = 0, nlev = 1 - written as out(npoints, nlev), points fastest,
 * npoints the point axis of the schedule's records: the grid, or the zoom's point list in list order.  Doubles (dtype
 * MCKPP_EXP_F64) or floats (MCKPP_EXP_F32).  The values are mckpp_hip_window_record_fetch's bit for bit; the mean is
 * sum / (double)period, formed in the delivery's own kernel, and a float is one conversion of that value, rounded to
 * nearest even.  fill_land != 0: every position of the point axis that is no row of the record - a grid point or a
 * listed point that is no resident column - gets land_value at every level of the plane; 0: those positions keep what
 * `out` held. */
typedef struct { int32_t sched, field, op, lev0, nlev, dtype, fill_land; int64_t rec; double land_value; void *out; }
    mckpp_dev_record_plane_c;

/* Delivers nplanes <= MCKPP_DEV_PLANES_MAX planes - of any schedules and any of their completed, unreleased records -
 * in one launch, ordered as said above.  Refused before anything is queued, with the schedules, their records and the
 * resident state untouched, by a message that names this function and planes[k]: more planes than that or a null
 * table; a schedule that is unknown or not set; a record that is incomplete or released (the message names the
 * record's steps); a field that is not in the schedule; an op the schedule does not keep for it; a level range outside
 * the kept levels, nlev < 1 included; an unknown dtype; and an `out` that is null, host memory - pinned or not -, too
 * small for npoints * nlev elements, or memory the context's device cannot reach.
 * The list of a zoom's listed points that are no row goes with the schedule, and the grid's with the resident state;
 * neither is built by a delivery in the steady state. */
int mckpp_hip_records_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_dev_record_plane_c *planes, void *consumer_stream);

/* All shards with the same table: every shard is checked before any shard queues; a shard writes its own rows, shard 0
 * also - with fill_land - the positions that no shard holds, so every element of a plane is written exactly once.  One
 * event on the caller's stream orders every shard. */
int mckpp_hip_multi_records_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_dev_record_plane_c *planes,
                                void *consumer_stream);

#ifdef __cplusplus
}
#endif
#endif
