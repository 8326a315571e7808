/*
 * mckpp_hip_zoom.h - output schedules over chosen points and levels: what XIOS offers per <file> of iodef.xml as
 * zoom_domain and zoom_axis.
 *
 * A companion of mckpp_hip.h.  mckpp_hip_window_schedule keeps, for every field of a schedule, every resident column
 * and - for a three-dimensional field - every level.  A zoomed schedule keeps a list of points and a range of levels:
 * its records, its export slots and its fetches are sized to the zoom, a column outside the list takes no part in the
 * column kernel's window stage, and a column in it touches only the levels kept.
 *
 *     int32_t pts[5] = {...};                                   five moorings
 *     mckpp_win_zoom_c z = {pts, 5, 0, 0};                      ... every level
 *     mckpp_hip_window_schedule_zoom(h, 1, 1, 1, 24, f, ops, 2, &z);   every step's profile: period 1, MCKPP_WIN_LAST
 *     mckpp_hip_step(h, 1, 24);                                 one launch
 *     mckpp_hip_window_record_fetch(h, 1, rec, MCKPP_OUT_T, 3, out);   out(5, nzp1)
 *
 * Everything else about a schedule is mckpp_hip.h's: mckpp_hip_window_records, _record_release, the ring guard, the
 * rule that the steps under a schedule follow on from one another, the rule for diagnostic fields, the cancelling by
 * mckpp_hip_upload and mckpp_hip_load_restart, and mckpp_hip_window_export with its layout and fetches.  Conventions
 * are those of mckpp_hip.h.
 */
#ifndef MCKPP_HIP_ZOOM_H
#define MCKPP_HIP_ZOOM_H

#include "mckpp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The zoom of a schedule.
 *  points   npoints distinct point numbers, 0-based, in the 3-D ordering (the numbering mckpp_hip_step_log_fetch
 *           reports), in any order; points that are no resident column (land) are allowed.  NULL: every point, in
 *           order (npoints is then not read).
 *  lev0, nlev   levels lev0 .. lev0 + nlev - 1 (0-based) of each three-dimensional field's own vertical axis, the
 *           convention of mckpp_dev_plane_c: both axes - levels 1..nzp1, interfaces 0..nz - have nzp1 entries.
 *           lev0 = 0, nlev = 0: the whole axis.  Two-dimensional fields ignore the range. */
typedef struct { const int32_t *points; int64_t npoints; int32_t lev0, nlev; } mckpp_win_zoom_c;

/* mckpp_hip_window_schedule with a zoom; zoom == NULL is that call itself (one body sets both).  Checked before the
 * schedule in place is touched, each failing by name and leaving the old schedule and the resident state as they were:
 * a point outside 0 .. npts-1; a point given twice (the message names the point and both positions); npoints < 1 with
 * a list; a level range outside 0 .. nzp1, or nlev < 0.
 *
 * The shape of a zoomed schedule: the point axis of its records is the list, in list order.
 *  - mckpp_hip_window_record_fetch writes out(npoints[, nlev]); listed points that are no resident column keep what
 *    `out` held (a list of land points only: every fetch leaves `out` as it was);
 *  - mckpp_hip_window_export_layout reports the zoomed nlev per plane and record_bytes over npoints points;
 *    mckpp_hip_window_export_fetch and _fetch_record deliver that layout, listed land points at land_value.
 *
 * Memory: a record plane has rows for the listed points that are resident columns, no others.  A row is one double
 * for a single level, otherwise the smallest multiple of 8 doubles that holds nlev.  (A schedule set without a zoom
 * keeps the rows it always had: every resident column, ld doubles.) */
int mckpp_hip_window_schedule_zoom(mckpp_hip_handle h, int sched, int nt_origin, int period, int nrec,
                                   const int32_t *fields, const uint32_t *ops, int32_t nfields,
                                   const mckpp_win_zoom_c *zoom);

/* The zoom of schedule `sched` - any schedule, zoomed or not: the points of its records' point axis, the level range
 * of its three-dimensional fields (the whole axis: 0, nzp1), and ring_bytes, the device bytes of its record ring
 * without the export.  Any output pointer may be NULL. */
int mckpp_hip_window_zoom(mckpp_hip_handle h, int sched, int64_t *npoints, int32_t *lev0, int32_t *nlev,
                          int64_t *ring_bytes);

/* XIOS zoom_domain -> point list, host only: the box of ni x nj points whose first is (ibegin, jbegin), 0-based, of a
 * grid of nx x ny points, as ni * nj point numbers j * nx + i, i fastest.  A box that is empty or not within the grid
 * is an error. */
int mckpp_host_zoom_box(int64_t nx, int64_t ny, int64_t ibegin, int64_t ni, int64_t jbegin, int64_t nj,
                        int32_t *points);

/* All shards.  Every shard checks the whole zoom and keeps rows only for the listed points it owns, so the shards'
 * ring_bytes - which mckpp_hip_multi_window_zoom adds up - come to a single context's for the same list.  Fetches
 * merge through list positions (mckpp_host_export_merge with the list positions as its points); the merged result is
 * the single context's, bit for bit. */
int mckpp_hip_multi_window_schedule_zoom(mckpp_hip_multi_handle m, int sched, int nt_origin, int period, int nrec,
                                         const int32_t *fields, const uint32_t *ops, int32_t nfields,
                                         const mckpp_win_zoom_c *zoom);
int mckpp_hip_multi_window_zoom(mckpp_hip_multi_handle m, int sched, int64_t *npoints, int32_t *lev0, int32_t *nlev,
                                int64_t *ring_bytes);

#ifdef __cplusplus
}
#endif
#endif
