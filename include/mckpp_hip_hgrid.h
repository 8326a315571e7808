/*
 * mckpp_hip_hgrid.h - the caller's horizontal grids: forcing in and fields out on points that are not the model's, by
 * remap weights the caller brings.
 *
 * A companion of mckpp_hip_device.h.  Every other call of the device-array interface takes and delivers (npts, ...)
 * arrays on the model's own points; an atmosphere emulator or a GPU atmosphere has a grid of its own, and the remap
 * between the two is the coupler's job (XIOS's interpolate_domain, SCRIP / OASIS remapping; the family's other members
 * are the zoom_* of mckpp_hip_zoom.h, the reduce_* of mckpp_hip_reduce.h and the interpolate_axis of mckpp_hip_vaxis.h):
 *
 *     mckpp_hip_upload(h, &state);                                  column map: what is resident
 *     mckpp_hip_hgrid_define(h, 0, n_atm, &atm_to_ocean, &ocean_to_atm);   the weights, once
 *     for every coupling interval:
 *       mckpp_hip_hgrid_fetch_dev(h, 1, &sst_on_atm_grid, s);       SST on the atmosphere's grid
 *       ... the atmosphere's kernels on s: eight flux fields on its grid ...
 *       mckpp_hip_hgrid_fluxes_dev(h, 0, nt, fields, 0, flsn, el, s);
 *       mckpp_hip_dev_fence(h, s);
 *       mckpp_hip_step(h, nt, ndtocn);
 *
 * The reference has nothing to restate here (its coupling weight cplwght is read and sent on, nothing more), so the
 * arithmetic and its order are stated here, once; the device, mckpp_host_hgrid_apply and several shards give the same
 * bits.  Every *, + and / below is one correctly rounded fp64 operation (-ffp-contract=off, IEEE divide).
 *
 * A weight table is CSR in host memory: row r has the entries ptr[r] .. ptr[r+1] - 1, entry e reads source index idx[e]
 * with weight w[e].  The USED entries of a row are its entries in ascending entry order - in the `out` direction
 * without those whose model point is no resident column (under a multi handle: a column of no shard).
 *
 *     a = w * x    of the first used entry                 (an assignment: a lone -0.0 survives)
 *     a = a + w * x   for each further used entry, in order
 *
 * In:  a resident column's value is a; all entries are used.  A call whose resident columns include one with an empty
 *      `in` row is refused before anything is queued, naming the point.
 * Out: norm MCKPP_HGRID_NORM_NONE: the value is a.
 *      norm MCKPP_HGRID_NORM_USED: the value is a / d, d the weights of the used entries summed in the same order
 *      (d = w; d = d + w): the couplers' "fracarea" normalisation along a coast.  d == 0.0 counts as no used entry.
 *      A caller point with no used entry gets land_value where the plane fills, and keeps what `out` held otherwise.
 *      x is mckpp_hip_fetch_dev's double for that field, point and level (S includes Sref); a float plane is one final
 *      conversion.
 *
 * Conventions are those of mckpp_hip_device.h: device pointers checked before anything is queued, streams passed as
 * void *, a refusal leaves state, schedules, rings and series untouched and names the function and the argument or
 * planes[k].
 */
#ifndef MCKPP_HIP_HGRID_H
#define MCKPP_HIP_HGRID_H

#include "mckpp_hip_device.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_HGRIDS 4              /* caller grids of a context: 0 .. MCKPP_HGRIDS - 1 */
#define MCKPP_HGRID_PLANES_MAX 64

enum { MCKPP_HGRID_NORM_NONE = 0, MCKPP_HGRID_NORM_USED = 1 };

/* CSR, host memory */
typedef struct { const int64_t *ptr; const int32_t *idx; const double *w; } mckpp_hgrid_table_c;

/* ---- HIP-free host side (mckpp_hgrid_table.cpp) ---- */

/* The checks of a define on table `name` ("in", "out") of nrows rows over source indices 0 .. nsrc - 1: ptr[0] == 0,
 * ptr does not decrease, every index in range, every weight finite.  Negative weights, repeated indices in a row and
 * empty rows pass.  Returns 0, or -1 with a text in msg[0 .. msglen - 1] that names the table, the row and the entry. */
int mckpp_host_hgrid_check(const char *name, int64_t nrows, int64_t nsrc, const mckpp_hgrid_table_c *t, char *msg, int64_t msglen);

/* The arithmetic above exactly as written, for one level: out[r] for the nrows rows of t from x[0 .. nsrc - 1].
 * used (null: every entry) marks per source index whether entries that read it are used.  norm < 0: the `in`
 * direction's plain a, a row without used entry gets 0.0.  Otherwise the `out` direction with that norm: a row with no
 * used entry gets land_value if fill != 0 and keeps out[r] if not.  Returns 0, or -1 for a null pointer or an unknown
 * norm.  The table is taken as checked. */
int mckpp_host_hgrid_apply(int64_t nrows, const mckpp_hgrid_table_c *t, const double *x, const unsigned char *used, int norm,
                           int fill, double land_value, double *out);

/* The device layout, a sliced ELL, of the rows rows[0 .. nlist - 1] of t (rows null: 0 .. nlist - 1) with the entries
 * dropped whose source index keep (null: none dropped) does not mark.  Slice s holds list rows 64 s .. 64 s + 63, one
 * slice per wave; its width is its longest row after dropping; entry k of list row r lies at
 * slice_off[s] + 64 * k + r % 64 of idx_out and w_out, and len[r] is the row's number of entries; entry order is kept.
 * slice_off has nslices + 1 = (nlist + 63) / 64 + 1 elements, slice_off[nslices] is the padded size.  Padding holds
 * index 0 and weight 0.0 and is never loaded by the kernels.  idx_out == NULL: only slice_off and len are written (the
 * sizing pass).  Returns the padded size, or -1 for a null pointer or a negative nlist. */
int64_t mckpp_host_hgrid_slices(int64_t nlist, const int64_t *rows, const mckpp_hgrid_table_c *t, const unsigned char *keep,
                                int64_t *slice_off, int32_t *len, int32_t *idx_out, double *w_out);

/* ---- a caller grid and its weight tables ---- */

/* Defines caller grid `grid` (0 .. MCKPP_HGRIDS - 1) of n points.  in (caller -> model): npts rows, one per model point
 * of the 3-D ordering, idx in [0, n).  out (model -> caller): n rows, idx in [0, npts).  Either may be NULL: that
 * direction is then refused by name when used.  n = 0 drops the grid (the tables are not read).  The tables are copied
 * and belong to the context, like the reduce weights: indexed by point, not by resident column, so mckpp_hip_upload and
 * mckpp_hip_load_restart keep them (a grid defined for another npts is refused by name when used).  They need the
 * grid's size, so a define is valid only after the first upload or load_restart.  Redefining a grid waits for the
 * context's stream and the flux stream first.  Refused, and the grid in place stays: what mckpp_host_hgrid_check
 * refuses, with its text.  There is no cap on row length; mckpp_hip_hgrid_info shows a pathological table. */
int mckpp_hip_hgrid_define(mckpp_hip_handle h, int grid, int64_t n, const mckpp_hgrid_table_c *in, const mckpp_hgrid_table_c *out);

/* info[0] = n, [1] = nnz of in, [2] = nnz of out (-1: the direction is missing), [3], [4] = the padded sizes of the
 * device tables of in and out for the present resident state (0: missing), [5] = the longest row of either table.  The
 * device tables depend on the column map: the in slices cover the rows of the resident columns in column order, the out
 * slices all n rows with the entries of non-resident points dropped.  They are built on first use - this call is one -
 * and go with the resident state, as the land list of mckpp_hip_fetch_dev does. */
int mckpp_hip_hgrid_info(mckpp_hip_handle h, int grid, int64_t info[6]);

/* ---- forcing in ---- */

/* mckpp_hip_fluxes_dev and mckpp_hip_flux_ring_put_dev with fields[m] as n doubles on caller grid `grid`, in device
 * memory: each resident column's eight values are the row sums of its `in` row, then what those calls do with them,
 * unchanged - the same streams, events (mckpp_hip_dev_fence), ring rules and messages, so one ring takes host puts,
 * device puts and remapped puts in any alternation.  Under a multi handle every shard sums for its own columns. */
int mckpp_hip_hgrid_fluxes_dev(mckpp_hip_handle h, int grid, int ntime, const double *const fields[8], int l_rest, double flsn,
                               double el, void *producer_stream);
int mckpp_hip_hgrid_flux_ring_put_dev(mckpp_hip_handle h, int grid, int rec, const double *const fields[8], void *producer_stream);

/* ---- fields out ---- */

/* One plane: mckpp_dev_plane_c's field, lev0, nlev and dtype, delivered as out(n, nlev) on caller grid `grid`, points
 * fastest, with norm and fill as stated above. */
typedef struct { int32_t field, lev0, nlev, dtype, grid, norm, fill_land; double land_value; void *out; } mckpp_hgrid_plane_c;

/* Two stages on the context's stream, behind what consumer_stream had queued at the call: mckpp_hip_fetch_dev's launch
 * into an internal staging plane (npts, nlev) of doubles, then one launch that forms every caller point's row sum from
 * it; consumer_stream waits for the second.  Refused, in addition to what mckpp_hip_fetch_dev refuses: an undefined
 * grid, a missing out table, an unknown norm, planes whose out arrays overlap, an out too small for n * nlev elements.
 * Under a multi handle the shards' first stage writes shard 0's staging and shard 0 alone runs the second with the
 * union of the shards' columns as residency: one context and several shards give the same bits. */
int mckpp_hip_hgrid_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hgrid_plane_c *planes, void *consumer_stream);

/* All shards: a grid is defined on every shard; info is shard 0's with the in padding summed over the shards. */
int mckpp_hip_multi_hgrid_define(mckpp_hip_multi_handle m, int grid, int64_t n, const mckpp_hgrid_table_c *in, const mckpp_hgrid_table_c *out);
int mckpp_hip_multi_hgrid_info(mckpp_hip_multi_handle m, int grid, int64_t info[6]);
int mckpp_hip_multi_hgrid_fluxes_dev(mckpp_hip_multi_handle m, int grid, int ntime, const double *const fields[8], int l_rest,
                                     double flsn, double el, void *producer_stream);
int mckpp_hip_multi_hgrid_flux_ring_put_dev(mckpp_hip_multi_handle m, int grid, int rec, const double *const fields[8], void *producer_stream);
int mckpp_hip_multi_hgrid_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hgrid_plane_c *planes, void *consumer_stream);

#ifdef __cplusplus
}
#endif
#endif
