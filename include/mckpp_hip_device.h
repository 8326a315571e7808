/*
 * mckpp_hip_device.h - the device-array interface of the column-physics library: forcing taken from arrays in device
 * memory, output fields delivered into arrays in device memory, ordered by events on the caller's stream.
 *
 * The companion of mckpp_hip.h, whose entry points move data through host pointers.  A producer that already lives on
 * the GPU - an atmosphere emulator in PyTorch, a GPU atmosphere, a flux computation from the ocean's own SST - couples
 * through these calls without crossing the bus and without a host wait:
 *
 *     mckpp_hip_fetch_dev(h, 1, &sst_plane, s);       SST into the caller's array; stream s waits for it on the device
 *     ... the caller's kernels on s: fluxes from SST ...
 *     mckpp_hip_fluxes_dev(h, nt, fields, 0, flsn, el, s);   behind those kernels, on the device
 *     mckpp_hip_dev_fence(h, s);                      s may rewrite the eight arrays once the library has read them
 *     mckpp_hip_step(h, nt, ndtocn);
 *
 * Conventions (those of mckpp_hip.h where nothing else is said)
 *  - array pointers address DEVICE memory in the layouts the host calls use: 3-D ordering, points fastest, fp64
 *    unless stated;
 *  - every array pointer is checked (hipPointerGetAttributes) before anything is queued: a host pointer - pinned or
 *    not -, a null, an allocation too small for the call, or memory the context's device cannot reach fails the call
 *    with a message that names the argument, the context's device and the pointer's.  Nothing is then launched and
 *    the resident state is untouched.  Memory of another device is reached through peer access, enabled once per
 *    pair of devices on first use;
 *  - `stream` arguments are the caller's hipStream_t passed as void *; NULL is the null stream.  The library's streams
 *    do not synchronise with the null stream implicitly: the ordering is the events' alone;
 *  - no call waits on the host for the device, apart from the waits the matching host call already has: the pinned
 *    images of the plane table and of the parameter block have two turns, so a call waits for the copy of two calls
 *    back if that is still in flight.
 *
 * The contract on the caller's arrays: arrays handed to mckpp_hip_fluxes_dev or mckpp_hip_flux_ring_put_dev are read
 * by a kernel that runs later.  They must stay allocated and unchanged until mckpp_hip_dev_fence on the stream that
 * next writes or frees them, or until mckpp_hip_synchronize.  Arrays handed to mckpp_hip_fetch_dev are written behind
 * what the consumer stream had queued at the call, and the consumer stream waits for the delivery; any other stream
 * that touches them orders itself against the consumer stream.
 */
#ifndef MCKPP_HIP_DEVICE_H
#define MCKPP_HIP_DEVICE_H

#include "mckpp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mckpp_hip_fluxes with the eight fields - fields[0..7] = taux, tauy, swf, lwf, lhf, shf, rain, snow, npts doubles
 * each - in device memory.  An event is recorded on producer_stream and the context's stream waits for it; then one
 * launch reads each resident column's eight values through the column map and assembles sflux(1:6) and the ntflux
 * refresh of wXNT(:,1): the arithmetic of mckpp_hip_fluxes, bit for bit.  No host image, no staging, no bus. */
int mckpp_hip_fluxes_dev(mckpp_hip_handle h, int ntime, const double *const fields[8], int l_rest, double flsn, double el,
                         void *producer_stream);

/* mckpp_hip_flux_ring_put from device arrays: the same in-order rule, messages and bookkeeping, and host puts and
 * device puts may alternate within one ring.  On the ring's transfer stream, in this order: a wait for the producer's
 * event, a wait for the launches of the last run_forced call that needed the record the slot held, one gather launch
 * (the eight fields through the column map into slot rec % nslots), the slot's arrival event.  No pinned staging, so
 * not the host put's wait for the copy of two puts back.
 * Overlap: a host put's copy is a DMA transfer, which runs under a column launch whatever that launch occupies.  The
 * gather is a kernel: it runs under a launch only where the launch's workgroups leave it wave slots, registers and LDS
 * on some compute unit, and otherwise when workgroups of the launch end.  Nothing in the interface promises either.
 * Measured on an MI355X at 1e5 x 60 and at the shipped shape (profiles/devcouple/README.md): four gathers queued
 * behind a launch of 24 steps had all run 0.5 - 0.8 ms into a launch of 44 - 55 ms, so with the column kernel's
 * present geometry a device put does run under it. */
int mckpp_hip_flux_ring_put_dev(mckpp_hip_handle h, int rec, const double *const fields[8], void *producer_stream);

/* One plane of a delivery: output field `field` (any MCKPP_OUT_*), levels lev0 .. lev0 + nlev - 1 (0-based) of the
 * vertical axis mckpp_hip_window_fetch documents for it - two-dimensional fields take lev0 = 0, nlev = 1 - written as
 * out(npts, nlev), points fastest: doubles (dtype MCKPP_EXP_F64) or floats (MCKPP_EXP_F32: one conversion, rounded to
 * nearest even).  fill_land != 0: every point that is no resident column gets land_value at every level of the plane;
 * 0: those points keep what `out` held.  Sea-surface temperature for a coupler is {MCKPP_OUT_T, 0, 1, ...}. */
typedef struct { int32_t field, lev0, nlev, dtype, fill_land; double land_value; void *out; } mckpp_dev_plane_c;
#define MCKPP_DEV_PLANES_MAX 64

/* Delivers nplanes <= MCKPP_DEV_PLANES_MAX planes in one launch on the context's stream, behind everything already
 * queued there and behind what consumer_stream had queued at the call; then an event is recorded that consumer_stream
 * waits for.  Each field is taken as it stands on the device: mckpp_hip_window_fetch(field, 3, ...)'s value.  An
 * unknown field, a range outside the axis (nlev < 1 included), an unknown dtype, or a correction field on a context
 * without its rows fails before anything is queued.  The list of non-resident points is built on first use and goes
 * with the resident state. */
int mckpp_hip_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_dev_plane_c *planes, void *consumer_stream);

/* Makes `stream` wait, on the device, for every read of caller arrays the handle has queued so far: one event per
 * library stream that reads them (the context's, the flux ring's), recorded behind each gather. */
int mckpp_hip_dev_fence(mckpp_hip_handle h, void *stream);

/* All shards with the same device pointers: a shard takes full-size arrays and touches only its own points.  One
 * event on the caller's stream orders every shard.  With fill_land, shard 0 writes the points no shard holds and the
 * other shards none, so every point of a plane is written exactly once. */
int mckpp_hip_multi_fluxes_dev(mckpp_hip_multi_handle m, int ntime, const double *const fields[8], int l_rest, double flsn,
                               double el, void *producer_stream);
int mckpp_hip_multi_flux_ring_put_dev(mckpp_hip_multi_handle m, int rec, const double *const fields[8], void *producer_stream);
int mckpp_hip_multi_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_dev_plane_c *planes, void *consumer_stream);
int mckpp_hip_multi_dev_fence(mckpp_hip_multi_handle m, void *stream);

#ifdef __cplusplus
}
#endif
#endif
