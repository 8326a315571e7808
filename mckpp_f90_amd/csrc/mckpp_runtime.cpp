// mckpp_runtime.cpp - host side of the C-ABI declared in include/mckpp_hip.h and its companions mckpp_hip_device.h,
// mckpp_hip_zoom.h, mckpp_hip_device_records.h, mckpp_hip_put.h, mckpp_hip_reduce.h, mckpp_hip_vaxis.h and
// mckpp_hip_hgrid.h with mckpp_hip_remap.h and mckpp_hip_hv.h.
//
// Owns the device-resident column state (level-fastest rows, one per
// run_physics column), the device copies of kpp_const_fields, one HIP stream
// and a pair of events per context.  No CPU fallback exists: every entry
// point that computes does so by launching the gfx950 kernels of
// mckpp_kernels.hip, and fails with an error code if HIP is unavailable.
//
// Every extern "C" function that returns an error code is `return entry(__func__, handle, body)` (mckpp_own.h): a null
// pointer for the handle and any C++ exception become -1 and a text that begins with the function's name (the body
// keeps the function's indentation: the lambda is the function).  The few that return something else - the
// finalizers, a count, a name, the void host helpers - keep their documented result for no handle and hold nothing
// that can throw (no allocation, no container growth, no call of fail); mckpp_hip_multi_ctx, which does report
// through fail, has the barrier.  (The header declares them without noexcept, so their definitions cannot carry it.)
#include "../../include/mckpp_hip_device.h"
#include "../../include/mckpp_hip_zoom.h"
#include "../../include/mckpp_hip_device_records.h"
#include "../../include/mckpp_hip_put.h"
#include "../../include/mckpp_hip_reduce.h"
#include "../../include/mckpp_hip_vaxis.h"
#include "../../include/mckpp_hip_hgrid.h"
#include "../../include/mckpp_hip_remap.h"
#include "../../include/mckpp_hip_hv.h"
#include "../../include/mckpp_hip_vrecords.h"
#include "mckpp_device.h"
#include "mckpp_math.h"
#include "mckpp_own.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace {

// profile rows (element j <-> level j+1)
enum { P_U = 0, P_V, P_T, P_S, P_US0, P_US1, P_VS0, P_VS1, P_TS0, P_TS1, P_SS0, P_SS1, P_UINIT, P_VINIT, P_COUNT };
// optional-physics input rows (allocated only when a switch needs them)
enum { E_FCORR_WITHZ = 0, E_SFCORR_WITHZ, E_OCNT_CLIM, E_SAL_CLIM, E_COUNT };
// optional-physics output rows (indexed by k like the diagnostics)
enum { O_TINC = 0, O_SINC, O_OCNTCORR, O_SCORR, O_COUNT };
// diagnostic rows (element k <-> reference index k)
enum { D_RHO = 0, D_CP, D_BUOY, D_TALPHA, D_SBETA, D_DIFM, D_DIFS, D_DIFT, D_GHAT, D_WU1, D_WU2,
       D_WX1, D_WX2, D_WX3, D_WXNT1, D_RIG, D_DBLOC, D_SHSQ, D_COUNT };

const double jer_rfac[6] = {0, 0.58, 0.62, 0.67, 0.77, 0.78};
const double jer_a1[6] = {0, 0.35, 0.6, 1.0, 1.5, 1.4};
const double jer_a2[6] = {0, 23.0, 20.0, 17.0, 14.0, 7.9};

}  // namespace

enum { QBLOCK_INTS = 64 };
// margins of the guesses the column kernel forms its bulk Richardson numbers down to (mckpp_kparams_t::first_margin,
// guess_margin): chosen on the headline workload, profiles/r06/README.md
enum { FIRST_MARGIN_DEFAULT = 12, GUESS_MARGIN_DEFAULT = 0 };

// The streams: the first base of the context, so declared before - and destroyed after - everything queued on them.
struct mckpp_ctx_streams {
  hip_stream stream;
  // Row transfers (upload / download): two device staging buffers used in turn and a copy stream, so the PCIe
  // transfer of one field runs while the layout kernel of the next does; the caller's arrays are pinned
  // (hipHostRegister, once per array) so those transfers are asynchronous and run at the bus rate.
  hip_stream copy_stream;
  hip_stream snap_stream;   // transfers of snapshot_save and of the export's fetches
  hip_stream flux_stream;   // the flux ring's host-to-device copies (mckpp_hip_flux_ring_put): they run under the launches
                            // already queued, so not on copy_stream, whose downloads wait for the kernels
};

// Everything sized to the resident columns: free_state drops it as a whole, by one assignment.  A new feature whose
// buffers live as long as the resident state adds its members here, and nothing to free_state or finalize.
struct mckpp_ctx_resident {
  int64_t npts = 0, ncol = 0;
  dev_buf<int> d_ipt;
  dev_buf<double> d_prof[P_COUNT];
  dev_buf<double> d_diag[D_COUNT];
  dev_buf<double> d_ext_in[E_COUNT];
  dev_buf<double> d_ext_out[O_COUNT];
  dev_buf<double> d_xs, d_adv_d;
  dev_buf<int> d_adv_i;
  // output-window reductions: per selected field (mckpp_hip_ctx::wsel) three accumulators (sum, min, max)
  std::vector<dev_buf<double>> d_wacc;   // [wsel.size()], each 3 * (ncol*ld | ncol) doubles
  int window_count = 0;
  // output windows the step launches accumulate themselves (mckpp_hip_window_schedule): per schedule its fields, their
  // operation masks and rings of records; the steps run under it; the device table of all schedules' fields
  // a device table of a caller's horizontal grid: see hgd below
  struct hgrid_dev {
    dev_buf<int64_t> off;
    dev_buf<int> len, idx;
    dev_buf<double> w;
    int64_t nrows = 0, padded = 0, empty_point = -1;
    int kind = 0;
  };
  struct win_sched {
    std::vector<int> fields;        // empty: no schedule
    std::vector<unsigned> ops;
    std::vector<int> ld_out;
    std::vector<dev_buf<double>> acc;   // [field]: nrec records of popcount(ops) planes of nrow * ld_out doubles
    int64_t origin = 1, period = 1;
    int nrec = 1;
    // The shape of a record (mckpp_hip_window_schedule_zoom; win_set).  A record plane is nrow rows, row r at position
    // map[r] of the record's point axis of npoints points: an unzoomed schedule has the resident columns as rows, the
    // column map as map and the grid's points as axis; a schedule with a point list has the listed resident columns, in
    // list order, their list positions (rowpos) and the list.  So a record is fetched and packed like a field of a
    // state of nrow columns among npoints points, by the kernels that do that.  [field] nlev levels from lev_off on of
    // the field's axis are kept (two-dimensional fields: their one value).
    bool zoomed = false;               // set through a non-null zoom (what mckpp_hip_window_zoom reports)
    bool listed = false;               // ... with a point list
    int64_t npoints = 0, nrow = 0;
    int lev0 = 0, znlev = 0;           // the level range as given
    std::vector<int> nlev, lev_off;
    std::vector<int> rowpos;           // listed: row -> list position
    dev_buf<int> d_rowpos, d_colrow;   // listed: rowpos; resident column -> row, -1 outside the list (mckpp_win_t::row)
    dev_buf<int> d_rowpt;              // listed: row -> point number, where the reductions look a row's point weight up
    std::vector<int> rowpt;            // ... and on the host, for what follows
    // listed: per caller grid the out table of mckpp_hip_remap_records_dev (include/mckpp_hip_remap.h), the grid's out
    // table with the entries kept whose point is a row of this schedule's records - kind as hgd[].out's: 0 not built,
    // 1 this context's rows, 2 (shard 0 of a multi handle) the rows of any shard.  Built on first use; it goes with the
    // schedule, being its member, and with the grid (hgrid_define)
    hgrid_dev hout[MCKPP_HGRIDS];
    // listed: the list positions that are no row, for the planes of mckpp_hip_records_dev that fill them (an unlisted
    // schedule's are the context's d_land).  d_norow holds nnorow positions: this context's own, set with the schedule
    // (norow_kind 1), or - shard 0 of a multi handle - those no shard has a row for, the other shards filling none (2);
    // group_norow brings it up to date for the group a call addresses
    dev_buf<int> d_norow;
    int64_t nnorow = 0;
    int norow_kind = 1;
    int64_t first_nt = -1, next_nt = -1;   // the first step run under the schedule, the step the next launch must start at (-1: none yet)
    int64_t first_kept = 0;                // the records before it are released, or began before first_nt
    // its export (mckpp_hip_window_export; dtype MCKPP_EXP_OFF: none): nrec slots of record_bytes each, record w in slot
    // w % nrec like the ring's, every plane as [nlev][npts] values of the dtype (npts: the grid's points, or with
    // `compact` - a shard of a multi handle - the resident columns themselves); per slot the event behind the launch
    // that packed it; the device table of the planes (k_record_pack)
    struct exp_plane { int field, op, nlev; int64_t offset; };
    struct win_export {
      int dtype = 0;
      bool compact = false;
      double land = 0;
      int64_t npts = 0;
      size_t record_bytes = 0;
      int maxlev = 0;
      std::vector<exp_plane> planes;
      dev_buf<char> slots;
      dev_buf<mckpp_pack_plane> d_tab;
      std::vector<hip_event> ev;
    } ex;
  } wsched[MCKPP_WIN_SCHEDULES];
  int nwin = 0;                 // entries of d_win in use (mckpp_kparams_t::nwin of the step launches)
  // restart snapshots the step launches take themselves (mckpp_hip_restart_schedule): a ring of slots, each a restart
  // set (mckpp_kparams_t::snap_*); the steps run under the schedule; per slot the event behind the launches of the
  // call that completed its snapshot
  struct snap_sched {
    int64_t origin = 1, period = 0;        // period 0: no schedule
    int nslots = 0;
    int64_t first_nt = -1, next_nt = -1;   // as win_sched's
    int64_t first_exists = 0;              // the snapshots before it were due before first_nt
    int64_t first_kept = 0;                // the snapshots before it are released, or do not exist
    dev_buf<double> rows, cs;
    dev_buf<int> ci;
    std::vector<hip_event> ev;             // [nslots]
  } rs;
  // the step log of the step launches (mckpp_hip_step_log): cap records and the two control ints - events so far,
  // OR of their status words (mckpp_kparams_t::log_*); cap 0: no log
  struct log_sched {
    dev_buf<mckpp_log_rec> rec;
    dev_buf<int> ctl;
    int64_t cap = 0;
    int min_passes = 0;
  } slog;
  // the resident bottom temperature (mckpp_hip_set_bottomtemp): ncol values in column order, an array of its own (the
  // staging buffer is rewritten by every transfer); empty: none is set (mckpp_kparams_t::bot_temp)
  dev_buf<double> d_bot_temp;
  // ancillary record series and their schedules (mckpp_hip_set_ancillary_series, mckpp_hip_ancillary_schedule), per kind:
  // `nrec` immutable records from number rec0 on, compacted to the resident columns ([ncol], or rows [ncol][ld]); step nt
  // belongs to epoch (nt - origin) / cadence, which ep[epoch - epoch0] describes (ep empty: no schedule).
  struct anc_kind { dev_buf<double> d; int rec0 = 0, nrec = 0, origin = 0, cadence = 0, epoch0 = 0; std::vector<mckpp_anc_epoch_c> ep; };
  anc_kind anc[MCKPP_ANC_COUNT];
  dev_buf<double> d_cs;
  dev_buf<int> d_ci;
  dev_buf<int> d_done;   // [2][ncol] steps of a multi-step launch each column has completed, and has started (mckpp_kparams_t::done)
  dev_buf<double> d_series;   // [nrec][8][ncol] forcing records (mckpp_hip_set_flux_series)
  int series_rec0 = 0, series_nrec = 0;
  // the ring of flux-record slots (mckpp_hip_flux_ring): record r in slot r % nslots, each [8][ncol] compacted like a
  // record of d_series; the records put so far are first_put .. next_put - 1, resident the last nslots of them.  Per
  // slot two events: `arrived` behind the copy of the record it holds (flux_stream), `last_read` behind the launches of
  // the last run_forced call that needed that record (the context's stream) - the next copy into the slot waits for it
  // on flux_stream.  The staging: the record compacted on the host, a pinned image used in turn.  nslots 0: no ring.
  struct flux_ring {
    int nslots = 0;
    int first_put = -1, next_put = -1;   // -1: nothing put yet (the first put names any record)
    dev_buf<double> slots;
    std::vector<hip_event> arrived, last_read;   // [nslots]
    pinned_turns<double> stage;
  } ring;
  // the grid points that are no resident column, for the planes of mckpp_hip_fetch_dev that fill them.  land_kind 0: not
  // built (first use builds it; a new column map drops it); 1: the complement of this context's column map; 2: shard 0 of a
  // multi handle - the points no shard holds, the other shards filling none (group_land)
  dev_buf<int> d_land;
  int64_t nland = 0;
  int land_kind = 0;
  dev_buf<double> d_stage;    // grow-only (ensure_stage)
  // The device tables of the caller's horizontal grids (include/mckpp_hip_hgrid.h), per grid and direction the sliced
  // ELL of mckpp_host_hgrid_slices.  They depend on the column map - `in` has the resident columns' rows in column
  // order, `out` every caller point's row without the entries of non-resident points - so they are built on first use
  // and go with the resident state, like d_land (a new column map marks them not built).  kind 0: not built; 1: for
  // this context's column map; 2 (out, shard 0 of a multi handle): for the union of the shards' columns.  empty_point:
  // the first resident column's point whose in row is empty (-1: none).  d_hstage: the staging plane(s) of
  // mckpp_hip_hgrid_fetch_dev, (npts, nlev) doubles per plane, grow-only (hgrid_stage).
  struct { hgrid_dev in, out; } hgd[MCKPP_HGRIDS];
  dev_buf<double> d_hstage;
  dev_buf<char> d_put_stage;  // the planes of mckpp_hip_put_host, grow-only: the call ends with a wait, so nothing reads it between calls
  dev_buf<double> d_xfer[2];  // the staging buffers of the row transfers, grow-only (ensure_xfer)
  // pinned host images of the column records and of the forcing staging (grow-only: ensure_host_f)
  pinned_buf<double> h_cs, h_f;
  pinned_buf<int> h_ci;
  // record slots as (npts) slabs in 3-D order, packed on the device (a context that holds every grid point)
  dev_buf<double> d_pack;       // packed record slabs of a download: device block,
  pinned_buf<double> h_pack;    // ... pinned host block
};

struct mckpp_hip_ctx : mckpp_ctx_streams, mckpp_ctx_resident {
  int device = 0;
  hip_event ev0, ev1;
  bool timed = false;
  int nlaunch = 0;
  int nkernels = 0;   // kernel launches of the last call (a call of several steps may be one launch)
  mckpp_const_c c{};
  int nz = 0, nzp1 = 0, lpl = 1, ld = 64, ldc = 72;
  double Vtc = 0, cg = 0, dm_nz = 0;
  std::vector<double> h_swfrac_tab, h_swdk_tab;
  dev_buf<double> d_zm, d_hm, d_tri0, d_tri1, d_swfrac_tab, d_swdk_tab, d_dm, d_hsum;
  dev_buf<double2> d_wtab;
  std::vector<int> ipt;      // the resident columns' grid points (d_ipt)
  bool ext = false;          // any optional-physics switch on: the context carries their input / output fields
  bool ext_kernel = false;   // ... and needs the kernel build with the N3 code (a T/S climatology for the reset of
                             // failed columns alone - the shipped namelist - does not: the default build reads it)
  std::vector<int> wsel{0, 1, 2, 3, 4};   // selected MCKPP_OUT_* fields of the output-window reductions (d_wacc)
  dev_buf<mckpp_win> d_win;   // [MCKPP_WIN_ENTRIES]: the device table of all output schedules' fields
  // the selection table of the latest launch call under ancillary schedules ([nsteps][kinds], mckpp_kparams_t::anc_sel),
  // grow-only, written on the stream ahead of its kernels from a pinned host image
  dev_buf<mckpp_anc_sel> d_anc_sel;
  pinned_turns<mckpp_anc_sel> h_anc_sel;
  int anc_mask = 0, anc_nt0 = 0;   // of the launch call being issued (anc_prepare)
  pinned_buf<char> h_snap[2];      // two pinned staging blocks for snapshot_save
  hip_event ev_snap[2];
  dev_buf<int> d_qhead;  // QBLOCK_INTS ints, zeroed before every launch: [0..15] queue heads, [16..31] queue owners, [32] stragglers on the device
  int view_kmax = 0;   // mckpp_kparams_t::view_kmax (MCKPP_VIEW_KMAX)
  int solo_after = 12, solo_limit = 8;   // mckpp_kparams_t::solo_after / solo_limit (MCKPP_SOLO=0, MCKPP_SOLO_AFTER, MCKPP_SOLO_LIMIT)
  bool multistep = true;   // mckpp_hip_step(nt, n > 1) as one launch (MCKPP_MULTISTEP=0: a launch per step)
  int nqueues = 0;         // XCDs of the device, found by a probe at init: the queues of such a launch
  int xcc_queue[16];       // hardware XCC id -> queue (-1: no workgroup of the probe ran there)
  int l3cap = 0;   // MCKPP_L3_CAP (tests): see mckpp_kparams_t::l3cap
  int first_guess = 1, first_margin = FIRST_MARGIN_DEFAULT, guess_margin = GUESS_MARGIN_DEFAULT;   // mckpp_kparams_t::first_margin, scan_rule
  int solver_mode = 0;   // mckpp_hip_set_solver_mode / MCKPP_SOLVER_MODE
  dev_buf<unsigned long long> d_dbg;
  dev_buf<mckpp_kparams> d_params;   // device copy of the kernel parameter block
  // its source: a pinned host image used in turn, so a call never waits for its own upload
  pinned_turns<mckpp_kparams> h_params;
  dev_buf<double> d_scratch;         // k_column_ps: scratch rows of the iterate, per (workgroup, slot)
  size_t scratch_doubles = 0;
  int num_cu = 256;
  int l2pre = 0;   // the reference-level sums of the deepest level span many layers: form the layer terms once per column
  mckpp_launch_info last_launch{};   // geometry of this context's most recent cooperative launch
  hip_event ev_lay[2], ev_copy[2];   // of the row transfers: layout kernel done / transfer done, per staging buffer
  unsigned xfer_seq = 0;
  std::vector<std::pair<const void *, size_t>> pinned;   // caller arrays this context registered
  std::vector<std::pair<const void *, size_t>> unpinnable;   // ... and those it could not (not tried again)
  hip_event ev_f;   // the forcing staging has been read
  // The device-array interface (include/mckpp_hip_device.h), everything created on first use.  ev_caller: recorded on the
  // caller's stream, what the library's stream then waits for; ev_delivered: behind the launch of mckpp_hip_fetch_dev, what
  // the consumer's stream waits for; ev_read / ev_read_flux: behind the last kernel on the context's stream / the flux
  // ring's that reads caller arrays (mckpp_hip_dev_fence; null: no such kernel yet).  The plane tables (mckpp_own.h) of
  // fetch_dev, of mckpp_hip_records_dev (its event behind the launch is ev_delivered too) and of mckpp_hip_put_dev /
  // _put_host (include/mckpp_hip_put.h; the event behind its launch is ev_read).
  hip_event ev_caller, ev_delivered, ev_read, ev_read_flux;
  plane_table<mckpp_fetch_plane, MCKPP_FETCH_PLANES> fetch_tab;
  plane_table<mckpp_rec_plane, MCKPP_DEV_PLANES_MAX> rec_tab;
  plane_table<mckpp_put_plane, MCKPP_PUT_PLANES> put_tab;
  // Records reduced over levels and points (include/mckpp_hip_reduce.h).  The weights are indexed by point and by
  // level, not by resident column, so they live as long as the context and no upload touches them: on the device
  // (empty: not set), the two level arrays on the host too, where a plane's W is summed.  The scratch of the
  // reductions, each block grow-only: the slabs of terms (under a multi handle shard 0's serves every shard), and for
  // the host form the results on the device and the pinned block they are copied through.  m: the terms a workgroup
  // finishes (MCKPP_RED_M; MCKPP_REDUCE_M, tests: the halving pass on small planes).  ev_fill / ev_terms: behind shard
  // 0's fill, which the other shards' terms wait for, and behind a shard's terms, which shard 0's tree waits for.
  struct reduce_state {
    dev_buf<double> d_wp, d_wl, d_wi;
    std::vector<double> wl, wi;
    dev_buf<double> d_terms, d_out;
    pinned_buf<double> h_out;
    hip_event ev_fill, ev_terms;
    int m = MCKPP_RED_M;
  } red;
  plane_table<mckpp_red_plane, MCKPP_DEV_PLANES_MAX> red_tab;
  // The caller's vertical axes (include/mckpp_hip_vaxis.h).  An axis is the context's, like the weights above: its
  // levels on the host (empty: not defined) and the two tables on the device - `in`, nzp1 entries, the axis as the
  // source of zm(1:nzp1), and `out`, an entry per caller level, zm(1:nzp1) as its source.  h_zm is zm(1:nzp1), kept
  // for them.  The plane tables of the puts and the fetches, and the word the Kelvin rule of
  // mckpp_hip_vaxis_init_profiles raises between its two launches.
  struct vaxis {
    std::vector<double> z;
    dev_buf<mckpp_vaxis_ent> d_in, d_out;
    // the out table's branch and kin on the host: which model levels a caller level reads, for the level rule of
    // include/mckpp_hip_vrecords.h
    std::vector<int32_t> out_branch, out_kin;
  } vax[MCKPP_VAXES];
  std::vector<double> h_zm;
  plane_table<mckpp_vaxis_put_plane, MCKPP_VAXIS_PLANES> vput_tab;
  plane_table<mckpp_vaxis_fetch_plane, MCKPP_VAXIS_PLANES> vfetch_tab;
  plane_table<mckpp_vrec_plane, MCKPP_VREC_PLANES> vrec_tab;   // records on a caller axis (include/mckpp_hip_vrecords.h)
  dev_buf<unsigned> d_kelvin;
  // The caller's horizontal grids (include/mckpp_hip_hgrid.h).  A grid is the context's, like the axes above: n points
  // (0: not defined), the npts it was defined for and the copies of its two CSR tables on the host (ptr empty: that
  // direction is missing).  The device tables are the resident state's (mckpp_ctx_resident::hgd).  The plane table of
  // the second stage of mckpp_hip_hgrid_fetch_dev.
  struct hgrid_csr {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    std::vector<double> w;
    mckpp_hgrid_table_c view() const { return mckpp_hgrid_table_c{ptr.data(), idx.data(), w.data()}; }
  };
  struct hgrid {
    int64_t n = 0, npts = 0;
    hgrid_csr in, out;
  } hg[MCKPP_HGRIDS];
  plane_table<mckpp_hgrid_plane, MCKPP_HGRID_PLANES> hgrid_tab;
  plane_table<mckpp_remap_put_plane, MCKPP_REMAP_PLANES> rput_tab;   // mckpp_hip_remap_put_dev's (include/mckpp_hip_remap.h)
  plane_table<mckpp_hv_put_plane, MCKPP_HV_PLANES> hvput_tab;        // mckpp_hip_hv_put_dev's (include/mckpp_hip_hv.h)
  std::vector<int> peers;   // devices whose memory this context's device has been given peer access to
  int diag = 1;
  // optional-physics contexts: the relaxation / correction / advection inputs come with upload (or
  // update_ancillaries); load_restart does not carry them, so stepping is refused until they are there
  bool ext_inputs_resident = false;
};

extern "C" {

const char *mckpp_hip_last_error(void) { return g_err.c_str(); }

#ifndef MCKPP_BUILD_ID
#define MCKPP_BUILD_ID "unknown"
#endif
const char *mckpp_hip_build_id(void) { return MCKPP_BUILD_ID; }
#ifndef MCKPP_BUILD_COMPILER
#define MCKPP_BUILD_COMPILER "unknown"
#endif
const char *mckpp_hip_build_compiler(void) { return MCKPP_BUILD_COMPILER; }

int mckpp_hip_device_count(void)
{
  return entry(__func__, [&]() -> int {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail("hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
  });
}

// mckpp_physics_lookup, src/mckpp_physics_lookup_mod.F90:11-66 (host, libm pow).
void mckpp_host_lookup(double vonk, double *wmt, double *wst)
{
  const int ni = MCKPP_NI, nj = MCKPP_NJ, n1 = ni + 2;
  const double epsln = 1.e-20, c1 = 5.0, zmin = -4.e-7, zmax = 0.0, umin = 0.0, umax = 0.04;
  const double am = 1.257, cm = 8.380, c2 = 16.0, zetam = -0.2, as = -28.86, cs = 98.96, c3 = 16.0,
               zetas = -1.0;
  const double deltaz = (zmax - zmin) / (ni + 1);
  const double deltau = (umax - umin) / (nj + 1);
  for (int j = 0; j <= nj + 1; ++j) {
    const double usta = deltau * (j) + umin;
    const double u3 = (usta * usta) * usta;
    for (int i = 0; i <= ni + 1; ++i) {
      const double zehat = deltaz * (i) + zmin;
      const double zeta = zehat / (u3 + epsln);
      double wm, ws;
      if (zehat >= 0.) {
        wm = vonk * usta / (1. + c1 * zeta);
        ws = wm;
      } else {
        wm = (zeta > zetam) ? vonk * usta * std::pow(1. - c2 * zeta, 1. / 4.)
                            : vonk * std::pow(am * u3 - cm * zehat, 1. / 3.);
        // **(1./2.) is a square root in the reference's build (oracle/conv_probe.F90), not libm's pow
        ws = (zeta > zetas) ? vonk * usta * std::sqrt(1. - c3 * zeta)
                            : vonk * std::pow(as * u3 - cs * zehat, 1. / 3.);
      }
      wmt[(size_t)j * n1 + i] = wm;
      wst[(size_t)j * n1 + i] = ws;
    }
  }
}

// tri(0:nztmax,0:1,1), src/mckpp_initialize_ocean.F90:30-43.  zm, hm are zm(1:nzp1), hm(1:nzp1).
void mckpp_host_tri(int32_t nz, int32_t nztmax, double dto, const double *zm, const double *hm, double *tri)
{
  const int n1 = nztmax + 1;
  auto Z = [&](int k) { return zm[k - 1]; };
  auto H = [&](int k) { return hm[k - 1]; };
  double *t0 = tri, *t1 = tri + n1;
  for (int k = 0; k < n1; ++k) { t0[k] = 0.0; t1[k] = 0.0; }
  t1[0] = dto / H(1);
  t1[1] = dto / H(1) / (Z(1) - Z(2));
  for (int k = 2; k <= nz; ++k) {
    t1[k] = dto / H(k) / (Z(k) - Z(k + 1));
    t0[k] = dto / H(k) / (Z(k - 1) - Z(k));
  }
}

int mckpp_hip_init(const mckpp_const_c *c, int device, mckpp_hip_handle *out)
{
  return entry(__func__, [&]() -> int {
  if (!c || !out) return fail("mckpp_hip_init: null argument");
  if (c->nz < 2) return fail("mckpp_hip_init: nz=%d (need >= 2)", c->nz);
  if (c->nztmax < c->nz + 1) return fail("mckpp_hip_init: nztmax=%d < nzp1=%d", c->nztmax, c->nz + 1);
  if (!c->zm || !c->hm || !c->dm || !c->tri || !c->wmt || !c->wst)
    return fail("mckpp_hip_init: zm/hm/dm/tri/wmt/wst must all be set");
  // LKPP=.FALSE. is not a defined configuration of the reference: kppmix then never assigns hbl / kbl
  // (src/mckpp_physics_verticalmixing_kppmix_mod.F90:87-118 is skipped), which ocnstep stores as hmix / kmix and uses as
  // the index of dm() (src/mckpp_physics_ocnstep_mod.F90:305-314, ocnint_mod.F90:97-114) - uninitialised memory.  Refused.
  if (!c->LKPP) return fail("mckpp_hip_init: LKPP=.FALSE. leaves hmix/kmix unassigned in the reference (kppmix_mod.F90:87-118): not a defined configuration, not emulated");
  if (c->maxmodeadv < 0 || c->maxmodeadv > 16) return fail("mckpp_hip_init: maxmodeadv=%d", c->maxmodeadv);
  int solver_mode_env = 0;   // default of mckpp_hip_set_solver_mode
  if (const char *e = getenv("MCKPP_SOLVER_MODE")) {
    solver_mode_env = atoi(e);
    if (solver_mode_env < 0 || solver_mode_env > 1) return fail("mckpp_hip_init: MCKPP_SOLVER_MODE=%s (0: the reference's order, 1: two-ended)", e);
  }
  if (c->L_NO_ISOTHERM && (c->iso_bot < 2 || c->iso_bot > c->nz + 1))
    return fail("mckpp_hip_init: iso_bot=%d outside 2..nzp1", c->iso_bot);
  const int nzp1 = c->nz + 1;
  const int lpl = (nzp1 + 2 + 63) / 64;
  if (lpl > 8) return fail("mckpp_hip_init: nz=%d too deep (max 509 levels: profile rows are padded to at most 512 doubles)", c->nz);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("mckpp_hip_init: device %d of %d", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail("mckpp_hip_init: device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);

  // any failure below releases what has been created so far (the HIPCHK returns and a throw included)
  half_built<mckpp_hip_ctx, mckpp_hip_finalize> g(new mckpp_hip_ctx());
  mckpp_hip_ctx *h = g.get();
  h->device = device;
  h->c = *c;
  h->nz = c->nz;
  h->nzp1 = nzp1;
  h->lpl = lpl;
  h->ld = 64 * lpl;
  h->ldc = 64 * lpl + 8;
  h->num_cu = prop.multiProcessorCount;
  h->ext = c->LDD || c->L_RELAX_SST || c->L_FCORR || c->L_FCORR_WITHZ || c->L_SFCORR || c->L_SFCORR_WITHZ ||
           c->L_RELAX_SAL || c->L_RELAX_OCNT || c->L_NO_FREEZE || c->L_NO_ISOTHERM || c->L_DAMP_CURR ||
           c->clim_present || c->L_ADVECT;
  h->ext_kernel = c->LDD || c->L_RELAX_SST || c->L_FCORR || c->L_FCORR_WITHZ || c->L_SFCORR || c->L_SFCORR_WITHZ ||
                  c->L_RELAX_SAL || c->L_RELAX_OCNT || c->L_NO_FREEZE || c->L_NO_ISOTHERM || c->L_DAMP_CURR || c->L_ADVECT;
  HIPCHK(h->stream.create());
  HIPCHK(h->d_qhead.alloc(QBLOCK_INTS));   // queue heads [16], queue owners [16], straggler count and spare [32]
  h->solo_after = 12;
  h->solo_limit = std::max(2, h->num_cu / 32);
  if (const char *e = getenv("MCKPP_SOLO")) { if (atoi(e) == 0) h->solo_limit = 0; }
  if (const char *e = getenv("MCKPP_SOLO_LIMIT")) h->solo_limit = std::max(0, atoi(e));
  if (const char *e = getenv("MCKPP_SOLO_AFTER")) h->solo_after = std::max(0, atoi(e));
  if (const char *e = getenv("MCKPP_VIEW_KMAX")) h->view_kmax = std::max(0, atoi(e));
  {   // the device's XCDs (a column of a multi-step launch stays on one: mckpp_kernels_ps.hip, M0)
    HIPCHK(hipMemsetAsync(h->d_qhead, 0, sizeof(int), h->stream));
    HIPCHK(mckpp_launch_xcc_probe(reinterpret_cast<unsigned *>(h->d_qhead.get()), h->stream));
    unsigned mask = 0;
    HIPCHK(hipMemcpyAsync(&mask, h->d_qhead, sizeof mask, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->nqueues = 0;
    for (int i = 0; i < 16; ++i) h->xcc_queue[i] = (mask >> i & 1u) ? h->nqueues++ : -1;
    if (h->nqueues == 0) h->multistep = false;
    // HIP promises nothing about where workgroups run: a launch may leave an XCD the probe saw without any (its queue is
    // then adopted, whole, by another XCD: k_column_ps M0), or run workgroups on one the probe did not see (they start
    // without a queue and adopt one, or end).  MCKPP_XCC_DROP=<bit mask of XCC ids> takes the queue away from those XCDs'
    // workgroups - the queues stay - so that both paths run on a device where they otherwise never would (tests).
    if (const char *e = getenv("MCKPP_XCC_DROP")) {
      const unsigned drop = (unsigned)strtoul(e, nullptr, 0);
      for (int i = 0; i < 16; ++i) if (drop >> i & 1u) h->xcc_queue[i] = -1;
    }
    if (getenv("MCKPP_PS_VERBOSE"))
      fprintf(stderr, "[mckpp] XCC ids seen by the probe: mask 0x%x, %d queues\n", mask, h->nqueues);
  }
  HIPCHK(h->d_params.alloc(1));
  h->scratch_doubles = mckpp_ps_scratch_doubles(nzp1, h->ext_kernel ? (c->LDD ? 2 : 1) : 0, h->num_cu);
  HIPCHK(h->d_scratch.alloc(h->scratch_doubles));
  HIPCHK(hipMemset(h->d_scratch, 0, h->scratch_doubles * sizeof(double)));
  if (getenv("MCKPP_STAMP")) {
    HIPCHK(h->d_dbg.alloc(40));
    HIPCHK(hipMemset(h->d_dbg, 0, 40 * sizeof(unsigned long long)));
  }
  HIPCHK(h->ev0.create(hipEventDefault));   // the two that are timed (mckpp_hip_last_kernel_ms)
  HIPCHK(h->ev1.create(hipEventDefault));
  HIPCHK(h->copy_stream.create());
  for (int b = 0; b < 2; ++b) {
    HIPCHK(h->ev_lay[b].create());
    HIPCHK(h->ev_copy[b].create());
  }
  HIPCHK(h->ev_f.create());
  HIPCHK(h->h_params.prepare(1));

  const int ldc = h->ldc, nz = h->nz, n1 = c->nztmax + 1;
  std::vector<double> zm(ldc, 0.0), hm(ldc, 0.0), t0(ldc, 0.0), t1(ldc, 0.0);
  for (int k = 1; k <= nzp1; ++k) { zm[k] = c->zm[k - 1]; hm[k] = c->hm[k - 1]; }
  for (int k = 0; k <= nz; ++k) { t0[k] = c->tri[k]; t1[k] = c->tri[n1 + k]; }
  h->dm_nz = c->dm[nz];
  {   // layers above a tenth of the deepest level's depth = trips of the reference-level loop (verticalmixing_mod.F90:118-131)
      // of that level: 6 on a uniform 60-level grid, 10 at 100 levels, 25 on the stretched 69-level grid.  From 16 on, the
      // extra phase that forms the whole-layer terms once per column pays (measured: +2 % on the stretched grid, -0.7 % at 60)
    int nref = 0;
    for (int k = 1; k <= nz; ++k) nref += c->zm[k - 1] > 0.1 * c->zm[nz - 1];
    h->l2pre = (nref >= 16 && !c->LDD) ? 1 : 0;
    if (const char *e = getenv("MCKPP_L2PRE")) h->l2pre = (atoi(e) != 0 && !c->LDD) ? 1 : 0;
    if (const char *e = getenv("MCKPP_L3_CAP")) h->l3cap = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = getenv("MCKPP_REDUCE_M")) {   // a power of two 64 .. MCKPP_RED_M, else the default
      const int v = atoi(e);
      if (v >= 64 && v <= MCKPP_RED_M && (v & (v - 1)) == 0) h->red.m = v;
    }
    // the guesses L3 works from (profiles/r06: the margins' sweep).  MCKPP_FIRST_GUESS=0 is the rule before them: every
    // level in a column's first pass, the scan's end plus eight after it (A/B runs, tests)
    if (const char *e = getenv("MCKPP_FIRST_MARGIN")) h->first_margin = std::min(std::max(0, atoi(e)), 0xffff);
    if (const char *e = getenv("MCKPP_GUESS_MARGIN")) h->guess_margin = std::min(std::max(0, atoi(e)), 0xffff);
    if (const char *e = getenv("MCKPP_FIRST_GUESS")) {
      if (atoi(e) == 0) { h->first_guess = 0; h->guess_margin = 8; }
    }
    h->solver_mode = solver_mode_env;
    if (const char *e = getenv("MCKPP_MULTISTEP")) h->multistep = atoi(e) != 0 && h->nqueues > 0;
  }
  auto up = [&](dev_buf<double> &dst, const double *src, size_t n) -> hipError_t {
    hipError_t e = dst.alloc(n);
    if (e != hipSuccess) return e;
    return hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice);
  };
  {
    std::vector<double> dm(ldc, 0.0), hs(ldc, 0.0);
    for (int k = 0; k <= nz; ++k) dm[k] = c->dm[k];
    double acc = 0.0;
    for (int n = 1; n <= nzp1; ++n) { acc = acc + hm[n]; hs[n] = acc; }
    HIPCHK(up(h->d_dm, dm.data(), ldc));
    HIPCHK(up(h->d_hsum, hs.data(), ldc));
  }
  // Jerlov tables: swfrac_opt (swfrac_mod.F90:36-41, fact = hbf = 1) and swdk_opt (fluxes_mod.F90:104-107)
  h->h_swfrac_tab.assign((size_t)6 * ldc, 0.0);
  h->h_swdk_tab.assign((size_t)6 * ldc, 0.0);
  for (int jw = 1; jw <= 5; ++jw) {
    for (int l = 1; l <= nzp1; ++l) {
      const double rmin = -80.;
      double r1 = zm[l] * 1.0 / jer_a1[jw]; r1 = r1 > rmin ? r1 : rmin;
      double r2 = zm[l] * 1.0 / jer_a2[jw]; r2 = r2 > rmin ? r2 : rmin;
      h->h_swfrac_tab[(size_t)jw * ldc + l] = jer_rfac[jw] * mckpp_exp(r1) + (1. - jer_rfac[jw]) * mckpp_exp(r2);
    }
    for (int k = 0; k <= nz; ++k) {
      const double z = -c->dm[k];
      h->h_swdk_tab[(size_t)jw * ldc + k] =
          jer_rfac[jw] * mckpp_exp(z / jer_a1[jw]) + (1.0 - jer_rfac[jw]) * mckpp_exp(z / jer_a2[jw]);
    }
  }
  {  // bldepth_mod.F90:91 and blmix_mod.F90:62
    const double cv = 1.6, cs = 98.96, epsilon = 0.1, Ricr = 0.30, cstar = 5.0;
    h->Vtc = cv * std::sqrt(0.2 / cs / epsilon) / (c->vonk * c->vonk) / Ricr;
    h->cg = cstar * c->vonk * std::pow(cs * c->vonk * epsilon, 1. / 3.);
  }
  const size_t nt = (size_t)(MCKPP_NI + 2) * (MCKPP_NJ + 2);
  std::vector<double2> wtab(nt);
  for (size_t i = 0; i < nt; ++i) wtab[i] = make_double2(c->wmt[i], c->wst[i]);

  HIPCHK(up(h->d_zm, zm.data(), ldc));
  h->h_zm.assign(c->zm, c->zm + nzp1);
  HIPCHK(up(h->d_hm, hm.data(), ldc));
  HIPCHK(up(h->d_tri0, t0.data(), ldc));
  HIPCHK(up(h->d_tri1, t1.data(), ldc));
  HIPCHK(up(h->d_swfrac_tab, h->h_swfrac_tab.data(), (size_t)6 * ldc));
  HIPCHK(up(h->d_swdk_tab, h->h_swdk_tab.data(), (size_t)6 * ldc));
  HIPCHK(h->d_wtab.alloc(nt));
  HIPCHK(hipMemcpy(h->d_wtab, wtab.data(), nt * sizeof(double2), hipMemcpyHostToDevice));
  // the host pointers are not kept
  h->c.zm = h->c.hm = h->c.dm = h->c.tri = h->c.wmt = h->c.wst = nullptr;
  *out = g.release();
  return 0;
  });
}

static int win_cancel_all(mckpp_hip_ctx *h);
static int snap_cancel(mckpp_hip_ctx *h);
static int log_cancel(mckpp_hip_ctx *h);
static int bt_cancel(mckpp_hip_ctx *h);
static int anc_cancel_all(mckpp_hip_ctx *h);
static int ring_cancel(mckpp_hip_ctx *h);

// Everything sized to the resident columns goes.  No wait here: the callers have cancelled the schedules, which waits
// for the launches that may still use their records.
static void free_state(mckpp_hip_ctx *h) { static_cast<mckpp_ctx_resident &>(*h) = mckpp_ctx_resident{}; }

// The caller's arrays stay pinned until the context goes (or mckpp_hip_release_host_arrays is called)
static void unpin_all(mckpp_hip_ctx *h)
{
  for (auto &r : h->pinned)
    if (hipHostUnregister(const_cast<void *>(r.first)) != hipSuccess) (void)hipGetLastError();
  h->pinned.clear();
  h->unpinnable.clear();
}

int mckpp_hip_finalize(mckpp_hip_handle h)
{
  if (!h) return 0;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);   // nothing in flight may still use what the owners release
  if (h->copy_stream) hipStreamSynchronize(h->copy_stream);
  if (h->snap_stream) hipStreamSynchronize(h->snap_stream);
  if (h->flux_stream) hipStreamSynchronize(h->flux_stream);
  unpin_all(h);
  delete h;
  return 0;
}

int64_t mckpp_hip_ncolumns(mckpp_hip_handle h) { return h ? h->ncol : -1; }

static int ensure_stage(mckpp_hip_ctx *h, size_t elems)
{
  if (elems <= h->d_stage.size()) return 0;
  // a fluxes / unpack / window kernel queued by an earlier call may still be reading the block (those calls do not
  // end with a synchronisation): wait for this context's stream, not - through hipFree - for the whole device
  if (h->d_stage) HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(h->d_stage.reserve(elems));
  return 0;
}

// MCKPP_HIP_NO_HOST_REGISTER=1: never pin the caller's arrays (transfers then go through the runtime's own
// pageable path: correct, several times slower)
static bool no_host_register()
{
  static const bool v = getenv("MCKPP_HIP_NO_HOST_REGISTER") != nullptr;
  return v;
}

// Pin a caller array once (portable: every device's transfers benefit).  Failure is not an error: an array that
// is already pinned (by another context, or by the caller) or cannot be is simply transferred as it is.
static void pin_host(mckpp_hip_ctx *h, const void *ptr, size_t bytes)
{
  if (!ptr || bytes < ((size_t)1 << 18) || no_host_register()) return;
  const char *b = static_cast<const char *>(ptr);
  for (auto &r : h->pinned)        // inside a range this context pinned
    if (b >= static_cast<const char *>(r.first) && b + bytes <= static_cast<const char *>(r.first) + r.second) return;
  for (auto &r : h->unpinnable)    // tried before: pinned by someone else, or cannot be
    if (r.first == ptr && r.second == bytes) return;
  static const bool verbose = getenv("MCKPP_HIP_VERBOSE") != nullptr;
  const hipError_t e = hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterPortable);
  if (e == hipSuccess) h->pinned.emplace_back(ptr, bytes);
  else { (void)hipGetLastError(); h->unpinnable.emplace_back(ptr, bytes); }
  if (verbose) fprintf(stderr, "[mckpp] hipHostRegister(%p, %zu B): %s\n", ptr, bytes, e == hipSuccess ? "pinned" : hipGetErrorString(e));
}

static int ensure_xfer(mckpp_hip_ctx *h, unsigned b, size_t elems)
{
  if (elems <= h->d_xfer[b].size()) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));        // nothing in flight may still use the buffer
  HIPCHK(hipStreamSynchronize(h->copy_stream));
  HIPCHK(h->d_xfer[b].reserve(elems));
  return 0;
}

// host Fortran slab (npts x nlev, from `src`) -> device rows.  Queued: the copy on the copy stream, the layout
// kernel behind it on the context's stream; the caller waits for the stream before `src` may change.
static int up_rows(mckpp_hip_ctx *h, const double *src, int nlev, double *dst, int dst_off, const double *whole = nullptr,
                   size_t whole_elems = 0)
{
  const size_t n = (size_t)h->npts * nlev;
  const unsigned b = h->xfer_seq++ & 1u;
  if (ensure_xfer(h, b, n)) return -1;
  // the array the slab belongs to is pinned as a whole (slabs of one array share pages at their boundaries)
  if (whole) pin_host(h, whole, whole_elems * sizeof(double));
  else pin_host(h, src, n * sizeof(double));
  HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_lay[b], 0));   // the layout kernel that last read this buffer
  HIPCHK(hipMemcpyAsync(h->d_xfer[b], src, n * sizeof(double), hipMemcpyHostToDevice, h->copy_stream));
  HIPCHK(hipEventRecord(h->ev_copy[b], h->copy_stream));
  HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copy[b], 0));
  HIPCHK(mckpp_launch_gather_rows(h->d_xfer[b], h->npts, nlev, 0, h->d_ipt, h->ncol, dst, h->ld, dst_off, h->stream));
  HIPCHK(hipEventRecord(h->ev_lay[b], h->stream));
  return 0;
}

// device rows -> host Fortran slab; entries of non-resident (land) columns keep their host values.  Queued: the
// layout kernel on the context's stream, the copy to the host behind it on the copy stream; xfer_finish() before
// the caller reads `dst`.
// The general form: `nrow` rows, row r at point map[r] (a device array) of `npts` points.
static int down_rows_map(mckpp_hip_ctx *h, const double *src, int src_ld, int src_off, int nlev, double *dst, const int *map,
                         int64_t nrow, int64_t npts, const double *whole = nullptr, size_t whole_elems = 0)
{
  const size_t n = (size_t)npts * nlev;
  const unsigned b = h->xfer_seq++ & 1u;
  if (ensure_xfer(h, b, n)) return -1;
  if (whole) pin_host(h, whole, whole_elems * sizeof(double));
  else pin_host(h, dst, n * sizeof(double));
  HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copy[b], 0));   // the transfer that last read this buffer
  if (nrow < npts)
    HIPCHK(hipMemcpyAsync(h->d_xfer[b], dst, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(mckpp_launch_scatter_rows(src, src_ld, src_off, map, nrow, h->d_xfer[b], npts, nlev, 0, h->stream));
  HIPCHK(hipEventRecord(h->ev_lay[b], h->stream));
  HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_lay[b], 0));
  HIPCHK(hipMemcpyAsync(dst, h->d_xfer[b], n * sizeof(double), hipMemcpyDeviceToHost, h->copy_stream));
  HIPCHK(hipEventRecord(h->ev_copy[b], h->copy_stream));
  return 0;
}

static int down_rows(mckpp_hip_ctx *h, const double *src, int src_ld, int src_off, int nlev, double *dst,
                     const double *whole = nullptr, size_t whole_elems = 0)
{
  return down_rows_map(h, src, src_ld, src_off, nlev, dst, h->d_ipt, h->ncol, h->npts, whole, whole_elems);
}

static int xfer_finish(mckpp_hip_ctx *h)
{
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->copy_stream));
  return 0;
}

// Device buffers of the column state for `ncol` resident columns out of `npts` grid points (every
// row zeroed).  Used by upload and by load_restart, so a context with the optional physics gets
// its input/output rows and per-column records from either.
static int alloc_state(mckpp_hip_ctx *h, int64_t npts, int64_t ncol)
{
  free_state(h);
  h->ext_inputs_resident = false;
  mckpp_ctx_resident n;   // built here and moved in whole: a failure leaves the context without a state, not with half of one
  n.npts = npts;
  n.ncol = ncol;
  if (ncol > 0) {
    auto zeroed = [&](auto &p, size_t elems) -> hipError_t {
      const hipError_t e = p.alloc(elems);
      return e != hipSuccess ? e : hipMemsetAsync(p, 0, elems * sizeof(*p.get()), h->stream);
    };
    const size_t rowelems = (size_t)ncol * h->ld;
    for (auto &p : n.d_prof) HIPCHK(zeroed(p, rowelems));
    for (auto &p : n.d_diag) HIPCHK(zeroed(p, rowelems));
    HIPCHK(n.d_cs.alloc((size_t)ncol * MCKPP_CS));
    HIPCHK(n.d_ci.alloc((size_t)ncol * MCKPP_CI));
    HIPCHK(n.d_ipt.alloc((size_t)ncol));
    HIPCHK(n.h_cs.alloc((size_t)ncol * MCKPP_CS));
    HIPCHK(n.h_ci.alloc((size_t)ncol * MCKPP_CI));
    if (h->ext) {
      for (auto &p : n.d_ext_in) HIPCHK(zeroed(p, rowelems));
      for (auto &p : n.d_ext_out) HIPCHK(zeroed(p, rowelems));
      const size_t nadv = (size_t)ncol * (h->c.maxmodeadv + 1);
      HIPCHK(zeroed(n.d_xs, (size_t)ncol * MCKPP_XS));
      HIPCHK(zeroed(n.d_adv_d, nadv));
      HIPCHK(zeroed(n.d_adv_i, nadv));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  static_cast<mckpp_ctx_resident &>(*h) = std::move(n);
  return 0;
}

// A new state arrives (upload, load_restart) for the resident columns `ipt` of `npts` grid points: whatever was built
// on the old state goes, the device state is allocated anew if its shape changes, the column map is handed over.  The
// two callers differ in this: an upload keeps the flux ring when the column map and npts are unchanged, a restart load
// always cancels it; and a restart load under another column map marks the optional-physics inputs as not resident -
// they were compacted with the old map and the file carries none - where an upload sends its own right afterwards.
static int new_state(mckpp_hip_ctx *h, int64_t npts, const std::vector<int> &ipt, bool from_restart)
{
  if (win_cancel_all(h)) return -1;   // the output schedules' records are of the old state
  if (snap_cancel(h)) return -1;      // ... and the restart schedule's snapshots
  if (log_cancel(h)) return -1;       // ... and the step log's records (they name resident columns)
  if (bt_cancel(h)) return -1;        // ... and the resident bottom temperature (the column map may change)
  if (anc_cancel_all(h)) return -1;   // ... and the ancillary record series and their schedules (likewise)
  const bool new_map = ipt != h->ipt;
  // the flux ring's records were compacted with the previous column map (it waits for what it has queued)
  if ((from_restart || new_map || npts != h->npts) && ring_cancel(h)) return -1;
  if ((int64_t)ipt.size() != h->ncol || npts != h->npts) {
    if (alloc_state(h, npts, (int64_t)ipt.size())) return -1;
  }
  if (new_map) {
    if (h->d_series) {   // resident flux records were compacted with the previous land mask
      h->d_series.reset();
      h->series_nrec = 0;
    }
    h->land_kind = 0;   // the list of non-resident points was of the previous column map
    for (auto &g : h->hgd) g.in.kind = g.out.kind = 0;   // ... and so were the device tables of the caller's grids (hgrid_build waits, then rebuilds)
    if (from_restart) h->ext_inputs_resident = false;
    h->ipt = ipt;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The caller's mckpp_state_ptrs_c <-> the device-resident state, stated once: upload, download and the restart set
// (restart_segments) read it here.
// ---------------------------------------------------------------------------
namespace {
using host_state = mckpp_state_ptrs_c;
enum { A_PROF, A_DIAG, A_CORR };        // d_prof, d_diag, d_ext_out: the correction rows, where the context carries them
enum { L_NZP1, L_NZP2, L_NZ, L_NZ1 };   // level counts: nzp1, nzp1 + 1, nz, nz + 1
enum { T_UP = 1, T_DOWN = 2 };

// Row fields.  Slab `slab` of the `nslabs` of the member's array that the library reads or writes (transferred one by
// one, pinned as a whole) is `lev` levels from element `off` of row `row` of the device array `arr`; a slab is nzp1
// levels long, or (tmax) nztmax + 1.  The order is that of the transfers of an upload and of a download.
struct row_field { double *host_state::*member; int slab, nslabs; bool tmax; int arr, row, off, lev; uint32_t group; int dir; };
const row_field row_fields[] = {
  {&host_state::U,  0, 2, false, A_PROF, P_U,   0, L_NZP1, MCKPP_F_PROFILES, T_UP | T_DOWN},
  {&host_state::U,  1, 2, false, A_PROF, P_V,   0, L_NZP1, MCKPP_F_PROFILES, T_UP | T_DOWN},
  {&host_state::X,  0, 2, false, A_PROF, P_T,   0, L_NZP1, MCKPP_F_PROFILES, T_UP | T_DOWN},
  {&host_state::X,  1, 2, false, A_PROF, P_S,   0, L_NZP1, MCKPP_F_PROFILES, T_UP | T_DOWN},
  {&host_state::Us, 0, 4, false, A_PROF, P_US0, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},   // Us(npts,nzp1,nvel,0:1)
  {&host_state::Us, 1, 4, false, A_PROF, P_VS0, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Us, 2, 4, false, A_PROF, P_US1, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Us, 3, 4, false, A_PROF, P_VS1, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Xs, 0, 4, false, A_PROF, P_TS0, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Xs, 1, 4, false, A_PROF, P_SS0, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Xs, 2, 4, false, A_PROF, P_TS1, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::Xs, 3, 4, false, A_PROF, P_SS1, 0, L_NZP1, MCKPP_F_SAVED, T_UP | T_DOWN},
  {&host_state::U_init, 0, 2, false, A_PROF, P_UINIT, 0, L_NZP1, 0, T_UP},
  {&host_state::U_init, 1, 2, false, A_PROF, P_VINIT, 0, L_NZP1, 0, T_UP},
  {&host_state::rho,   0, 1, false, A_DIAG, D_RHO,   0, L_NZP2, MCKPP_F_DIAG, T_DOWN},
  {&host_state::cp,    0, 1, false, A_DIAG, D_CP,    0, L_NZP2, MCKPP_F_DIAG, T_DOWN},
  {&host_state::buoy,  0, 1, false, A_DIAG, D_BUOY,  1, L_NZP1, MCKPP_F_DIAG, T_DOWN},
  {&host_state::difm,  0, 1, false, A_DIAG, D_DIFM,  0, L_NZP2, MCKPP_F_DIAG, T_DOWN},
  {&host_state::difs,  0, 1, false, A_DIAG, D_DIFS,  0, L_NZP2, MCKPP_F_DIAG, T_DOWN},
  {&host_state::dift,  0, 1, false, A_DIAG, D_DIFT,  0, L_NZP2, MCKPP_F_DIAG, T_DOWN},
  {&host_state::ghat,  0, 1, false, A_DIAG, D_GHAT,  1, L_NZ,   MCKPP_F_DIAG, T_DOWN},
  {&host_state::wU,    0, 2, true,  A_DIAG, D_WU1,   0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::wU,    1, 2, true,  A_DIAG, D_WU2,   0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::wX,    0, 3, true,  A_DIAG, D_WX1,   0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::wX,    1, 3, true,  A_DIAG, D_WX2,   0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::wX,    2, 3, true,  A_DIAG, D_WX3,   0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::wXNT,  0, 1, true,  A_DIAG, D_WXNT1, 0, L_NZ1,  MCKPP_F_DIAG, T_DOWN},
  {&host_state::Rig,   0, 1, false, A_DIAG, D_RIG,   1, L_NZ,   MCKPP_F_DIAG, T_DOWN},
  {&host_state::Shsq,  0, 1, false, A_DIAG, D_SHSQ,  1, L_NZ,   MCKPP_F_DIAG, T_DOWN},
  {&host_state::dbloc, 0, 1, false, A_DIAG, D_DBLOC, 1, L_NZ,   MCKPP_F_DIAG, T_DOWN},
  {&host_state::tinc_fcorr, 0, 1, false, A_CORR, O_TINC,     1, L_NZP1, MCKPP_F_DIAG, T_DOWN},
  {&host_state::sinc_fcorr, 0, 1, false, A_CORR, O_SINC,     1, L_NZP1, MCKPP_F_DIAG, T_DOWN},
  {&host_state::ocnTcorr,   0, 1, false, A_CORR, O_OCNTCORR, 1, L_NZP1, MCKPP_F_DIAG, T_DOWN},
  {&host_state::scorr,      0, 1, false, A_CORR, O_SCORR,    1, L_NZP1, MCKPP_F_DIAG, T_DOWN},
};

// Per-column records.  The member's entry at npts * (off + off_nsflxs * nsflxs) - sflux(:,1:6,5,0) lies four times
// (npts,nsflxs) in - is slot `slot`; an upload stores `def` for a NULL member; a download of `group` brings the slot
// back (0: it never comes back), ext_only: on a context with the optional physics alone.  The order is that of a
// download's packed slabs.
struct rec_double { double *host_state::*member; int off, off_nsflxs, slot; double def; uint32_t group; bool ext_only; };
struct rec_int { int32_t *host_state::*member; int slot, def; uint32_t group; };
constexpr rec_double rec_doubles[] = {
  {&host_state::hmixd, 0, 0, CS_HMIXD0, 0.0, MCKPP_F_SAVED},
  {&host_state::hmixd, 1, 0, CS_HMIXD1, 0.0, MCKPP_F_SAVED},
  {&host_state::hmix, 0, 0, CS_HMIX, 0.0, MCKPP_F_SCALARS},
  {&host_state::kmix, 0, 0, CS_KMIX, 0.0, MCKPP_F_SCALARS},
  {&host_state::Tref, 0, 0, CS_TREF, 0.0, MCKPP_F_SCALARS},
  {&host_state::uref, 0, 0, CS_UREF, 0.0, MCKPP_F_SCALARS},
  {&host_state::vref, 0, 0, CS_VREF, 0.0, MCKPP_F_SCALARS},
  {&host_state::Ssurf, 0, 0, CS_SSURF, 0.0, MCKPP_F_SCALARS},
  {&host_state::reset_flag, 0, 0, CS_RESET, 0.0, MCKPP_F_SCALARS},
  {&host_state::dampu_flag, 0, 0, CS_DAMPU, 0.0, MCKPP_F_SCALARS},
  {&host_state::dampv_flag, 0, 0, CS_DAMPV, 0.0, MCKPP_F_SCALARS},
  {&host_state::freeze_flag, 0, 0, CS_FREEZE, 0.0, MCKPP_F_SCALARS},
  {&host_state::fcorr, 0, 0, CS_FCORR, 0.0, MCKPP_F_SCALARS, true},
  {&host_state::sflux, 0, 4, CS_SFLUX1, 0.0, MCKPP_F_SCALARS},   // sflux(:,1:6,5,0)
  {&host_state::sflux, 1, 4, CS_SFLUX2, 0.0, MCKPP_F_SCALARS},
  {&host_state::sflux, 2, 4, CS_SFLUX3, 0.0, MCKPP_F_SCALARS},
  {&host_state::sflux, 3, 4, CS_SFLUX4, 0.0, MCKPP_F_SCALARS},
  {&host_state::sflux, 4, 4, CS_SFLUX5, 0.0, MCKPP_F_SCALARS},
  {&host_state::sflux, 5, 4, CS_SFLUX6, 0.0, MCKPP_F_SCALARS},
  {&host_state::f, 0, 0, CS_F, 0.0, 0},
  {&host_state::Sref, 0, 0, CS_SREF, 0.0, 0},
  {&host_state::SSref, 0, 0, CS_SSREF, 0.0, 0},
  {&host_state::ocdepth, 0, 0, CS_OCDEPTH, -10000.0, 0},
};
constexpr rec_int rec_ints[] = {
  {&host_state::old, CI_OLD, 0, MCKPP_F_SAVED},
  {&host_state::new_, CI_NEW, 1, MCKPP_F_SAVED},
  {&host_state::l_initflag, CI_INITFLAG, 0, MCKPP_F_SCALARS},
  {&host_state::jerlov, CI_JERLOV, 3, 0},
  {&host_state::l_ocean, CI_LOCEAN, 1, 0},
};
static_assert(std::size(rec_doubles) <= MCKPP_CS && std::size(rec_ints) <= MCKPP_CI, "a slot per entry at the most");

// where the entry lies in the member's array
static int64_t rec_offset(const mckpp_hip_ctx *h, const rec_double &e)
{
  return h->npts * (e.off + (int64_t)e.off_nsflxs * h->c.nsflxs);
}

// One row field of a state view on one context: the device rows, the first element taken and the level count, the slab
// in the caller's array, and that array as a whole with its size - what gets pinned (null: the slab alone)
struct row_xfer { double *dev; int off, nlev; double *host; const double *whole; size_t whole_elems; };

// The row fields of direction `dir` and of the groups in `mask` whose member `s` sets.  The list depends on these and
// the pointers only, so the contexts of a multi-device handle produce lists that correspond entry by entry.
static void row_plan(mckpp_hip_ctx *h, const mckpp_state_ptrs_c *s, int dir, uint32_t mask, std::vector<row_xfer> &plan)
{
  const int levels[] = {h->nzp1, h->nzp1 + 1, h->nz, h->nz + 1};
  for (const row_field &f : row_fields) {
    double *a = s->*f.member;
    if (!(f.dir & dir) || !a || (dir == T_DOWN && !(f.group & mask))) continue;
    if (f.arr == A_CORR && !h->d_ext_out[O_TINC]) continue;   // (a context of the default physics has them only once something needed them)
    double *dev = f.arr == A_PROF ? h->d_prof[f.row] : f.arr == A_DIAG ? h->d_diag[f.row] : h->d_ext_out[f.row];
    const size_t slab = (size_t)h->npts * (f.tmax ? h->c.nztmax + 1 : h->nzp1);
    plan.push_back({dev, f.off, levels[f.lev], a + f.slab * slab, f.nslabs > 1 ? a : nullptr, f.nslabs * slab});
  }
}
}  // namespace

// Inputs of the optional physics: what mckpp_boundary_update and the ancillary readers
// rewrite on the host between steps (src/mckpp_ocean_model_3D.F90:51-55) - relaxation times and targets,
// flux corrections, climatologies, prescribed advection.  Rows go through the staging buffer; the
// per-column scalars are compacted on the host.
static int upload_ancillaries(mckpp_hip_ctx *h, const mckpp_state_ptrs_c *s, const char *who)
{
  const mckpp_const_c &k = h->c;
  const int64_t npts = h->npts, ncol = h->ncol;
  const int nzp1 = h->nzp1;
  const std::vector<int> &ipt = h->ipt;
  if ((k.L_FCORR_WITHZ && !s->fcorr_withz) || (k.L_SFCORR_WITHZ && !s->sfcorr_withz) ||
      ((k.L_RELAX_OCNT || k.clim_present || k.L_NO_ISOTHERM) && !s->ocnT_clim) ||
      ((k.L_RELAX_SAL || k.clim_present || k.L_NO_ISOTHERM) && !s->sal_clim) ||
      (k.L_RELAX_SST && (!s->relax_sst || !s->SST0)) || (k.L_FCORR && !s->fcorr_twod) ||
      (k.L_RELAX_SAL && !s->relax_sal) || (k.L_RELAX_OCNT && !s->relax_ocnT))
    return fail("%s: a switch is on but the field it reads is a NULL pointer", who);
  const int mm = k.maxmodeadv;
  // the advection slots, checked before anything is copied: a refused call leaves the resident inputs as they were
  for (int64_t c = 0; k.L_ADVECT && s->nmodeadv && c < ncol; ++c) {
    const int64_t i = ipt[c];
    const int nm = s->nmodeadv[i + npts * 1];   // nmodeadv(ipt,2)
    if (nm < 0 || nm > mm) return fail("%s: nmodeadv(%lld,2)=%d outside 0..%d", who, (long long)i + 1, nm, mm);
    for (int j = 0; j < nm; ++j) {   // a live slot above 7: the reference aborts (solvers.F90:320-323), the kernel would skip it
      const int mode = s->modeadv ? s->modeadv[i + npts * (j + (int64_t)mm * 1)] : 0;   // modeadv(ipt,j+1,2)
      if (mode > 7)
        return fail("%s: modeadv(%lld,%d,2)=%d is no mode of rhsmod (1..7; 0 or less switches a slot off)", who,
                    (long long)i + 1, j + 1, mode);
    }
  }
  if (s->fcorr_withz && up_rows(h, s->fcorr_withz, nzp1, h->d_ext_in[E_FCORR_WITHZ], 0)) return -1;
  if (s->sfcorr_withz && up_rows(h, s->sfcorr_withz, nzp1, h->d_ext_in[E_SFCORR_WITHZ], 0)) return -1;
  if (s->ocnT_clim && up_rows(h, s->ocnT_clim, nzp1, h->d_ext_in[E_OCNT_CLIM], 0)) return -1;
  if (s->sal_clim && up_rows(h, s->sal_clim, nzp1, h->d_ext_in[E_SAL_CLIM], 0)) return -1;
  std::vector<double> xs((size_t)ncol * MCKPP_XS, 0.0), ad((size_t)ncol * (mm + 1), 0.0);
  std::vector<int> ai((size_t)ncol * (mm + 1), 0);
  for (int64_t c = 0; c < ncol; ++c) {
    const int64_t i = ipt[c];
    double *x = &xs[(size_t)c * MCKPP_XS];
    x[XS_RELAX_SST] = s->relax_sst ? s->relax_sst[i] : 0.0;
    x[XS_SST0] = s->SST0 ? s->SST0[i] : 0.0;
    x[XS_FCORR_TWOD] = s->fcorr_twod ? s->fcorr_twod[i] : 0.0;
    x[XS_RELAX_SAL] = s->relax_sal ? s->relax_sal[i] : 0.0;
    x[XS_RELAX_OCNT] = s->relax_ocnT ? s->relax_ocnT[i] : 0.0;
    ai[(size_t)c * (mm + 1)] = (k.L_ADVECT && s->nmodeadv) ? s->nmodeadv[i + npts * 1] : 0;   // nmodeadv(ipt,2)
    for (int j = 0; j < mm; ++j) {
      ai[(size_t)c * (mm + 1) + 1 + j] = s->modeadv ? s->modeadv[i + npts * (j + (int64_t)mm * 1)] : 0;
      ad[(size_t)c * (mm + 1) + j] = s->advection ? s->advection[i + npts * (j + (int64_t)mm * 1)] : 0.0;
    }
  }
  HIPCHK(hipMemcpy(h->d_xs, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_adv_d, ad.data(), ad.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_adv_i, ai.data(), ai.size() * sizeof(int), hipMemcpyHostToDevice));
  h->ext_inputs_resident = true;
  return 0;
}

static void fill_params(mckpp_hip_ctx *h, mckpp_kparams &p, int ntime, int mode);

int mckpp_hip_upload(mckpp_hip_handle h, const mckpp_state_ptrs_c *s)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!s) return fail("mckpp_hip_upload: null argument");
  if (s->npts <= 0) return fail("mckpp_hip_upload: npts=%lld", (long long)s->npts);
  if (!s->U || !s->X) return fail("mckpp_hip_upload: U and X are required");
  HIPCHK(hipSetDevice(h->device));
  const int64_t npts = s->npts;
  std::vector<int> ipt;
  ipt.reserve(npts);
  for (int64_t i = 0; i < npts; ++i)
    if (!s->run_physics || s->run_physics[i]) ipt.push_back((int)i);
  const int64_t ncol = (int64_t)ipt.size();
  if (new_state(h, npts, ipt, false)) return -1;
  if (ncol == 0) return 0;
  HIPCHK(hipMemcpyAsync(h->d_ipt, ipt.data(), (size_t)ncol * sizeof(int), hipMemcpyHostToDevice, h->stream));
  std::vector<row_xfer> plan;
  row_plan(h, s, T_UP, ~0u, plan);
  for (const row_xfer &x : plan)
    if (up_rows(h, x.host, x.nlev, x.dev, x.off, x.whole, x.whole_elems)) return -1;
  if (h->ext && upload_ancillaries(h, s, who)) return -1;
  std::vector<double> cs((size_t)ncol * MCKPP_CS, 0.0);
  std::vector<int> ci((size_t)ncol * MCKPP_CI, 0);
  const double *srcd[std::size(rec_doubles)];   // the members' entries, resolved outside the loop over the columns
  const int32_t *srci[std::size(rec_ints)];
  for (size_t j = 0; j < std::size(rec_doubles); ++j)
    srcd[j] = s->*rec_doubles[j].member ? s->*rec_doubles[j].member + rec_offset(h, rec_doubles[j]) : nullptr;
  for (size_t j = 0; j < std::size(rec_ints); ++j) srci[j] = s->*rec_ints[j].member;
  for (int64_t c = 0; c < ncol; ++c) {
    const int64_t i = ipt[c];
    double *r = &cs[(size_t)c * MCKPP_CS];
    int *q = &ci[(size_t)c * MCKPP_CI];
    for (size_t j = 0; j < std::size(rec_doubles); ++j) r[rec_doubles[j].slot] = srcd[j] ? srcd[j][i] : rec_doubles[j].def;
    for (size_t j = 0; j < std::size(rec_ints); ++j) q[rec_ints[j].slot] = srci[j] ? srci[j][i] : rec_ints[j].def;
    if (q[CI_JERLOV] < 1 || q[CI_JERLOV] > 5) return fail("mckpp_hip_upload: jerlov(%lld)=%d outside 1..5", (long long)i + 1, q[CI_JERLOV]);
    q[CI_INITFLAG] = q[CI_INITFLAG] != 0;   // the LOGICALs: any non-zero word is .TRUE.
    q[CI_LOCEAN] = q[CI_LOCEAN] != 0;
    q[CI_IPT] = (int)i;
  }
  HIPCHK(hipMemcpyAsync(h->d_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_ci, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
  });
}

static int ensure_host_f(mckpp_hip_ctx *h, size_t elems)
{
  if (elems <= h->h_f.size()) return 0;
  HIPCHK(hipEventSynchronize(h->ev_f));   // the copy that last read the block
  HIPCHK(h->h_f.reserve(elems));
  return 0;
}

int mckpp_hip_set_forcing(mckpp_hip_handle h, const double *sflux)
{
  return entry(__func__, h, [&]() -> int {
  if (!sflux) return fail("mckpp_hip_set_forcing: null argument");
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  // sflux(:,1:6,5,0) is six contiguous (npts) slabs: up as they are (from the caller's array, pinned on first
  // use), compacted into the records' flux slots on the device.  The call returns when the slabs have been read -
  // the caller may rewrite its array - not when the records are updated (that is stream-ordered before the step).
  const size_t n6 = (size_t)h->npts * 6;
  const double *slabs = sflux + h->npts * (int64_t)h->c.nsflxs * 4;
  if (ensure_stage(h, n6)) return -1;
  pin_host(h, sflux, (size_t)h->npts * h->c.nsflxs * 5 * (size_t)(h->c.njdt + 1) * sizeof(double));
  HIPCHK(hipMemcpyAsync(h->d_stage, slabs, n6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->ev_f, h->stream));
  HIPCHK(mckpp_launch_unpack_sflux(h->d_stage, h->d_ipt, h->d_cs, h->ncol, h->npts, h->stream));
  HIPCHK(hipEventSynchronize(h->ev_f));
  return 0;
  });
}

// mckpp_fluxes (src/mckpp_fluxes_mod.F90:35-89) on the device: eight forcing fields (npts each, 3D
// ordering) -> sflux(:,1:6,5,0) of every resident l_ocean column, plus the ntflux refresh of wXNT(:,1).
int mckpp_hip_fluxes(mckpp_hip_handle h, int ntime, const double *taux, const double *tauy, const double *swf,
                     const double *lwf, const double *lhf, const double *shf, const double *rain,
                     const double *snow, int l_rest, double flsn, double el)
{
  return entry(__func__, h, [&]() -> int {
  if (!taux || !tauy || !swf || !lwf || !lhf || !shf || !rain || !snow)
    return fail("mckpp_hip_fluxes: null argument");
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  const double *src[8] = {taux, tauy, swf, lwf, lhf, shf, rain, snow};
  const size_t n8 = (size_t)8 * h->ncol;
  if (ensure_host_f(h, n8) || ensure_stage(h, n8)) return -1;
  HIPCHK(hipEventSynchronize(h->ev_f));
  for (int m = 0; m < 8; ++m)
    for (int64_t c = 0; c < h->ncol; ++c) h->h_f[(size_t)m * h->ncol + c] = src[m][h->ipt[c]];
  HIPCHK(hipMemcpyAsync(h->d_stage, h->h_f, n8 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->ev_f, h->stream));
  mckpp_kparams p;
  fill_params(h, p, ntime, MCKPP_MODE_STEP);
  HIPCHK(mckpp_launch_fluxes(p, ntime, h->d_stage, l_rest, flsn, el, h->stream));
  return 0;
  });
}

// default-physics contexts carry no correction rows until someone needs them
static int ensure_correction_rows(mckpp_hip_ctx *h)
{
  if (h->d_ext_out[O_TINC]) return 0;
  const size_t rowelems = (size_t)h->ncol * h->ld;
  dev_buf<double> rows[O_COUNT];   // all four or none
  for (auto &p : rows) { HIPCHK(p.alloc(rowelems)); HIPCHK(hipMemsetAsync(p, 0, rowelems * sizeof(double), h->stream)); }
  for (int o = 0; o < O_COUNT; ++o) h->d_ext_out[o] = std::move(rows[o]);
  return 0;
}

int mckpp_hip_bottomtemp(mckpp_hip_handle h, const double *bottom_temp)
{
  return entry(__func__, h, [&]() -> int {
  if (!bottom_temp) return fail("mckpp_hip_bottomtemp: null argument");
  if (h->d_bot_temp)
    return fail("mckpp_hip_bottomtemp: a bottom temperature is resident (mckpp_hip_set_bottomtemp) and every step launch "
                "already applies the override; a second one would zero tinc_fcorr and ocnTcorr of the bottom level - drop "
                "this call, or cancel the resident field with mckpp_hip_set_bottomtemp(NULL)");
  if (!h->anc[MCKPP_ANC_BOTTOM_TEMP].ep.empty())
    return fail("mckpp_hip_bottomtemp: the bottom temperature has a schedule (mckpp_hip_ancillary_schedule) and every step "
                "launch already applies the override; a second one would zero tinc_fcorr and ocnTcorr of the bottom level - "
                "drop this call, or cancel the schedule");
  if (h->ncol == 0) return 0;
  if (!h->diag) return fail("mckpp_hip_bottomtemp: needs the diagnostics on (rho, cp of the last vmix)");
  HIPCHK(hipSetDevice(h->device));
  if (ensure_correction_rows(h)) return -1;
  std::vector<double> bt((size_t)h->ncol);
  for (int64_t c = 0; c < h->ncol; ++c) bt[(size_t)c] = bottom_temp[h->ipt[c]];
  if (ensure_stage(h, bt.size())) return -1;
  HIPCHK(hipMemcpyAsync(h->d_stage, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  mckpp_kparams p;
  fill_params(h, p, 0, MCKPP_MODE_STEP);
  HIPCHK(mckpp_launch_bottomtemp(p, h->d_stage, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
  });
}

static int bt_cancel(mckpp_hip_ctx *h)
{
  if (!h->d_bot_temp) return 0;
  if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still read the field
  h->d_bot_temp.reset();
  return 0;
}

// The resident form of the override: from here on every MCKPP_MODE_STEP launch ends each column-step with it
// (k_column_ps, finish round).  Output, restart and step-log schedules are left alone.
int mckpp_hip_set_bottomtemp(mckpp_hip_handle h, const double *bottom_temp)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  HIPCHK(hipSetDevice(h->device));
  if (!bottom_temp) return bt_cancel(h);
  if (!h->anc[MCKPP_ANC_BOTTOM_TEMP].ep.empty())
    return fail("%s: the bottom temperature has a schedule (mckpp_hip_ancillary_schedule, MCKPP_ANC_BOTTOM_TEMP); the two "
                "are mutually exclusive - cancel the schedule first", who);
  if (h->npts <= 0) return fail("%s: upload the state first (the field is compacted to the resident columns)", who);
  if (h->ncol == 0) return 0;
  if (ensure_correction_rows(h)) return -1;
  std::vector<double> bt((size_t)h->ncol);
  for (int64_t c = 0; c < h->ncol; ++c) bt[(size_t)c] = bottom_temp[h->ipt[c]];
  dev_buf<double> first;   // a first field is built here and moved in once it is filled
  if (!h->d_bot_temp) HIPCHK(first.alloc(bt.size()));
  // on the launches' stream, behind those already queued (they keep the field they were launched with); the host
  // image is this call's own, so wait for the copy
  HIPCHK(hipMemcpyAsync(first ? first : h->d_bot_temp, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (first) h->d_bot_temp = std::move(first);
  return 0;
  });
}

// ---------------------------------------------------------------------------
// Ancillary record series: boundary updates inside the launches
// ---------------------------------------------------------------------------
static const char *const anc_names[MCKPP_ANC_COUNT] = {"SST0", "fcorr_twod", "fcorr_withz", "sfcorr_withz", "ocnT_clim",
                                                       "sal_clim", "bottom_temp"};
static_assert(MCKPP_ANC_COUNT == MCKPP_ANC_KINDS && (int)MCKPP_ANC_BOTTOM_TEMP == (int)ANC_BOTTOM_TEMP &&
              (int)MCKPP_ANC_OCNT_CLIM == (int)ANC_OCNT_CLIM, "the kinds of the header are those of the kernel");
static bool anc_is_3d(int kind) { return kind >= MCKPP_ANC_FCORR_WITHZ && kind <= MCKPP_ANC_SAL_CLIM; }
static size_t anc_stride(const mckpp_hip_ctx *h, int kind) { return anc_is_3d(kind) ? (size_t)h->ncol * h->ld : (size_t)h->ncol; }

static int anc_free_records(mckpp_hip_ctx *h, int kind)
{
  auto &a = h->anc[kind];
  if (a.d) {
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still read the records
    a.d.reset();
  }
  a.nrec = 0; a.rec0 = 0;
  return 0;
}

static int anc_cancel_all(mckpp_hip_ctx *h)
{
  for (int k = 0; k < MCKPP_ANC_COUNT; ++k) {
    if (anc_free_records(h, k)) return -1;
    h->anc[k].ep.clear();
  }
  return 0;
}

static int anc_check_kind(mckpp_hip_ctx *h, int kind, const char *who)
{
  if (kind < 0 || kind >= MCKPP_ANC_COUNT) return fail("%s: kind=%d (0..%d)", who, kind, MCKPP_ANC_COUNT - 1);
  if (kind != MCKPP_ANC_BOTTOM_TEMP && !h->ext)
    return fail("%s: %s on a context of the default physics: nothing there reads it (the switch that does is off: "
                "L_RELAX_SST / L_FCORR / L_FCORR_WITHZ / L_SFCORR_WITHZ / L_RELAX_OCNT / L_RELAX_SAL / L_NO_ISOTHERM / "
                "clim_present in mckpp_const_c)", who, anc_names[kind]);
  return 0;
}

int mckpp_hip_set_ancillary_series(mckpp_hip_handle h, int kind, int rec0, int nrec, const double *records)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (anc_check_kind(h, kind, who)) return -1;
  if (nrec < 0 || rec0 < 0 || (nrec > 0 && !records))
    return fail("%s: %s rec0=%d nrec=%d records=%s", who, anc_names[kind], rec0, nrec, records ? "set" : "NULL");
  if (nrec > 0 && h->npts <= 0) return fail("%s: upload the state first (the records are compacted to the resident columns)", who);
  HIPCHK(hipSetDevice(h->device));
  if (anc_free_records(h, kind)) return -1;
  if (nrec == 0) return 0;
  auto &a = h->anc[kind];
  dev_buf<double> d;   // built here, moved in once every record is there
  if (h->ncol > 0) {
    const size_t stride = anc_stride(h, kind), n = stride * (size_t)nrec;
    HIPCHK(d.alloc(n));
    if (anc_is_3d(kind)) {   // rows, by the path of upload / update_ancillaries
      const size_t slab = (size_t)h->npts * h->nzp1;
      HIPCHK(hipMemsetAsync(d, 0, n * sizeof(double), h->stream));
      for (int r = 0; r < nrec; ++r)
        if (up_rows(h, records + (size_t)r * slab, h->nzp1, d + (size_t)r * stride, 0, records, slab * (size_t)nrec)) return -1;
      if (xfer_finish(h)) return -1;   // the caller's array is its own again
    } else {
      std::vector<double> f(n);
      for (int r = 0; r < nrec; ++r)
        for (int64_t c = 0; c < h->ncol; ++c) f[(size_t)r * stride + (size_t)c] = records[(size_t)r * (size_t)h->npts + h->ipt[c]];
      // on the launches' stream, behind those already queued; the host image is this call's own, so wait for the copy
      HIPCHK(hipMemcpyAsync(d, f.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
  }
  a.d = std::move(d);
  a.rec0 = rec0;
  a.nrec = nrec;
  return 0;
  });
}

int mckpp_hip_ancillary_schedule(mckpp_hip_handle h, int kind, int nt_origin, int cadence, int epoch0, int nepochs,
                                 const mckpp_anc_epoch_c *epochs)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (anc_check_kind(h, kind, who)) return -1;
  if (nepochs < 0) return fail("%s: %s nepochs=%d", who, anc_names[kind], nepochs);
  if (nepochs == 0) { h->anc[kind].ep.clear(); return 0; }
  if (!epochs || cadence < 1 || epoch0 < 0 || nt_origin < 0)
    return fail("%s: %s nt_origin=%d cadence=%d epoch0=%d epochs=%s", who, anc_names[kind], nt_origin, cadence, epoch0,
                epochs ? "set" : "NULL");
  const bool interp_ok = kind == MCKPP_ANC_OCNT_CLIM || kind == MCKPP_ANC_SAL_CLIM;
  for (int i = 0; i < nepochs; ++i) {
    if (epochs[i].rec_prev < 0) return fail("%s: %s epoch %d: rec_prev=%d", who, anc_names[kind], epoch0 + i, epochs[i].rec_prev);
    if (epochs[i].rec_next >= 0 && !interp_ok)
      return fail("%s: %s epoch %d is interpolated (rec_next=%d): the reference interpolates ocnT_clim and sal_clim only "
                  "(L_INTERP_OCNT, L_INTERP_SAL)", who, anc_names[kind], epoch0 + i, epochs[i].rec_next);
  }
  if (kind == MCKPP_ANC_BOTTOM_TEMP) {
    if (h->d_bot_temp)
      return fail("%s: a bottom temperature is resident (mckpp_hip_set_bottomtemp); the two are mutually exclusive - cancel "
                  "it with mckpp_hip_set_bottomtemp(NULL) first", who);
    if (h->npts <= 0) return fail("%s: upload the state first", who);
    HIPCHK(hipSetDevice(h->device));
    if (h->ncol > 0 && ensure_correction_rows(h)) return -1;
  }
  auto &a = h->anc[kind];
  a.origin = nt_origin; a.cadence = cadence; a.epoch0 = epoch0;
  a.ep.assign(epochs, epochs + nepochs);
  return 0;
  });
}

// A step launch call under ancillary schedules: every step's selection of every scheduled kind, checked - nothing is
// launched for a step before the origin, an epoch outside the table or a record that is not resident - and then written
// behind the launches already queued, ahead of this call's own.
static int anc_prepare(mckpp_hip_ctx *h, int nt0, int nsteps, const char *who)
{
  h->anc_mask = 0;
  h->anc_nt0 = nt0;
  int mask = 0;
  for (int k = 0; k < MCKPP_ANC_COUNT; ++k) if (!h->anc[k].ep.empty()) mask |= 1 << k;
  if (!mask) return 0;
  if ((mask >> MCKPP_ANC_BOTTOM_TEMP & 1) && !h->diag)
    return fail("%s: the bottom temperature has a schedule (mckpp_hip_ancillary_schedule) and the diagnostics are switched "
                "off (mckpp_hip_set_diagnostics): the override needs rho and cp of the last vmix, which are diagnostics", who);
  const size_t n = (size_t)nsteps * MCKPP_ANC_KINDS;
  std::vector<mckpp_anc_sel> sel(n, mckpp_anc_sel{0, -1, 0.0, 0.0});
  for (int k = 0; k < MCKPP_ANC_COUNT; ++k) {
    if (!(mask >> k & 1)) continue;
    const auto &a = h->anc[k];
    const long long stride = (long long)anc_stride(h, k);
    auto resident = [&](int rec) { return rec >= a.rec0 && rec < a.rec0 + a.nrec; };
    for (int i = 0; i < nsteps; ++i) {
      const int nt = nt0 + i;
      if (nt < a.origin) return fail("%s: %s: step %d lies before the schedule's origin %d", who, anc_names[k], nt, a.origin);
      const int e = (nt - a.origin) / a.cadence;
      if (e < a.epoch0 || e >= a.epoch0 + (int)a.ep.size())
        return fail("%s: %s: step %d is in epoch %d, the table holds epochs %d..%d", who, anc_names[k], nt, e, a.epoch0,
                    a.epoch0 + (int)a.ep.size() - 1);
      const mckpp_anc_epoch_c &ep = a.ep[(size_t)(e - a.epoch0)];
      for (const int rec : {ep.rec_prev, ep.rec_next}) {
        if (rec < 0 || resident(rec)) continue;
        if (a.nrec == 0) return fail("%s: %s: step %d (epoch %d) needs record %d, none is resident", who, anc_names[k], nt, e, rec);
        return fail("%s: %s: step %d (epoch %d) needs record %d, resident are %d..%d", who, anc_names[k], nt, e, rec, a.rec0,
                    a.rec0 + a.nrec - 1);
      }
      mckpp_anc_sel &q = sel[(size_t)i * MCKPP_ANC_KINDS + k];
      q.off_prev = (ep.rec_prev - a.rec0) * stride;
      q.off_next = ep.rec_next < 0 ? -1 : (ep.rec_next - a.rec0) * stride;
      q.w_prev = ep.w_prev; q.w_next = ep.w_next;
    }
  }
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (n > h->d_anc_sel.size()) {
    if (h->d_anc_sel) HIPCHK(hipStreamSynchronize(h->stream));   // a launch in flight may still read the table
    HIPCHK(h->d_anc_sel.reserve(n));
  }
  mckpp_anc_sel *img = nullptr;
  HIPCHK(h->h_anc_sel.take(n, &img));   // (waits for the copy that last read this host image)
  memcpy(img, sel.data(), n * sizeof(mckpp_anc_sel));
  HIPCHK(hipMemcpyAsync(h->d_anc_sel, img, n * sizeof(mckpp_anc_sel), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h->h_anc_sel.queued(h->stream));
  h->anc_mask = mask;
  return 0;
}

// mckpp_boundary_interpolate_temp / _sal, boundary_interpolate.F90:25-35 and :49-50 (:80-90, :104-105): true_time,
// prev_time and next_time are INTEGER there, so each REAL assigned to them is truncated toward zero.
void mckpp_host_interp_weights(double time, int32_t ndtupd, double dto, double spd, int32_t period, int32_t *prev_time,
                               int32_t *next_time, double *w_prev, double *w_next)
{
  const int32_t true_time = (int32_t)time;                                                          // :25
  const double ndays = ndtupd * dto / spd;                                                          // :26
  int32_t prev = (int32_t)(std::floor((true_time + ndays / 2) / ndays) * ndays - ndays * 0.5);      // :29
  double wp;
  if (prev < 0) {
    wp = (ndays - std::abs(true_time - prev)) / ndays;                                              // :31
    prev = prev + period;                                                                           // :32
  } else {
    wp = (ndays - (true_time - prev)) / ndays;                                                      // :34
  }
  if (prev_time) *prev_time = prev;
  if (next_time) *next_time = (int32_t)(prev + ndays);                                              // :49
  if (w_prev) *w_prev = wp;
  if (w_next) *w_next = 1 - wp;                                                                     // :50
}

// the caller's arrays pinned on behalf of this context go back to pageable memory (before the caller frees them)
int mckpp_hip_release_host_arrays(mckpp_hip_handle h)
{
  return entry(__func__, h, [&]() -> int {
  HIPCHK(hipSetDevice(h->device));
  if (xfer_finish(h)) return -1;
  unpin_all(h);
  return 0;
  });
}

int mckpp_hip_set_diagnostics(mckpp_hip_handle h, int on)
{
  return entry(__func__, h, [&]() -> int {
  h->diag = on ? 1 : 0;
  return 0;
  });
}

int mckpp_hip_set_solver_mode(mckpp_hip_handle h, int mode)
{
  return entry(__func__, h, [&]() -> int {
  if (mode < 0 || mode > 1) return fail("mckpp_hip_set_solver_mode: unknown solver mode (0: the reference's order, 1: two-ended)");
  h->solver_mode = mode;
  return 0;
  });
}

int mckpp_hip_get_solver_mode(mckpp_hip_handle h) { return entry(__func__, h, [&]() -> int { return h->solver_mode; }); }

// output fields that are diagnostics of the last vmix (or correction rows): need mckpp_hip_set_diagnostics on
static bool win_is_diag(int f) { return f >= MCKPP_OUT_B && f <= MCKPP_OUT_SINC_FCORR; }

static void fill_params(mckpp_hip_ctx *h, mckpp_kparams &p, int ntime, int mode)
{
  memset(&p, 0, sizeof p);
  p.nz = h->nz; p.nzp1 = h->nzp1; p.ncol = (int)h->ncol; p.ld = h->ld;
  p.ntime = ntime; p.itermax = h->c.itermax; p.mode = mode; p.diag = h->diag;
  p.L_SSref = h->c.L_SSref; p.LDD = h->c.LDD; p.clim_present = h->c.clim_present;
  p.l2pre = h->l2pre; p.LRI = h->c.LRI ? 1 : 0; p.l3cap = h->l3cap;
  p.first_margin = h->first_guess ? h->first_margin : -1; p.scan_rule = h->guess_margin | (h->first_guess ? 1 << 16 : 0);
  p.solver_mode = h->solver_mode;
  p.hmixtolfrac = h->c.hmixtolfrac; p.dto = h->c.dto; p.grav = h->c.grav; p.vonk = h->c.vonk; p.sice = h->c.sice;
  p.Vtc = h->Vtc; p.cg = h->cg; p.dm_nz = h->dm_nz;
  p.zm = h->d_zm; p.hm = h->d_hm; p.tri0 = h->d_tri0; p.tri1 = h->d_tri1;
  p.swfrac_tab = h->d_swfrac_tab; p.swdk_tab = h->d_swdk_tab; p.ldc = h->ldc; p.wtab = reinterpret_cast<const double *>(h->d_wtab.get());
  p.U = h->d_prof[P_U]; p.V = h->d_prof[P_V]; p.T = h->d_prof[P_T]; p.S = h->d_prof[P_S];
  p.Us[0] = h->d_prof[P_US0]; p.Us[1] = h->d_prof[P_US1]; p.Vs[0] = h->d_prof[P_VS0]; p.Vs[1] = h->d_prof[P_VS1];
  p.Ts[0] = h->d_prof[P_TS0]; p.Ts[1] = h->d_prof[P_TS1]; p.Ss[0] = h->d_prof[P_SS0]; p.Ss[1] = h->d_prof[P_SS1];
  p.U_init = h->d_prof[P_UINIT]; p.V_init = h->d_prof[P_VINIT];
  p.cs = h->d_cs; p.ci = h->d_ci; p.qhead = h->d_qhead; p.dbg = h->d_dbg;
  p.nsteps_launch = 1; p.done = h->d_done; p.nqueues = h->nqueues; p.qowner = h->d_qhead + 16;
  p.sync = h->d_qhead + 32; p.solo_after = h->solo_after; p.solo_limit = h->solo_limit; p.view_kmax = h->view_kmax;
  for (int i = 0; i < 16; ++i) p.xcc_queue[i] = h->xcc_queue[i];
  p.ext = h->ext_kernel ? 1 : 0;
  p.L_RELAX_SST = h->c.L_RELAX_SST; p.L_RELAX_CALCONLY = h->c.L_RELAX_CALCONLY; p.L_FCORR = h->c.L_FCORR;
  p.L_FCORR_WITHZ = h->c.L_FCORR_WITHZ; p.L_SFCORR = h->c.L_SFCORR; p.L_SFCORR_WITHZ = h->c.L_SFCORR_WITHZ;
  p.L_RELAX_SAL = h->c.L_RELAX_SAL; p.L_RELAX_OCNT = h->c.L_RELAX_OCNT; p.L_NO_FREEZE = h->c.L_NO_FREEZE;
  p.L_NO_ISOTHERM = h->c.L_NO_ISOTHERM; p.L_DAMP_CURR = h->c.L_DAMP_CURR; p.iso_bot = h->c.iso_bot;
  p.dt_uvdamp = h->c.dt_uvdamp; p.maxmodeadv = h->c.maxmodeadv; p.iso_thresh = h->c.iso_thresh;
  p.dm = h->d_dm; p.hsum = h->d_hsum; p.xs = h->d_xs; p.adv_i = h->d_adv_i; p.adv_d = h->d_adv_d;
  p.fcorr_withz = h->d_ext_in[E_FCORR_WITHZ]; p.sfcorr_withz = h->d_ext_in[E_SFCORR_WITHZ];
  p.ocnT_clim = h->d_ext_in[E_OCNT_CLIM]; p.sal_clim = h->d_ext_in[E_SAL_CLIM];
  p.tinc_fcorr = h->d_ext_out[O_TINC]; p.sinc_fcorr = h->d_ext_out[O_SINC];
  p.ocnTcorr = h->d_ext_out[O_OCNTCORR]; p.scorr = h->d_ext_out[O_SCORR];
  p.rho = h->d_diag[D_RHO]; p.cp = h->d_diag[D_CP]; p.buoy = h->d_diag[D_BUOY];
  p.talpha = h->d_diag[D_TALPHA]; p.sbeta = h->d_diag[D_SBETA];
  p.difm = h->d_diag[D_DIFM]; p.difs = h->d_diag[D_DIFS]; p.dift = h->d_diag[D_DIFT]; p.ghat = h->d_diag[D_GHAT];
  p.wU1 = h->d_diag[D_WU1]; p.wU2 = h->d_diag[D_WU2];
  p.wX1 = h->d_diag[D_WX1]; p.wX2 = h->d_diag[D_WX2]; p.wX3 = h->d_diag[D_WX3]; p.wXNT1 = h->d_diag[D_WXNT1];
  p.Rig = h->d_diag[D_RIG]; p.dbloc = h->d_diag[D_DBLOC]; p.Shsq = h->d_diag[D_SHSQ];
  p.scratch = h->d_scratch; p.scratch_doubles = h->scratch_doubles;
  if (mode == MCKPP_MODE_STEP && h->nwin > 0) { p.win = h->d_win; p.nwin = h->nwin; }   // (init / vmix never accumulate)
  if (mode == MCKPP_MODE_STEP && h->rs.period > 0 && h->rs.rows) {   // (... and never take a snapshot)
    p.snap_rows = h->rs.rows; p.snap_cs = h->rs.cs; p.snap_ci = h->rs.ci;
    p.snap_plane = (long long)h->ncol * h->ld; p.snap_slot = MCKPP_SNAP_ROWS * p.snap_plane;
    p.snap_origin = (int)h->rs.origin; p.snap_period = (int)h->rs.period; p.snap_nslots = h->rs.nslots;
  }
  if (mode == MCKPP_MODE_STEP && h->slog.cap > 0) {   // (... and never log)
    p.log_rec = h->slog.rec; p.log_ctl = h->slog.ctl;
    p.log_cap = (int)h->slog.cap; p.log_min_passes = h->slog.min_passes;
  }
  if (mode == MCKPP_MODE_STEP) p.bot_temp = h->d_bot_temp;   // (init / vmix / pass never apply the override)
  if (mode == MCKPP_MODE_STEP && h->anc_mask) {   // (... and never read a series; anc_prepare of this launch call)
    p.anc_sel = h->d_anc_sel; p.anc_mask = h->anc_mask; p.anc_nt0 = h->anc_nt0;
    for (int k = 0; k < MCKPP_ANC_KINDS; ++k) p.anc_rec[k] = h->anc[k].d;
  }
  // Which steps of a launch store their diagnostics: every one if something inside the launch reads them - a window
  // folds every step of its period, the bottom-temperature override takes rho and cp of each step's last vmix - or if
  // MCKPP_LEAN_DIAG=0 says so (read at every launch: A/B runs, tests); otherwise the kernel keeps them for the
  // launch's last step and the snapshot steps, the only ones anything can see (k_column_ps, M0).
  p.diag_every = h->diag ? 1 : 0;
  if (mode == MCKPP_MODE_STEP && h->diag) {
    const char *e = getenv("MCKPP_LEAN_DIAG");
    bool every = e && atoi(e) == 0;
    every = every || h->d_bot_temp || (h->anc_mask >> MCKPP_ANC_BOTTOM_TEMP & 1);
    if (h->nwin > 0)
      for (const auto &w : h->wsched)
        for (int f : w.fields) every = every || win_is_diag(f);
    p.diag_every = every ? 1 : 0;
  }
}

// the records a forced run reads: the linear series from record rec0 on, or (nring > 0) the ring's slots
struct forced_run { int ndtocn, l_rest; double flsn, el; const double *series; int rec0, nring; };

static int win_check_launch(mckpp_hip_ctx *h, int nt0, int nsteps, const char *who);
static void win_advance(mckpp_hip_ctx *h, int nt0, int nsteps);
static int exp_advance(mckpp_hip_ctx *h, int nt0);
static int snap_check_launch(mckpp_hip_ctx *h, int nt0, int nsteps, const char *who);
static int snap_advance(mckpp_hip_ctx *h, int nt0, int nsteps);
static int run_launch(mckpp_hip_ctx *h, int ntime, int nsteps, int mode, const forced_run *forced);

// A step launch under output schedules and the restart schedule: checked against them before anything is launched,
// then the schedules know which steps have run (and so which of their records and snapshots are complete)
static int run(mckpp_hip_ctx *h, const char *who, int ntime, int nsteps, int mode, const forced_run *forced = nullptr)
{
  const bool sched = mode == MCKPP_MODE_STEP && nsteps > 0;
  if (sched && h->d_bot_temp && !h->diag)
    return fail("%s: a bottom temperature is resident (mckpp_hip_set_bottomtemp) and the diagnostics are switched off "
                "(mckpp_hip_set_diagnostics): the override needs rho and cp of the last vmix, which are diagnostics", who);
  if (sched && (win_check_launch(h, ntime, nsteps, who) || snap_check_launch(h, ntime, nsteps, who))) return -1;
  if (sched && anc_prepare(h, ntime, nsteps, who)) return -1;
  if (run_launch(h, ntime, nsteps, mode, forced)) return -1;
  if (sched) win_advance(h, ntime, nsteps);
  if (sched && exp_advance(h, ntime)) return -1;
  if (sched && snap_advance(h, ntime, nsteps)) return -1;
  return 0;
}

static int run_launch(mckpp_hip_ctx *h, int ntime, int nsteps, int mode, const forced_run *forced)
{
  if (h->ncol == 0) { h->nlaunch = 0; h->timed = false; return 0; }
  if (h->ext && !h->ext_inputs_resident)
    return fail("optional-physics context: the relaxation / correction / advection inputs are not resident "
                "(after mckpp_hip_load_restart call mckpp_hip_update_ancillaries before stepping)");
  HIPCHK(hipSetDevice(h->device));
  {   // parameter block (identical for every launch of this call but ntime), from a pinned slot: no host wait
    mckpp_kparams *q = nullptr;
    HIPCHK(h->h_params.take(1, &q));
    fill_params(h, *q, ntime, mode);
    HIPCHK(hipMemcpyAsync(h->d_params, q, sizeof(mckpp_kparams), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h->h_params.queued(h->stream));
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  // Several steps of constant forcing (mckpp_hip_step with nsteps > 1): ONE launch takes every column through all of
  // them - ncol x nsteps tickets, a column's step waiting only for that column's previous step (k_column_ps, M0) -
  // instead of a launch per step, each of which would wait for its slowest column.  Same results bit for bit (the
  // columns are independent; every step stores its outputs, and its diagnostics if anything can read them before the
  // column's next step overwrites them - fill_params, diag_every).  The forced run too: a step
  // that is a flux update assembles its column's forcing from the resident record itself.  Not for a step at ntime = 0.
  if (mode == MCKPP_MODE_STEP && nsteps > 1 && ntime >= 1 && h->multistep) {
    if (!h->d_done) HIPCHK(h->d_done.alloc(2 * (size_t)h->ncol));   // done[ncol], then the steps started (k_column_ps, M0)
    const int per_launch = (int)std::max<int64_t>(1, ((int64_t)1 << 30) / h->ncol);   // tickets are 32-bit (per queue: fewer still)
    for (int i = 0; i < nsteps; i += per_launch) {
      const int n = nsteps - i < per_launch ? nsteps - i : per_launch;
      mckpp_kparams *qp = nullptr;   // this launch's parameter block (its step count differs from the call's first)
      HIPCHK(h->h_params.take(1, &qp));
      mckpp_kparams &q = *qp;
      fill_params(h, q, ntime + i, mode);
      q.nsteps_launch = n;
      if (forced) {   // the forced run: every step finds its flux record itself (k_column_ps, M0)
        q.series = forced->series; q.series_rec0 = forced->rec0; q.series_nring = forced->nring;
        q.ndtocn = forced->ndtocn; q.l_rest = forced->l_rest;
        q.flsn = forced->flsn; q.el = forced->el;
      }
      HIPCHK(hipMemcpyAsync(h->d_params, qp, sizeof(mckpp_kparams), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h->h_params.queued(h->stream));
      HIPCHK(hipMemsetAsync(h->d_qhead, 0, QBLOCK_INTS * sizeof(int), h->stream));
      HIPCHK(hipMemsetAsync(h->d_done, 0, 2 * (size_t)h->ncol * sizeof(int), h->stream));
      HIPCHK(mckpp_launch_column_kernel_ps(q, h->d_params, h->num_cu, h->stream, &h->last_launch));
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->nlaunch = nsteps;   // (mckpp_hip_last_kernel_ms: time per STEP, whatever the number of launches)
    h->nkernels = (nsteps + per_launch - 1) / per_launch;
    h->timed = true;
    return 0;
  }
  for (int i = 0; i < nsteps; ++i) {
    mckpp_kparams p;
    fill_params(h, p, ntime + i, mode);
    if (forced && (ntime + i - 1) % forced->ndtocn == 0) {   // ocean_model_3D.F90:44-48
      const int upd = (ntime + i - 1) / forced->ndtocn;
      const int rec = forced->nring > 0 ? upd % forced->nring : upd - forced->rec0;   // the ring's slot | the series' index
      HIPCHK(mckpp_launch_fluxes(p, ntime + i, forced->series + (size_t)rec * 8 * (size_t)h->ncol, forced->l_rest,
                                 forced->flsn, forced->el, h->stream));
    }
    HIPCHK(hipMemsetAsync(h->d_qhead, 0, QBLOCK_INTS * sizeof(int), h->stream));
    HIPCHK(mckpp_launch_column_kernel_ps(p, h->d_params, h->num_cu, h->stream, &h->last_launch));
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  h->nlaunch = nsteps;
  h->nkernels = nsteps;
  h->timed = true;
  return 0;
}

static int run_one(const char *who, mckpp_hip_ctx *h, int ntime, int mode)
{
  return entry(who, h, [&]() -> int { return run(h, who, ntime, 1, mode); });
}
int mckpp_hip_init_ocean(mckpp_hip_handle h, int ntime) { return run_one(__func__, h, ntime, MCKPP_MODE_INIT); }
int mckpp_hip_step(mckpp_hip_handle h, int ntime, int nsteps)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (nsteps < 0) return fail("mckpp_hip_step: nsteps=%d", nsteps);
  return run(h, who, ntime, nsteps, MCKPP_MODE_STEP);
  });
}
int mckpp_hip_vmix_pass(mckpp_hip_handle h, int ntime) { return run_one(__func__, h, ntime, MCKPP_MODE_PASS); }
int mckpp_hip_vmix_only(mckpp_hip_handle h, int ntime) { return run_one(__func__, h, ntime, MCKPP_MODE_VMIX); }

int mckpp_hip_set_flux_series(mckpp_hip_handle h, int rec0, int nrec, const double *fields)
{
  return entry(__func__, h, [&]() -> int {
  if (!fields) return fail("mckpp_hip_set_flux_series: null argument");
  if (nrec < 1 || rec0 < 0) return fail("mckpp_hip_set_flux_series: rec0=%d nrec=%d", rec0, nrec);
  if (h->npts <= 0) return fail("mckpp_hip_set_flux_series: upload the state first (the records are compacted to the resident columns)");
  if (h->ring.nslots > 0)
    return fail("mckpp_hip_set_flux_series: a flux ring of %d slots is set (mckpp_hip_flux_ring); the two are mutually "
                "exclusive - cancel the ring first (mckpp_hip_flux_ring with 0 slots)", h->ring.nslots);
  HIPCHK(hipSetDevice(h->device));
  h->d_series.reset();
  h->series_rec0 = rec0;
  h->series_nrec = nrec;
  if (h->ncol == 0) return 0;
  const size_t n = (size_t)nrec * 8 * (size_t)h->ncol;
  std::vector<double> f(n);
  for (int r = 0; r < nrec; ++r)
    for (int m = 0; m < 8; ++m) {
      const double *src = fields + ((size_t)r * 8 + m) * (size_t)h->npts;
      double *dst = f.data() + ((size_t)r * 8 + m) * (size_t)h->ncol;
      for (int64_t c = 0; c < h->ncol; ++c) dst[c] = src[h->ipt[c]];
    }
  HIPCHK(h->d_series.alloc(n));
  HIPCHK(hipMemcpy(h->d_series, f.data(), n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
  });
}

// ---------------------------------------------------------------------------
// The flux-record ring: forcing streamed in while earlier launches run
// ---------------------------------------------------------------------------
// the records the ring holds (-1, -1: none)
static void ring_range(const mckpp_hip_ctx::flux_ring &g, int *first, int *last)
{
  *first = *last = -1;
  if (g.nslots == 0 || g.next_put < 0) return;
  *last = g.next_put - 1;
  *first = std::max(g.first_put, g.next_put - g.nslots);
}

static int ring_cancel(mckpp_hip_ctx *h)
{
  if (h->ring.nslots == 0) return 0;
  if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));             // no launch in flight may still read the slots
  if (h->flux_stream) HIPCHK(hipStreamSynchronize(h->flux_stream));   // no copy in flight may still write them, or read the staging
  h->ring = mckpp_hip_ctx::flux_ring{};
  return 0;
}

int mckpp_hip_flux_ring(mckpp_hip_handle h, int nslots)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (nslots < 0) return fail("%s: nslots=%d (0 cancels the ring)", who, nslots);
  if (nslots > 0 && h->npts <= 0) return fail("%s: upload the state first (the slots are sized to the resident columns)", who);
  HIPCHK(hipSetDevice(h->device));
  if (ring_cancel(h)) return -1;
  if (nslots == 0) return 0;
  mckpp_hip_ctx::flux_ring g;   // built here, moved in when all of it is there
  if (h->ncol > 0) {
    if (!h->flux_stream) HIPCHK(h->flux_stream.create());
    const size_t rec = 8 * (size_t)h->ncol;
    g.arrived.resize((size_t)nslots);
    g.last_read.resize((size_t)nslots);
    hipError_t e = g.slots.alloc((size_t)nslots * rec);
    for (int i = 0; i < nslots && e == hipSuccess; ++i) {
      e = g.arrived[(size_t)i].create();
      if (e == hipSuccess) e = g.last_read[(size_t)i].create();
    }
    if (e == hipSuccess) e = g.stage.prepare(rec);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail("%s: cannot allocate the %d slots of %zu bytes each (%s); no ring is set", who, nslots, rec * sizeof(double),
                  hipGetErrorString(e));
    }
  }
  g.nslots = nslots;
  if (h->d_series) {   // the ring takes the series' place
    HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still read its records
    h->d_series.reset();
  }
  h->series_nrec = 0;
  h->ring = std::move(g);
  return 0;
  });
}

// what a put - from host or from device arrays - needs before it queues anything: a state, a ring, the next record
static int ring_put_check(mckpp_hip_ctx *h, const char *who, int rec)
{
  if (h->npts <= 0) return fail("%s: upload the state and set a ring first (mckpp_hip_flux_ring)", who);
  const auto &g = h->ring;
  if (g.nslots == 0) return fail("%s: no flux ring is set (mckpp_hip_flux_ring)", who);
  if (g.next_put < 0 ? rec < 0 : rec != g.next_put)
    return fail("%s: record %d, but the records arrive in order: %s%d", who, rec,
                g.next_put < 0 ? "the first one is any record >= " : "the next one is record ", g.next_put < 0 ? 0 : g.next_put);
  return 0;
}

// ... and its bookkeeping, once the record's arrival is queued
static void ring_put_done(mckpp_hip_ctx::flux_ring &g, int rec)
{
  if (g.next_put < 0) g.first_put = rec;
  g.next_put = rec + 1;
}

int mckpp_hip_flux_ring_put(mckpp_hip_handle h, int rec, const double *fields)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!fields) return fail("%s: null argument", who);
  if (ring_put_check(h, who, rec)) return -1;
  auto &g = h->ring;
  if (h->ncol > 0) {
    HIPCHK(hipSetDevice(h->device));
    const size_t ncol = (size_t)h->ncol, npts = (size_t)h->npts;
    const int slot = rec % g.nslots;
    double *st = nullptr;
    HIPCHK(g.stage.take(8 * ncol, &st));   // (the only host wait: for the copy of two puts back, if still in flight)
    const int *ipt = h->ipt.data();
    for_columns(h->ncol, [=](int64_t a, int64_t b) {
      for (int m = 0; m < 8; ++m) {
        const double *src = fields + (size_t)m * npts;
        double *dst = st + (size_t)m * ncol;
        for (int64_t c = a; c < b; ++c) dst[c] = src[ipt[c]];
      }
    });
    // behind the launches of the last call that needed the record the slot held - on the device, never on the host
    HIPCHK(hipStreamWaitEvent(h->flux_stream, g.last_read[(size_t)slot], 0));
    HIPCHK(hipMemcpyAsync(g.slots + (size_t)slot * 8 * ncol, st, 8 * ncol * sizeof(double), hipMemcpyHostToDevice, h->flux_stream));
    HIPCHK(g.stage.queued(h->flux_stream));
    HIPCHK(hipEventRecord(g.arrived[(size_t)slot], h->flux_stream));
  }
  ring_put_done(g, rec);
  return 0;
  });
}

int mckpp_hip_flux_ring_records(mckpp_hip_handle h, int *first, int *last)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (h->ring.nslots == 0) return fail("%s: no flux ring is set (mckpp_hip_flux_ring)", who);
  int a, b;
  ring_range(h->ring, &a, &b);
  if (first) *first = a;
  if (last) *last = b;
  return 0;
  });
}

int mckpp_hip_run_forced(mckpp_hip_handle h, int nt_first, int nsteps, int ndtocn, int l_rest, double flsn, double el)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (nt_first < 1 || nsteps < 0 || ndtocn < 1)
    return fail("mckpp_hip_run_forced: nt_first=%d nsteps=%d ndtocn=%d", nt_first, nsteps, ndtocn);
  if (nsteps == 0) return 0;
  // every flux update of the span must be resident before anything is launched
  const int first_upd = (nt_first - 1 + ndtocn - 1) / ndtocn, last_upd = (nt_first + nsteps - 2) / ndtocn;
  auto &g = h->ring;
  if (g.nslots > 0) {
    int a, b;
    ring_range(g, &a, &b);
    if (first_upd <= last_upd && (b < 0 || first_upd < a || last_upd > b))
      return fail("mckpp_hip_run_forced: steps %d..%d need flux records %d..%d, the ring of %d slots holds %d..%d", nt_first,
                  nt_first + nsteps - 1, first_upd, last_upd, g.nslots, a, b);
  } else if (first_upd <= last_upd &&
      (h->series_nrec == 0 || first_upd < h->series_rec0 || last_upd >= h->series_rec0 + h->series_nrec))
    return fail("mckpp_hip_run_forced: steps %d..%d need flux records %d..%d, resident are %d..%d", nt_first,
                nt_first + nsteps - 1, first_upd, last_upd, h->series_rec0, h->series_rec0 + h->series_nrec - 1);
  if (g.nslots == 0) {
    const forced_run fr{ndtocn, l_rest, flsn, el, h->d_series, h->series_rec0, 0};
    return run(h, who, nt_first, nsteps, MCKPP_MODE_STEP, &fr);
  }
  // the ring: the launches wait, on the device, for the copies of the records they need; behind them the slots are
  // marked as read, which is what the next copy into each waits for
  const bool live = h->ncol > 0;
  if (live) HIPCHK(hipSetDevice(h->device));
  for (int r = first_upd; live && r <= last_upd; ++r) HIPCHK(hipStreamWaitEvent(h->stream, g.arrived[(size_t)(r % g.nslots)], 0));
  const forced_run fr{ndtocn, l_rest, flsn, el, g.slots, 0, g.nslots};
  const int rc = run(h, who, nt_first, nsteps, MCKPP_MODE_STEP, &fr);
  // (also after a failure: some of the call's launches may be queued)
  for (int r = first_upd; live && r <= last_upd; ++r) {
    const hipError_t e = hipEventRecord(g.last_read[(size_t)(r % g.nslots)], h->stream);
    if (e != hipSuccess && rc == 0) HIPCHK(e);
  }
  return rc;
  });
}

int mckpp_hip_synchronize(mckpp_hip_handle h)
{
  return entry(__func__, h, [&]() -> int {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  // (the contract of mckpp_hip_device.h: after this call the caller's device arrays are its own again - also those of a
  // put from device arrays that no launch has waited for yet)
  if (h->ev_read_flux) HIPCHK(hipEventSynchronize(h->ev_read_flux));
  if (getenv("MCKPP_LIST_DEBUG") && h->d_qhead) {   // after the last launch: the queues' heads, and (stamp builds) the stragglers' passes
    int qb[QBLOCK_INTS];
    HIPCHK(hipMemcpy(qb, h->d_qhead, sizeof qb, hipMemcpyDeviceToHost));
    fprintf(stderr, "[mckpp queues] stragglers left %d; (stamp builds: straggler passes in a view %d, beside others %d; workgroup passes with one %d | %d, their active slots %d | %d); heads",
            qb[32], qb[33], qb[34], qb[35], qb[36], qb[37], qb[38]);
    for (int q = 0; q < h->nqueues; ++q) fprintf(stderr, " %d", qb[q]);
    fprintf(stderr, "\n");
  }
  if (h->d_dbg) {   // MCKPP_STAMP=1: print and reset the per-segment cycle sums of the stamping wave of every workgroup
    unsigned long long t[40];
    HIPCHK(hipMemcpy(t, h->d_dbg, sizeof t, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->d_dbg, 0, sizeof t));
    if (t[31]) {
      const char *nm[23] = {"L1", "w", "M1L2", "w", "L3", "w", "M2", "w", "L4", "w", "M3", "w", "L5", "w", "L6", "w",
                            "M4back", "w", "L7", "w", "M5back", "w", "finish"};
      fprintf(stderr, "[mckpp stamps ps] wave-passes %llu; cycles per wave-pass:", t[31]);
      double tot = 0;
      for (int i = 0; i < 23; ++i) {
        if (i == 16 || i == 20) {   // the forward parts of the two sweeps have their own accumulators
          fprintf(stderr, " %s=%.0f", i == 16 ? "M4fwd" : "M5fwd", (double)t[i == 16 ? 24 : 25] / (double)t[31]);
          tot += (double)t[i == 16 ? 24 : 25];
        }
        fprintf(stderr, " %s=%.0f", nm[i], (double)t[i] / (double)t[31]);
        tot += (double)t[i];
      }
      {   // the finish round in parts (its own accumulators; "finish" above is what follows the last of them)
        const char *fn[5] = {"trap-terms", "trap-decision", "outputs", "time-level+check_profile", "refill"};
        double fin = (double)t[22];
        fprintf(stderr, " [finish:");
        for (int i = 0; i < 5; ++i) { fprintf(stderr, " %s=%.0f", fn[i], (double)t[26 + i] / (double)t[31]); fin += (double)t[26 + i]; tot += (double)t[26 + i]; }
        fprintf(stderr, " all=%.0f]", fin / (double)t[31]);
      }
      fprintf(stderr, " total=%.0f\n", tot / (double)t[31]);
      if (t[38] + t[39]) fprintf(stderr, "[mckpp steps ps] diagnostic column-steps %llu, lean %llu\n", t[38], t[39]);
      if (t[32] + t[33])   // how far down L3 formed the bulk Richardson numbers, per workgroup pass (first: a column was started before it)
        fprintf(stderr, "[mckpp guesses ps] first passes %llu, mean kguess %.1f; later passes %llu, mean kguess %.1f; second rounds %llu "
                        "(%.4f of the passes); mean end of the first scan %.1f\n",
                t[32], t[32] ? (double)t[34] / (double)t[32] : 0.0, t[33], t[33] ? (double)t[35] / (double)t[33] : 0.0, t[36],
                (double)t[36] / (double)(t[32] + t[33]), (double)t[37] / (double)(t[32] + t[33]));
    }
  }
  return 0;
  });
}

const char *mckpp_hip_kernel_name(mckpp_hip_handle h)
{
  if (!h) return "none";
  return h->ext_kernel ? "k_column_ps<EXT>" : "k_column_ps";
}

int mckpp_hip_kernel_residency(mckpp_hip_handle h, int32_t *blocks_per_cu, int32_t *max_blocks_per_cu,
                               int32_t *threads_per_block, int64_t *lds_bytes_per_block)
{
  return entry(__func__, h, [&]() -> int {
  if (h->last_launch.threads == 0)
    return fail("mckpp_hip_kernel_residency: no cooperative-kernel launch yet");
  if (blocks_per_cu) *blocks_per_cu = (h->last_launch.nblocks + h->num_cu - 1) / h->num_cu;
  if (max_blocks_per_cu) *max_blocks_per_cu = h->last_launch.max_blocks_per_cu;
  if (threads_per_block) *threads_per_block = h->last_launch.threads;
  if (lds_bytes_per_block) *lds_bytes_per_block = (int64_t)h->last_launch.lds_bytes;
  return 0;
  });
}

int mckpp_hip_last_kernel_ms(mckpp_hip_handle h, double *ms, int32_t *nlaunch)
{
  return entry(__func__, h, [&]() -> int {
  if (!h->timed) { if (ms) *ms = 0.0; if (nlaunch) *nlaunch = 0; return 0; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventSynchronize(h->ev1));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, h->ev0, h->ev1));
  if (ms) *ms = (double)t;
  if (nlaunch) *nlaunch = h->nlaunch;
  return 0;
  });
}

int32_t mckpp_hip_last_launch_count(mckpp_hip_handle h) { return h && h->timed ? h->nkernels : 0; }

// The per-column records of one context -> the caller's (npts) arrays: one transfer of each record array into
// pinned memory, then a host loop over the context's columns.
static int download_records(mckpp_hip_ctx *h, mckpp_state_ptrs_c *s, uint32_t mask)
{
  const int nzp1 = h->nzp1, nz = h->nz;
  const int64_t npts = h->npts, ncol = h->ncol;
  const bool want_tabs = (mask & MCKPP_F_DIAG) && (s->swfrac || s->swdk_opt);
  if (!(mask & (MCKPP_F_SAVED | MCKPP_F_SCALARS)) && !want_tabs) return 0;
  // where each entry of the record tables goes in the caller's arrays (null: not wanted), resolved once: both paths
  // below work from it
  constexpr int ND = (int)std::size(rec_doubles), NI = (int)std::size(rec_ints);
  double *dd[ND];
  int32_t *di[NI];
  for (int j = 0; j < ND; ++j) {
    const rec_double &e = rec_doubles[j];
    dd[j] = (e.group & mask) && s->*e.member && (!e.ext_only || h->ext) ? s->*e.member + rec_offset(h, e) : nullptr;
  }
  for (int j = 0; j < NI; ++j) di[j] = (rec_ints[j].group & mask) ? s->*rec_ints[j].member : nullptr;
  if (ncol == npts && !want_tabs) {
    mckpp_pack_list l{};   // the wanted slots, in the tables' order
    for (int j = 0; j < ND; ++j) if (dd[j]) l.dslot[l.nd++] = rec_doubles[j].slot;
    for (int j = 0; j < NI; ++j) if (di[j]) l.islot[l.ni++] = rec_ints[j].slot;
    // every grid point is a resident column: the wanted record slots are packed into (npts) slabs on the device and
    // land in the caller's arrays as they are - no host loop, half the bytes.
    // One device block (the double slabs, then the int slabs right behind them) and ONE transfer of it into a pinned
    // block of the library's own; the caller's arrays - a dozen of them, anywhere - are filled from there by the host
    // threads.  (A transfer per array costs a round trip each: 1.8 ms of a 4.7 ms drop-in step on a link that has
    // been idle, r03.)
    const size_t pack_bytes = (size_t)npts * (MCKPP_CS * sizeof(double) + MCKPP_CI * sizeof(int));
    if (!h->d_pack) HIPCHK(h->d_pack.alloc((pack_bytes + 7) / sizeof(double)));
    if (!h->h_pack) HIPCHK(h->h_pack.alloc((pack_bytes + 7) / sizeof(double)));
    int *d_ipack = reinterpret_cast<int *>(h->d_pack + (size_t)npts * l.nd);
    HIPCHK(mckpp_launch_pack_records(h->d_cs, h->d_ci, h->d_ipt, ncol, npts, l, h->d_pack, d_ipack, h->stream));
    const size_t used = (size_t)npts * (l.nd * sizeof(double) + l.ni * sizeof(int));
    if (used) HIPCHK(hipMemcpyAsync(h->h_pack, h->d_pack, used, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double *hd = h->h_pack;
    const int *hi = reinterpret_cast<const int *>(h->h_pack + (size_t)npts * l.nd);
    for_columns(npts, [&](int64_t c0, int64_t c1) {
      for (int j = 0, k = 0; j < ND; ++j) if (dd[j]) memcpy(dd[j] + c0, hd + (size_t)npts * k++ + c0, (size_t)(c1 - c0) * sizeof(double));
      for (int j = 0, k = 0; j < NI; ++j) if (di[j]) memcpy(di[j] + c0, hi + (size_t)npts * k++ + c0, (size_t)(c1 - c0) * sizeof(int));
    });
    return 0;
  }
  if (mask & (MCKPP_F_SAVED | MCKPP_F_SCALARS))
    HIPCHK(hipMemcpyAsync(h->h_cs, h->d_cs, (size_t)ncol * MCKPP_CS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(h->h_ci, h->d_ci, (size_t)ncol * MCKPP_CI * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const double *cs = h->h_cs;
  const int *ci = h->h_ci;
  const int *ipt = h->ipt.data();
  for_columns(ncol, [&](int64_t c0, int64_t c1) {
    // one pass over each record; the loops over the tables have constant bounds and constant slots, so they compile to
    // the straight lines one would write by hand: a test of the destination and a store per entry
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t i = ipt[c];
      const double *r = &cs[(size_t)c * MCKPP_CS];
      const int *q = &ci[(size_t)c * MCKPP_CI];
      for (int j = 0; j < ND; ++j) if (dd[j]) dd[j][i] = r[rec_doubles[j].slot];
      for (int j = 0; j < NI; ++j) if (di[j]) di[j][i] = q[rec_ints[j].slot];
    }
  });
  if (want_tabs) {   // level by level within a block of columns: every destination slab is written front to back
    const double *tf = h->h_swfrac_tab.data(), *tk = h->h_swdk_tab.data();
    const size_t ldc = (size_t)h->ldc;
    for_columns(ncol, [&](int64_t c0, int64_t c1) {
      if (s->swfrac)
        for (int l = 1; l <= nzp1; ++l) {
          double *dst = s->swfrac + npts * (int64_t)(l - 1);
          for (int64_t c = c0; c < c1; ++c) dst[ipt[c]] = tf[(size_t)ci[(size_t)c * MCKPP_CI + CI_JERLOV] * ldc + l];
        }
      if (s->swdk_opt)
        for (int k = 0; k <= nz; ++k) {
          double *dst = s->swdk_opt + npts * (int64_t)k;
          for (int64_t c = c0; c < c1; ++c) dst[ipt[c]] = tk[(size_t)ci[(size_t)c * MCKPP_CI + CI_JERLOV] * ldc + k];
        }
    });
  }
  return 0;
}

int mckpp_hip_download(mckpp_hip_handle h, mckpp_state_ptrs_c *s, uint32_t mask)
{
  return entry(__func__, h, [&]() -> int {
  if (!s) return fail("mckpp_hip_download: null argument");
  if (s->npts != h->npts) return fail("mckpp_hip_download: npts=%lld but %lld were uploaded", (long long)s->npts, (long long)h->npts);
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  std::vector<row_xfer> plan;
  row_plan(h, s, T_DOWN, mask, plan);
  for (const row_xfer &x : plan)
    if (down_rows(h, x.dev, h->ld, x.off, x.nlev, x.host, x.whole, x.whole_elems)) return -1;
  if (download_records(h, s, mask)) return -1;   // (waits for the context's stream: the last step has finished)
  return xfer_finish(h);
  });
}

// ---------------------------------------------------------------------------
// Restart set.  The reference writes U,V,T,S,CP,rho,hmix,kmix,Sref,SSref,Ssurf,
// Tref,old,new,Us,Vs,Ts,Ss,hmixd through XIOS (src/mckpp_xios_io.F90:368-387, 413-431) and reads
// them back at :436-465; here the same set (the device-resident state) goes to a flat binary file.
// ---------------------------------------------------------------------------
namespace {
struct restart_header {
  char magic[8];
  int32_t version, nz, ld, cs, ci, nprof;
  int64_t npts, ncol;
};
const char kRestartMagic[8] = {'M', 'C', 'K', 'P', 'P', 'R', 'S', '1'};

// The payload of a restart file as device segments in file order: RESTART_ROWS whole rows (ncol * ld doubles each: the
// profile rows in the order of the P_ enumeration, cp, rho), the cs records, the ci records.  Their source is the live
// state, or (slot >= 0) a slot of the restart schedule's ring: the same rows in the same order but U_init / V_init, which
// no step writes and the live rows give (k_column_ps, finish round: planes 0 .. P_UINIT - 1, then cp, rho).
enum { RESTART_ROWS = P_COUNT + 2 };   // restart_header::nprof
static_assert(P_UINIT == P_COUNT - 2 && P_VINIT == P_COUNT - 1 && MCKPP_SNAP_ROWS == RESTART_ROWS - 2,
              "a snapshot slot: the profile rows, which U_init and V_init end, without those two; cp; rho");
struct restart_seg { char *dev; size_t bytes; };
static void restart_segments(mckpp_hip_ctx *h, int64_t slot, std::vector<restart_seg> &segs)
{
  const size_t rowelems = (size_t)h->ncol * h->ld, ncs = (size_t)h->ncol * MCKPP_CS, nci = (size_t)h->ncol * MCKPP_CI;
  double *snap = slot < 0 ? nullptr : h->rs.rows + (size_t)slot * MCKPP_SNAP_ROWS * rowelems;   // the slot's next plane
  for (int i = 0; i < RESTART_ROWS; ++i) {
    double *row = i < P_COUNT ? h->d_prof[i] : h->d_diag[i == P_COUNT ? D_CP : D_RHO];
    if (snap && i != P_UINIT && i != P_VINIT) { row = snap; snap += rowelems; }
    segs.push_back({reinterpret_cast<char *>(row), rowelems * sizeof(double)});
  }
  segs.push_back({reinterpret_cast<char *>(slot < 0 ? h->d_cs.get() : h->rs.cs + (size_t)slot * ncs), ncs * sizeof(double)});
  segs.push_back({reinterpret_cast<char *>(slot < 0 ? h->d_ci.get() : h->rs.ci + (size_t)slot * nci), nci * sizeof(int)});
}

// The file of a restart set - the one writer of mckpp_hip_save_restart and mckpp_hip_restart_snapshot_save: the
// header, the column map, then what `payload` writes: the segments of restart_segments.
int restart_write(mckpp_hip_ctx *h, const char *who, const char *path, const std::function<bool(FILE *)> &payload)
{
  FILE *f = fopen(path, "wb");
  if (!f) return fail("%s: cannot open %s", who, path);
  restart_header hd{};
  memcpy(hd.magic, kRestartMagic, 8);
  hd.version = 1; hd.nz = h->nz; hd.ld = h->ld; hd.cs = MCKPP_CS; hd.ci = MCKPP_CI; hd.nprof = RESTART_ROWS;
  hd.npts = h->npts; hd.ncol = h->ncol;
  bool ok = fwrite(&hd, sizeof hd, 1, f) == 1;
  ok = ok && fwrite(h->ipt.data(), sizeof(int), (size_t)h->ncol, f) == (size_t)h->ncol;
  ok = ok && payload(f);
  ok = (fclose(f) == 0) && ok;
  if (!ok) return fail("%s: write to %s failed", who, path);
  return 0;
}
}  // namespace

int mckpp_hip_save_restart(mckpp_hip_handle h, const char *path)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!path) return fail("mckpp_hip_save_restart: null argument");
  if (h->ncol <= 0) return fail("mckpp_hip_save_restart: no resident columns");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return restart_write(h, who, path, [&](FILE *f) {
    std::vector<char> buf;
    std::vector<restart_seg> segs;
    restart_segments(h, -1, segs);
    for (const restart_seg &g : segs) {
      if (g.bytes > buf.size()) buf.resize(g.bytes);
      if (hipMemcpy(buf.data(), g.dev, g.bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
      if (fwrite(buf.data(), 1, g.bytes, f) != g.bytes) return false;
    }
    return true;
  });
  });
}

// ---------------------------------------------------------------------------
// Restart snapshots taken inside the step launches (mckpp_hip_restart_schedule): k_column_ps copies the restart set
// of every column that has finished a scheduled step into a ring slot (see mckpp_kparams_t::snap_*).  The host keeps
// the bookkeeping, as for the output schedules: which steps have run under the schedule, so which snapshots are
// complete, and which are released; a launch that would overwrite a kept snapshot fails before anything is launched.
// Snapshot s is the state after step origin + (s+1)*period - 1.
// ---------------------------------------------------------------------------
static long long snap_step(const mckpp_hip_ctx::snap_sched &r, int64_t s) { return r.origin + (s + 1) * r.period - 1; }

// the first snapshot whose step is nt0 or later
static int64_t snap_first_from(const mckpp_hip_ctx::snap_sched &r, int64_t nt0)
{
  return nt0 <= r.origin ? 0 : (nt0 - r.origin) / r.period;
}

// the last snapshot whose step has run (-1: none)
static int64_t snap_last_complete(const mckpp_hip_ctx::snap_sched &r)
{
  if (r.next_nt < 0 || r.next_nt < r.origin) return -1;
  return (r.next_nt - r.origin) / r.period - 1;
}

static int snap_cancel(mckpp_hip_ctx *h)
{
  auto &r = h->rs;
  if (r.period == 0) return 0;
  if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still write the slots
  if (h->snap_stream) HIPCHK(hipStreamSynchronize(h->snap_stream));
  r = mckpp_hip_ctx::snap_sched{};
  return 0;
}

static int snap_check_launch(mckpp_hip_ctx *h, int nt0, int nsteps, const char *who)
{
  const auto &r = h->rs;
  if (r.period == 0) return 0;
  const int64_t last = (int64_t)nt0 + nsteps - 1;
  if (r.next_nt >= 0 && nt0 != r.next_nt)
    return fail("%s: steps %d..%lld, but the restart schedule has run up to step %lld: the steps under a schedule follow "
                "on from one another (the next launch starts at step %lld)", who, nt0, (long long)last,
                (long long)r.next_nt - 1, (long long)r.next_nt);
  if (last - r.origin + 1 < r.period) return 0;   // no snapshot step yet
  const int64_t kept = r.first_nt < 0 ? snap_first_from(r, nt0) : r.first_kept;
  const int64_t sl = (last - r.origin + 1) / r.period - 1;
  if (sl >= kept + r.nslots)
    return fail("%s: steps %d..%lld reach restart snapshot %lld (after step %lld), whose slot in the ring of %d still holds "
                "snapshot %lld (after step %lld), not released: save and release snapshots first", who, nt0, (long long)last,
                (long long)sl, snap_step(r, sl), r.nslots, (long long)(sl - r.nslots), snap_step(r, sl - r.nslots));
  return 0;
}

// after the call's launches: the schedule knows the steps, and every snapshot they completed gets the event its
// save waits for
static int snap_advance(mckpp_hip_ctx *h, int nt0, int nsteps)
{
  auto &r = h->rs;
  if (r.period == 0) return 0;
  if (r.first_nt < 0) { r.first_nt = nt0; r.first_exists = r.first_kept = snap_first_from(r, nt0); }
  r.next_nt = (int64_t)nt0 + nsteps;
  if (h->ncol == 0) return 0;
  const int64_t lc = snap_last_complete(r);
  for (int64_t s = std::max(r.first_exists, snap_first_from(r, nt0)); s <= lc; ++s)
    HIPCHK(hipEventRecord(r.ev[(size_t)(s % r.nslots)], h->stream));
  return 0;
}

int mckpp_hip_restart_schedule(mckpp_hip_handle h, int nt_origin, int period, int nslots)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (period < 0) return fail("%s: period=%d (0 cancels the schedule)", who, period);
  if (period > 0) {   // everything is checked before the schedule in place is touched
    if (nt_origin < 1 || nslots < 1) return fail("%s: nt_origin=%d nslots=%d (each at least 1)", who, nt_origin, nslots);
    if (h->npts <= 0) return fail("%s: upload the state first (the slots are sized to the resident columns)", who);
  }
  HIPCHK(hipSetDevice(h->device));
  if (snap_cancel(h)) return -1;
  if (period == 0) return 0;
  mckpp_hip_ctx::snap_sched r;   // built here, moved in when all of it is there
  if (h->ncol > 0) {
    if (!h->snap_stream) HIPCHK(h->snap_stream.create());
    const size_t plane = (size_t)h->ncol * h->ld;
    const size_t ne[3] = {(size_t)nslots * MCKPP_SNAP_ROWS * plane, (size_t)nslots * h->ncol * MCKPP_CS, (size_t)nslots * h->ncol * MCKPP_CI};
    r.ev.resize((size_t)nslots);
    hipError_t e = r.rows.alloc(ne[0]);
    if (e == hipSuccess) e = r.cs.alloc(ne[1]);
    if (e == hipSuccess) e = r.ci.alloc(ne[2]);
    for (int i = 0; i < nslots && e == hipSuccess; ++i) e = r.ev[(size_t)i].create();
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail("%s: cannot allocate %zu bytes of device memory for the %d snapshot slots (%s); the schedule is not set",
                  who, (ne[0] + ne[1]) * sizeof(double) + ne[2] * sizeof(int), nslots, hipGetErrorString(e));
    }
  }
  r.origin = nt_origin; r.period = period; r.nslots = nslots;
  h->rs = std::move(r);
  return 0;
  });
}

int mckpp_hip_restart_snapshots(mckpp_hip_handle h, int64_t *first_kept, int64_t *last_complete)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (h->rs.period == 0) return fail("%s: no restart schedule is set", who);
  if (first_kept) *first_kept = h->rs.first_kept;
  if (last_complete) *last_complete = snap_last_complete(h->rs);
  return 0;
  });
}

int mckpp_hip_restart_snapshot_release(mckpp_hip_handle h, int64_t upto_snap)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  auto &r = h->rs;
  if (r.period == 0) return fail("%s: no restart schedule is set", who);
  const int64_t lc = snap_last_complete(r);
  if (upto_snap > lc)
    return fail("%s: snapshot %lld (after step %lld) is not complete (complete are up to snapshot %lld)", who,
                (long long)upto_snap, snap_step(r, upto_snap), (long long)lc);
  if (upto_snap + 1 > r.first_kept) r.first_kept = upto_snap + 1;
  return 0;
  });
}

// Snapshot `snap` as the file mckpp_hip_save_restart would have written after the snapshot's step.  Waits for the
// event behind the launches of the call that completed the snapshot - not for the context's stream: launches queued
// later keep running, and the ring guard keeps them off the slot.  The copies run on the snapshot transfer stream
// through two pinned staging blocks: the next chunk crosses the bus while the previous one is written to the file.
int mckpp_hip_restart_snapshot_save(mckpp_hip_handle h, int64_t snap, const char *path)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!path) return fail("%s: null argument", who);
  const auto &r = h->rs;
  if (r.period == 0) return fail("%s: no restart schedule is set", who);
  if (snap < 0) return fail("%s: snapshot %lld", who, (long long)snap);
  const long long st = snap_step(r, snap);
  if (r.first_nt >= 0 && snap < r.first_exists)
    return fail("%s: snapshot %lld (after step %lld) does not exist: that step ran before the schedule was set (its first "
                "step was %lld)", who, (long long)snap, st, (long long)r.first_nt);
  if (snap < r.first_kept) return fail("%s: snapshot %lld (after step %lld) has been released", who, (long long)snap, st);
  if (snap > snap_last_complete(r))
    return fail("%s: snapshot %lld (after step %lld) is incomplete: steps have run up to %lld", who, (long long)snap, st,
                (long long)(r.next_nt < 0 ? r.origin - 1 : r.next_nt - 1));
  if (h->ncol <= 0) return fail("%s: no resident columns", who);
  HIPCHK(hipSetDevice(h->device));
  const size_t chunk = (size_t)32 << 20;
  for (int b = 0; b < 2; ++b) {
    if (!h->h_snap[b]) HIPCHK(h->h_snap[b].alloc(chunk));
    if (!h->ev_snap[b]) HIPCHK(h->ev_snap[b].create());
  }
  const size_t slot = (size_t)(snap % r.nslots);
  std::vector<restart_seg> segs, chunks;
  restart_segments(h, (int64_t)slot, segs);
  for (const restart_seg &g : segs)
    for (size_t o = 0; o < g.bytes; o += chunk) chunks.push_back({g.dev + o, std::min(chunk, g.bytes - o)});
  HIPCHK(hipStreamWaitEvent(h->snap_stream, r.ev[slot], 0));
  hipError_t herr = hipSuccess;
  const int rc = restart_write(h, who, path, [&](FILE *f) {
    auto issue = [&](size_t i) {
      herr = hipMemcpyAsync(h->h_snap[i & 1], chunks[i].dev, chunks[i].bytes, hipMemcpyDeviceToHost, h->snap_stream);
      if (herr == hipSuccess) herr = hipEventRecord(h->ev_snap[i & 1], h->snap_stream);
      return herr == hipSuccess;
    };
    if (!issue(0)) return false;
    for (size_t i = 0; i < chunks.size(); ++i) {
      if (i + 1 < chunks.size() && !issue(i + 1)) return false;   // (its block was written out in the previous round)
      herr = hipEventSynchronize(h->ev_snap[i & 1]);
      if (herr != hipSuccess) return false;
      if (fwrite(h->h_snap[i & 1], 1, chunks[i].bytes, f) != chunks[i].bytes) return false;
    }
    return true;
  });
  if (herr != hipSuccess) {
    (void)hipStreamSynchronize(h->snap_stream);
    return fail("%s: copy of snapshot %lld (after step %lld) failed: %s", who, (long long)snap, st, hipGetErrorString(herr));
  }
  return rc;
  });
}

// ---------------------------------------------------------------------------
// The step log (mckpp_hip_step_log): k_column_ps appends a record {nt, resident column, status, passes} for every
// column-step of a MCKPP_MODE_STEP launch that ends flagged or after min_passes passes (mckpp_kparams_t::log_*).  The
// host only sets, reads and zeroes it: no launch is checked against it, and an overflow costs records, never the
// count or the OR of the status words.
// ---------------------------------------------------------------------------
static int log_cancel(mckpp_hip_ctx *h)
{
  if (h->slog.cap == 0) return 0;
  if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still write the records
  h->slog = mckpp_hip_ctx::log_sched{};
  return 0;
}

int mckpp_hip_step_log(mckpp_hip_handle h, int64_t capacity, int min_passes)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (capacity < 0 || min_passes < 0)
    return fail("%s: capacity=%lld min_passes=%d (capacity 0 cancels the log, min_passes 0 logs flagged steps only)", who,
                (long long)capacity, min_passes);
  if (capacity > INT32_MAX) return fail("%s: capacity=%lld (at most %d records)", who, (long long)capacity, INT32_MAX);
  if (capacity > 0 && h->npts <= 0) return fail("%s: upload the state first (the records name the resident columns)", who);
  HIPCHK(hipSetDevice(h->device));
  if (log_cancel(h)) return -1;
  if (capacity == 0) return 0;
  mckpp_hip_ctx::log_sched l;   // built here, moved in when all of it is there
  hipError_t e = l.rec.alloc((size_t)capacity);
  if (e == hipSuccess) e = l.ctl.alloc(2);
  if (e == hipSuccess) e = hipMemsetAsync(l.ctl, 0, 2 * sizeof(int), h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: cannot allocate %zu bytes of device memory for %lld records (%s); no log is set", who,
                (size_t)capacity * sizeof(mckpp_log_rec), (long long)capacity, hipGetErrorString(e));
  }
  l.cap = capacity; l.min_passes = min_passes;
  h->slog = std::move(l);
  return 0;
  });
}

// events so far (the device counts them in 32 bits), how many of them are stored, the OR of all their status words
static int log_read_ctl(mckpp_hip_ctx *h, int64_t *n_events, int64_t *n_stored, int32_t *status_or)
{
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  int ctl[2] = {0, 0};
  HIPCHK(hipMemcpy(ctl, h->slog.ctl, sizeof ctl, hipMemcpyDeviceToHost));
  const int64_t n = (int64_t)(uint32_t)ctl[0];
  if (n_events) *n_events = n;
  if (n_stored) *n_stored = std::min(n, h->slog.cap);
  if (status_or) *status_or = ctl[1];
  return 0;
}

int mckpp_hip_step_log_count(mckpp_hip_handle h, int64_t *n_events, int64_t *n_stored, int32_t *status_or)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (h->slog.cap == 0) return fail("%s: no step log is set", who);
  return log_read_ctl(h, n_events, n_stored, status_or);
  });
}

namespace {
struct log_event { int32_t nt, point, status, npasses; };
bool log_before(const log_event &a, const log_event &b) { return a.nt != b.nt ? a.nt < b.nt : a.point < b.point; }

// the first n stored records of a context, points in the caller's numbering, unsorted
int log_fetch_raw(mckpp_hip_ctx *h, const char *who, int64_t n, std::vector<log_event> &out)
{
  int64_t stored = 0;
  if (log_read_ctl(h, nullptr, &stored, nullptr)) return -1;
  if (n < 0 || n > stored) return fail("%s: n=%lld (%lld records are stored)", who, (long long)n, (long long)stored);
  out.resize((size_t)n);
  if (n == 0) return 0;
  static_assert(sizeof(log_event) == sizeof(mckpp_log_rec), "a record is four ints");
  HIPCHK(hipMemcpy(out.data(), h->slog.rec, (size_t)n * sizeof(log_event), hipMemcpyDeviceToHost));
  for (auto &e : out) {
    if (e.point < 0 || e.point >= h->ncol) return fail("%s: a record names column %d of %lld", who, e.point, (long long)h->ncol);
    e.point = h->ipt[(size_t)e.point];
  }
  return 0;
}

int log_deliver(std::vector<log_event> &ev, int32_t *nt, int32_t *point, int32_t *status, int32_t *npasses)
{
  std::sort(ev.begin(), ev.end(), log_before);
  for (size_t i = 0; i < ev.size(); ++i) {
    if (nt) nt[i] = ev[i].nt;
    if (point) point[i] = ev[i].point;
    if (status) status[i] = ev[i].status;
    if (npasses) npasses[i] = ev[i].npasses;
  }
  return 0;
}
}  // namespace

int mckpp_hip_step_log_fetch(mckpp_hip_handle h, int64_t n, int32_t *nt, int32_t *point, int32_t *status, int32_t *npasses)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (h->slog.cap == 0) return fail("%s: no step log is set", who);
  std::vector<log_event> ev;
  if (log_fetch_raw(h, who, n, ev)) return -1;
  return log_deliver(ev, nt, point, status, npasses);
  });
}

int mckpp_hip_step_log_clear(mckpp_hip_handle h)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (h->slog.cap == 0) return fail("%s: no step log is set", who);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemsetAsync(h->slog.ctl, 0, 2 * sizeof(int), h->stream));   // (behind the launches already queued)
  return 0;
  });
}

int mckpp_hip_load_restart(mckpp_hip_handle h, const char *path)
{
  return entry(__func__, h, [&]() -> int {
  if (!path) return fail("mckpp_hip_load_restart: null argument");
  HIPCHK(hipSetDevice(h->device));
  // The whole file is read and checked on the host first; the resident state is replaced only
  // once everything is known to be there and consistent.
  struct closer { FILE *f; ~closer() { if (f) fclose(f); } } fc{fopen(path, "rb")};
  FILE *f = fc.f;
  if (!f) return fail("mckpp_hip_load_restart: cannot open %s", path);
  restart_header hd{};
  if (fread(&hd, sizeof hd, 1, f) != 1 || memcmp(hd.magic, kRestartMagic, 8) != 0 || hd.version != 1)
    return fail("mckpp_hip_load_restart: %s is not a restart file of this library", path);
  if (hd.nz != h->nz || hd.ld != h->ld || hd.cs != MCKPP_CS || hd.ci != MCKPP_CI || hd.nprof != RESTART_ROWS ||
      hd.ncol <= 0 || hd.ncol > hd.npts)
    return fail("mckpp_hip_load_restart: %s was written for nz=%d (context has nz=%d) or another layout", path,
                hd.nz, h->nz);
  const size_t ncol = (size_t)hd.ncol;
  // the payload as the file holds it (restart_segments): the rows and the cs records, then the ci records
  const size_t ndoubles = ncol * ((size_t)RESTART_ROWS * h->ld + MCKPP_CS), nbytes = ndoubles * sizeof(double) + ncol * MCKPP_CI * sizeof(int);
  std::vector<int> ipt(ncol);
  std::vector<double> payload((nbytes + 7) / sizeof(double));
  const int *ci = reinterpret_cast<const int *>(payload.data() + ndoubles);
  if (fread(ipt.data(), sizeof(int), ipt.size(), f) != ipt.size() || fread(payload.data(), 1, nbytes, f) != nbytes)
    return fail("mckpp_hip_load_restart: %s is truncated or unreadable", path);
  for (size_t c = 0; c < ncol; ++c) {   // the column map scatters into (npts) arrays at download
    if (ipt[c] < 0 || ipt[c] >= hd.npts || (c > 0 && ipt[c] <= ipt[c - 1]))
      return fail("mckpp_hip_load_restart: %s has a corrupt column map (entry %zu = %d, npts = %lld)", path, c,
                  ipt[c], (long long)hd.npts);
    const int jw = ci[c * MCKPP_CI + CI_JERLOV];
    if (jw < 1 || jw > 5) return fail("mckpp_hip_load_restart: %s: jerlov=%d in column %zu", path, jw, c);
  }
  if (new_state(h, hd.npts, ipt, true)) return -1;
  HIPCHK(hipMemcpy(h->d_ipt, ipt.data(), ipt.size() * sizeof(int), hipMemcpyHostToDevice));
  const char *src = reinterpret_cast<const char *>(payload.data());
  std::vector<restart_seg> segs;
  restart_segments(h, -1, segs);
  for (const restart_seg &g : segs) {
    HIPCHK(hipMemcpy(g.dev, src, g.bytes, hipMemcpyHostToDevice));
    src += g.bytes;
  }
  return 0;
  });
}

// Re-upload of what the host rewrites between steps for the optional physics
// (mckpp_boundary_update, src/mckpp_ocean_model_3D.F90:51-55): SST0 / relaxation times, flux
// corrections, climatologies, prescribed advection.  Prognostic state is not touched.
int mckpp_hip_update_ancillaries(mckpp_hip_handle h, const mckpp_state_ptrs_c *s)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!s) return fail("mckpp_hip_update_ancillaries: null argument");
  if (h->npts <= 0) return fail("mckpp_hip_update_ancillaries: no resident state (upload or load_restart first)");
  if (s->npts != h->npts) return fail("mckpp_hip_update_ancillaries: npts=%lld but %lld are resident", (long long)s->npts, (long long)h->npts);
  if (!h->ext || h->ncol == 0) return 0;   // the default physics reads none of them
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return upload_ancillaries(h, s, who);
  });
}

// ---------------------------------------------------------------------------
// Output-window reductions
// ---------------------------------------------------------------------------
namespace {
// Where an output field lives on the device.  3-D fields give nzp1 values per column (the vertical axes of
// src/mckpp_xios_io.F90:96-176: levels 1..nzp1, or interfaces 0..nz for fluxes and diffusivities, whose
// shifted copies temp_2d(:,1)=0, temp_2d(:,2:NZP1)=dif*(:,1:NZ) are exactly dif*(0:nz)); 2-D fields one.
struct out_desc { const double *src; int ld, off, nlev, add_sref; };

int out_field(mckpp_hip_ctx *h, int f, out_desc &d)
{
  const int nzp1 = h->nzp1;
  auto prof = [&](int p) { d = {h->d_prof[p], h->ld, 0, nzp1, 0}; return 0; };             // element j <-> level j+1
  auto diag = [&](int q, int off) { d = {h->d_diag[q], h->ld, off, nzp1, 0}; return 0; };   // element k <-> index k
  auto corr = [&](int o) {
    if (!h->d_ext_out[o]) return fail("mckpp_hip_window: field %d needs the correction rows (optional physics or bottomtemp)", f);
    d = {h->d_ext_out[o], h->ld, 1, nzp1, 0};
    return 0;
  };
  auto scal = [&](int slot) { d = {h->d_cs, MCKPP_CS, slot, 1, 0}; return 0; };
  switch (f) {
    case MCKPP_OUT_U: return prof(P_U);
    case MCKPP_OUT_V: return prof(P_V);
    case MCKPP_OUT_T: return prof(P_T);
    case MCKPP_OUT_S_ANOM: return prof(P_S);
    case MCKPP_OUT_HMIX: return scal(CS_HMIX);
    case MCKPP_OUT_S: prof(P_S); d.add_sref = 1; return 0;
    case MCKPP_OUT_B: return diag(D_BUOY, 1);
    case MCKPP_OUT_WU: return diag(D_WU1, 0);
    case MCKPP_OUT_WV: return diag(D_WU2, 0);
    case MCKPP_OUT_WT: return diag(D_WX1, 0);
    case MCKPP_OUT_WS: return diag(D_WX2, 0);
    case MCKPP_OUT_WB: return diag(D_WX3, 0);
    case MCKPP_OUT_WTNT: return diag(D_WXNT1, 0);
    case MCKPP_OUT_DIFM: return diag(D_DIFM, 0);
    case MCKPP_OUT_DIFT: return diag(D_DIFT, 0);
    case MCKPP_OUT_DIFS: return diag(D_DIFS, 0);
    case MCKPP_OUT_RHO: return diag(D_RHO, 1);
    case MCKPP_OUT_CP: return diag(D_CP, 1);
    case MCKPP_OUT_SCORR: return corr(O_SCORR);
    case MCKPP_OUT_RIG: return diag(D_RIG, 1);
    case MCKPP_OUT_DBLOC: return diag(D_DBLOC, 1);
    case MCKPP_OUT_SHSQ: return diag(D_SHSQ, 1);
    case MCKPP_OUT_TINC_FCORR: return corr(O_TINC);
    case MCKPP_OUT_FCORR_Z: return corr(O_OCNTCORR);
    case MCKPP_OUT_SINC_FCORR: return corr(O_SINC);
    case MCKPP_OUT_FCORR: return scal(CS_FCORR);
    case MCKPP_OUT_TAUX_IN: return scal(CS_SFLUX1);
    case MCKPP_OUT_TAUY_IN: return scal(CS_SFLUX2);
    case MCKPP_OUT_SOLAR_IN: return scal(CS_SFLUX3);
    case MCKPP_OUT_NSOLAR_IN: return scal(CS_SFLUX4);
    case MCKPP_OUT_PMINUSE_IN: return scal(CS_SFLUX6);
    case MCKPP_OUT_FREEZE_FLAG: return scal(CS_FREEZE);
    case MCKPP_OUT_COMP_FLAG: return scal(CS_RESET);
    case MCKPP_OUT_DAMPU_FLAG: return scal(CS_DAMPU);
    case MCKPP_OUT_DAMPV_FLAG: return scal(CS_DAMPV);
    default: return fail("mckpp_hip_window: unknown output field %d", f);
  }
}
}  // namespace

int mckpp_hip_window_select(mckpp_hip_handle h, const int32_t *fields, int32_t nfields)
{
  return entry(__func__, h, [&]() -> int {
  if ((nfields > 0 && !fields) || nfields < 0) return fail("mckpp_hip_window_select: bad argument");
  for (int i = 0; i < nfields; ++i)
    if (fields[i] < 0 || fields[i] >= MCKPP_OUT_COUNT) return fail("mckpp_hip_window_select: unknown output field %d", fields[i]);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->d_wacc.clear();
  h->wsel.assign(fields, fields + nfields);
  h->window_count = 0;
  return 0;
  });
}

int mckpp_hip_window_reset(mckpp_hip_handle h)
{
  return entry(__func__, h, [&]() -> int {
  h->window_count = 0;
  return 0;
  });
}

int mckpp_hip_window_accumulate(mckpp_hip_handle h)
{
  return entry(__func__, h, [&]() -> int {
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (h->d_wacc.size() != h->wsel.size()) h->d_wacc = std::vector<dev_buf<double>>(h->wsel.size());
  for (size_t i = 0; i < h->wsel.size(); ++i) {
    out_desc d;
    if (out_field(h, h->wsel[i], d)) return -1;
    if ((h->wsel[i] >= MCKPP_OUT_B && h->wsel[i] <= MCKPP_OUT_SINC_FCORR) && !h->diag)
      return fail("mckpp_hip_window_accumulate: field %d is a diagnostic, and diagnostics are switched off", h->wsel[i]);
    const int ld_out = d.nlev == 1 ? 1 : h->ld;
    const size_t n = (size_t)h->ncol * ld_out;
    if (!h->d_wacc[i]) HIPCHK(h->d_wacc[i].alloc(3 * n));
    HIPCHK(mckpp_launch_out_sample(d.src, d.ld, d.off, h->d_cs, d.add_sref, h->ncol, d.nlev, ld_out, h->d_wacc[i],
                                   h->d_wacc[i] + n, h->d_wacc[i] + 2 * n, h->window_count == 0, nullptr, h->stream));
  }
  h->window_count += 1;
  return 0;
  });
}

// The reduced (or sampled) field of this context's columns, compacted, left in device memory: `src` rows of
// `ld_out` doubles, `nlev` of them meaningful.  (The mean is formed into the context's staging buffer.)
static int window_prepare(mckpp_hip_ctx *h, int field, int op, const double **src_out, int *ld_out_, int *nlev_)
{
  if (op < 0 || op > 3) return fail("mckpp_hip_window_fetch: op %d (0 mean, 1 min, 2 max, 3 instant)", op);
  out_desc d;
  if (out_field(h, field, d)) return -1;
  const int ld_out = d.nlev == 1 ? 1 : h->ld;
  *ld_out_ = ld_out;
  *nlev_ = d.nlev;
  *src_out = nullptr;
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  const size_t n = (size_t)h->ncol * ld_out;
  if (ensure_stage(h, n)) return -1;
  double *tmp = h->d_stage;
  const double *src = nullptr;
  if (op == 3) {   // the field as it stands (XIOS operation "instant" at the output step)
    HIPCHK(mckpp_launch_out_sample(d.src, d.ld, d.off, h->d_cs, d.add_sref, h->ncol, d.nlev, ld_out, nullptr, nullptr,
                                   nullptr, 0, tmp, h->stream));
    src = tmp;
  } else {
    size_t i = 0;
    while (i < h->wsel.size() && h->wsel[i] != field) ++i;
    if (i == h->wsel.size()) return fail("mckpp_hip_window_fetch: field %d is not among the selected window fields", field);
    if (h->window_count == 0 || i >= h->d_wacc.size() || !h->d_wacc[i]) return fail("mckpp_hip_window_fetch: empty window");
    src = h->d_wacc[i] + (size_t)op * n;
    if (op == 0) {
      HIPCHK(mckpp_launch_window_mean(src, tmp, n, (double)h->window_count, h->stream));
      src = tmp;
    }
  }
  *src_out = src;
  return 0;
}

int mckpp_hip_window_fetch(mckpp_hip_handle h, int field, int op, double *out)
{
  return entry(__func__, h, [&]() -> int {
  if (!out) return fail("mckpp_hip_window_fetch: null argument");
  const double *src = nullptr;
  int ld_out = 0, nlev = 0;
  if (window_prepare(h, field, op, &src, &ld_out, &nlev)) return -1;
  if (h->ncol == 0) return 0;
  if (down_rows(h, src, ld_out, 0, nlev, out)) return -1;
  return xfer_finish(h);
  });
}

// ---------------------------------------------------------------------------
// The device-array interface (include/mckpp_hip_device.h): forcing from the caller's device arrays, output fields into
// them, ordered by events on the caller's stream.  Every call is a check, which queues nothing, and a part that queues.
//
// A call has one body, which takes the contexts it addresses as a ctx_group - a lone context is a group of one, a multi
// handle the group of its shards, shard 0 the root - and keeps one order: every shard is checked before anything is
// queued; the root's lists and tables of the points the group holds are brought up to date; one event goes on the
// caller's stream; every shard's part is queued behind it; the root's last stage, where the call has one, runs.  Both
// extern "C" entries of a call hand their group to that body.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
const char *const flux_field_names[8] = {"taux", "tauy", "swf", "lwf", "lhf", "shf", "rain", "snow"};

// The contexts a call addresses.  kind: what the root's lists and tables of the group's points are marked with (land_kind,
// norow_kind, hgrid_dev::kind) - 1 a lone context's own columns, 2 the union of a multi handle's shards; so a shard
// addressed on its own after its multi handle finds the union's and builds its own again, and the other way round.
// ev: the event recorded on the caller's stream.  A lone context's is its own, on its device (ev_dev null); a multi
// handle's lives on *ev_dev, the device of the call's first array, and is made anew when that changes - the two differ
// for arrays on a peer device.
struct ctx_group {
  mckpp_hip_ctx *const *ctx;
  int n, kind;
  hip_event *ev;
  int *ev_dev;
  mckpp_hip_ctx *root() const { return ctx[0]; }
  mckpp_hip_ctx *const *begin() const { return ctx; }
  mckpp_hip_ctx *const *end() const { return ctx + n; }
};

ctx_group lone(mckpp_hip_ctx *&h) { return ctx_group{&h, 1, 1, &h->ev_caller, nullptr}; }

// what opens the checks of the plane tables: the count against the call's cap, and a state to deliver from or write to
int planes_count_check(const char *who, int32_t nplanes, const void *planes, int cap)
{
  if (nplanes >= 0 && nplanes <= cap && (nplanes == 0 || planes)) return 0;
  return fail("%s: nplanes=%d (0..%d) or a null table", who, nplanes, cap);
}

int uploaded_check(const mckpp_hip_ctx *h, const char *who) { return h->npts > 0 ? 0 : fail("%s: upload the state first", who); }

// Is `p` device memory with room for `bytes` that the context's device reaches?  (The context's device is current.)
int dev_ptr_check(mckpp_hip_ctx *h, const char *who, const char *arg, const void *p, size_t bytes, int *dev_out = nullptr)
{
  if (!p) return fail("%s: %s is null (the context is on device %d, the pointer on no device)", who, arg, h->device);
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) (void)hipGetLastError();   // (runtimes that know no unregistered host memory report it as an error)
  if (e != hipSuccess || a.type != hipMemoryTypeDevice) {
    const char *what = e != hipSuccess || a.type == hipMemoryTypeUnregistered ? "host memory"
                       : a.type == hipMemoryTypeHost ? "pinned host memory"
                       : a.type == hipMemoryTypeManaged ? "managed memory" : "no device allocation";
    return fail("%s: %s is %s: the call takes device arrays (the context is on device %d, the pointer on no device); the "
                "host forms are in mckpp_hip.h", who, arg, what, h->device);
  }
  if (a.device != h->device && std::find(h->peers.begin(), h->peers.end(), a.device) == h->peers.end()) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, h->device, a.device) != hipSuccess) { (void)hipGetLastError(); can = 0; }
    hipError_t pe = can ? hipDeviceEnablePeerAccess(a.device, 0) : hipErrorInvalidDevice;
    if (pe == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); pe = hipSuccess; }
    if (pe != hipSuccess) {
      (void)hipGetLastError();
      return fail("%s: %s is memory of device %d, which the context's device %d cannot reach (no peer access)", who, arg,
                  a.device, h->device);
    }
    h->peers.push_back(a.device);
  }
  void *base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) (void)hipGetLastError();
  else if (static_cast<const char *>(p) + bytes > static_cast<const char *>(base) + size)
    return fail("%s: %s: the allocation holds %zu bytes from the pointer on, the call needs %zu (the context is on device %d, "
                "the pointer on device %d)", who, arg, (size_t)(static_cast<const char *>(base) + size - static_cast<const char *>(p)),
                bytes, h->device, a.device);
  if (dev_out) *dev_out = a.device;
  return 0;
}

// the eight fields of a forcing record; *dev (where asked for): the device they - the first of them - live on
int dev_fields_check(mckpp_hip_ctx *h, const char *who, const double *const fields[8], int *dev)
{
  if (!fields) return fail("%s: null argument", who);
  HIPCHK(hipSetDevice(h->device));
  for (int m = 0; m < 8; ++m) {
    char arg[48];
    snprintf(arg, sizeof arg, "fields[%d] (%s)", m, flux_field_names[m]);
    if (dev_ptr_check(h, who, arg, fields[m], (size_t)h->npts * sizeof(double), m == 0 ? dev : nullptr)) return -1;
  }
  return 0;
}

// The group's event on the caller's stream, recorded now: what the library's streams wait for.  dev: the device of the
// call's first array, taken to be that of the caller's stream (ctx_group::ev).
int caller_event(const ctx_group &g, int dev, void *stream)
{
  if (!g.ev_dev) dev = g.root()->device;
  else if (*g.ev_dev != dev) { g.ev->reset(); *g.ev_dev = dev; }
  HIPCHK(hipSetDevice(dev));
  HIPCHK(g.ev->record(static_cast<hipStream_t>(stream)));
  return 0;
}

// t (null: none): the fields live on a caller's grid and reach the columns through its in table (mckpp_hip_hgrid.h)
int fluxes_dev_queue(mckpp_hip_ctx *h, int ntime, const double *const fields[8], int l_rest, double flsn, double el,
                     hipEvent_t produced, const mckpp_hgrid_ell *t = nullptr)
{
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamWaitEvent(h->stream, produced, 0));
  mckpp_kparams p;
  fill_params(h, p, ntime, MCKPP_MODE_STEP);
  mckpp_dev_fields f;
  for (int m = 0; m < 8; ++m) f.f[m] = fields[m];
  if (t) HIPCHK(mckpp_launch_hgrid_fluxes(p, ntime, *t, f, l_rest, flsn, el, h->stream));
  else HIPCHK(mckpp_launch_fluxes_dev(p, ntime, f, h->d_ipt, l_rest, flsn, el, h->stream));
  HIPCHK(h->ev_read.record(h->stream));
  return 0;
}

int ring_put_dev_queue(mckpp_hip_ctx *h, int rec, const double *const fields[8], hipEvent_t produced,
                       const mckpp_hgrid_ell *t = nullptr)
{
  auto &g = h->ring;
  if (h->ncol > 0) {
    HIPCHK(hipSetDevice(h->device));
    const size_t slot = (size_t)(rec % g.nslots);
    mckpp_dev_fields f;
    for (int m = 0; m < 8; ++m) f.f[m] = fields[m];
    HIPCHK(hipStreamWaitEvent(h->flux_stream, produced, 0));
    // behind the launches of the last call that needed the record the slot held - on the device, never on the host
    HIPCHK(hipStreamWaitEvent(h->flux_stream, g.last_read[slot], 0));
    if (t) HIPCHK(mckpp_launch_hgrid_flux_gather(*t, f, h->ncol, g.slots + slot * 8 * (size_t)h->ncol, h->flux_stream));
    else HIPCHK(mckpp_launch_flux_gather(f, h->d_ipt, h->ncol, g.slots + slot * 8 * (size_t)h->ncol, h->flux_stream));
    HIPCHK(hipEventRecord(g.arrived[slot], h->flux_stream));
    HIPCHK(h->ev_read_flux.record(h->flux_stream));
  }
  ring_put_done(g, rec);
  return 0;
}

// What the checks of the plane tables share (fetch_dev_check, put_check, records_dev_check), for planes[k] of entry `who`.
// Levels lev0 .. lev0 + nlev - 1 of a field's axis of `axis` levels; sched >= 0: the axis is what that schedule keeps.
int plane_levels_check(const char *who, int k, int lev0, int nlev, int field, int axis, int sched = -1)
{
  if (lev0 >= 0 && nlev >= 1 && (int64_t)lev0 + nlev <= axis) return 0;
  if (sched < 0)
    return fail("%s: planes[%d]: lev0=%d nlev=%d is no range of levels of field %d, whose axis has %d (lev0 >= 0, nlev >= 1)",
                who, k, lev0, nlev, field, axis);
  return fail("%s: planes[%d]: lev0=%d nlev=%d is no range of the levels schedule %d keeps of field %d, which are %d (lev0 >= 0, "
              "nlev >= 1)", who, k, lev0, nlev, sched, field, axis);
}

// the size of an element of the plane's dtype; 0, and the refusal, where it is neither of the two
size_t plane_elem(const char *who, int k, int dtype)
{
  if (dtype == MCKPP_EXP_F64 || dtype == MCKPP_EXP_F32) return dtype == MCKPP_EXP_F32 ? sizeof(float) : sizeof(double);
  fail("%s: planes[%d]: dtype %d (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", who, k, dtype);
  return 0;
}

// The planes of a delivery, checked and resolved into the kernel's table; *any_fill: a plane fills the land points
int fetch_dev_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_dev_plane_c *planes,
                    std::vector<mckpp_fetch_plane> &tab, int *maxlev, bool *any_fill, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_DEV_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  tab.clear();
  *maxlev = 0;
  *any_fill = false;
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_dev_plane_c &q = planes[k];
    out_desc d;
    if (out_field(h, q.field, d)) return -1;
    if (plane_levels_check(who, k, q.lev0, q.nlev, q.field, d.nlev)) return -1;
    const size_t elem = plane_elem(who, k, q.dtype);
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d].out", k);
    if (!elem || dev_ptr_check(h, who, arg, q.out, (size_t)h->npts * (size_t)q.nlev * elem, k == 0 ? dev : nullptr)) return -1;
    tab.push_back(mckpp_fetch_plane{d.src, q.out, q.land_value, d.ld, d.off + q.lev0, q.nlev, d.add_sref,
                                    q.dtype == MCKPP_EXP_F32 ? 1 : 0, q.fill_land ? 1 : 0});
    *maxlev = std::max(*maxlev, (int)q.nlev);
    *any_fill = *any_fill || q.fill_land;
  }
  return 0;
}

// A list of the positions a context's planes fill with their land value - the grid's points (mckpp_ctx_resident::d_land)
// or those of a schedule's point list (win_sched::d_norow) - as what `covered` does not mark, with its count and kind.
int fill_list_set(mckpp_hip_ctx *h, dev_buf<int> &d, int64_t &n, int &kind_of, const std::vector<unsigned char> &covered, int kind)
{
  std::vector<int> list;
  for (size_t i = 0; i < covered.size(); ++i)
    if (!covered[i]) list.push_back((int)i);
  HIPCHK(hipSetDevice(h->device));
  // first use, a new column map, or a change of who addresses the shard: a launch in flight may read the old list
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(d.reserve(std::max<size_t>(list.size(), 1)));
  if (!list.empty()) HIPCHK(hipMemcpy(d, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice));
  n = (int64_t)list.size();
  kind_of = kind;
  return 0;
}

// Which points does the group hold?  covered[i]: point i is a resident column of one of its contexts.
int group_columns(const ctx_group &g, const char *who, std::vector<unsigned char> &covered)
{
  covered.assign((size_t)g.root()->npts, 0);
  for (auto *x : g)
    for (int i : x->ipt) {
      if (i < 0 || (size_t)i >= covered.size()) return fail("%s: a column map names a point outside the grid", who);
      covered[(size_t)i] = 1;
    }
  return 0;
}

// the root's land list as the points the group does not hold, where it is not that already: the root fills them, the
// other shards of a multi handle fill none, so every point is written once
int group_land(const ctx_group &g, const char *who)
{
  mckpp_hip_ctx *root = g.root();
  if (root->land_kind == g.kind) return 0;
  std::vector<unsigned char> covered;
  if (group_columns(g, who, covered)) return -1;
  return fill_list_set(root, root->d_land, root->nland, root->land_kind, covered, g.kind);
}

// any_fill: this context fills the land points (group_land has brought its list up to date)
int fetch_dev_queue(mckpp_hip_ctx *h, const std::vector<mckpp_fetch_plane> &tab, int maxlev, bool any_fill, hipEvent_t before,
                    void *consumer_stream)
{
  if (tab.empty()) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->fetch_tab.put(tab, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(mckpp_launch_fetch_planes(h->fetch_tab, (int)tab.size(), maxlev, h->d_ipt, h->ncol, h->npts, h->d_cs,
                                   any_fill ? h->d_land.get() : nullptr, any_fill ? h->nland : 0, h->stream));
  HIPCHK(h->ev_delivered.record(h->stream));
  HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_delivered, 0));
  return 0;
}

int dev_fence_queue(mckpp_hip_ctx *h, void *stream)
{
  if (h->ev_read) HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->ev_read, 0));
  if (h->ev_read_flux) HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->ev_read_flux, 0));
  return 0;
}

// (what a forcing call on a caller's grid checks in place of dev_fields_check: with the caller's horizontal grids, below)
int hgrid_in_check(mckpp_hip_ctx *h, const char *who, int grid, const double *const fields[8], mckpp_hgrid_ell *t, int *dev);

// mckpp_hip_fluxes_dev and, with a grid (include/mckpp_hip_hgrid.h), mckpp_hip_hgrid_fluxes_dev: every shard forms the
// forcing of its own columns from the same caller arrays
int fluxes_dev(const ctx_group &g, const char *who, int ntime, const double *const fields[8], int l_rest, double flsn, double el,
               void *producer_stream, const int *grid = nullptr)
{
  std::vector<mckpp_hgrid_ell> t((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (!grid ? dev_fields_check(g.ctx[d], who, fields, &dev) : hgrid_in_check(g.ctx[d], who, *grid, fields, &t[(size_t)d], &dev))
      return -1;
  if (dev < 0) return 0;
  if (caller_event(g, dev, producer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (fluxes_dev_queue(g.ctx[d], ntime, fields, l_rest, flsn, el, *g.ev, grid ? &t[(size_t)d] : nullptr)) return -1;
  return 0;
}

// mckpp_hip_flux_ring_put_dev and mckpp_hip_hgrid_flux_ring_put_dev likewise
int flux_ring_put_dev(const ctx_group &g, const char *who, int rec, const double *const fields[8], void *producer_stream,
                      const int *grid = nullptr)
{
  if (!fields) return fail("%s: null argument", who);
  std::vector<mckpp_hgrid_ell> t((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d) {
    if (ring_put_check(g.ctx[d], who, rec)) return -1;
    if (!grid ? dev_fields_check(g.ctx[d], who, fields, &dev) : hgrid_in_check(g.ctx[d], who, *grid, fields, &t[(size_t)d], &dev))
      return -1;
  }
  if (dev < 0) return 0;
  if (caller_event(g, dev, producer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (ring_put_dev_queue(g.ctx[d], rec, fields, *g.ev, grid ? &t[(size_t)d] : nullptr)) return -1;
  return 0;
}

// mckpp_hip_fetch_dev: a shard writes its own columns of every plane, the root the land values
int fetch_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_dev_plane_c *planes, void *consumer_stream)
{
  std::vector<std::vector<mckpp_fetch_plane>> tabs((size_t)g.n);
  int maxlev = 0, dev = -1;
  bool any_fill = false;
  for (int d = 0; d < g.n; ++d)
    if (fetch_dev_check(g.ctx[d], who, nplanes, planes, tabs[(size_t)d], &maxlev, &any_fill, &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  if (any_fill) {
    for (int d = 1; d < g.n; ++d)
      for (auto &e : tabs[(size_t)d]) e.fill_land = 0;
    if (group_land(g, who)) return -1;
  }
  if (caller_event(g, dev, consumer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (fetch_dev_queue(g.ctx[d], tabs[(size_t)d], maxlev, any_fill && d == 0, *g.ev, consumer_stream)) return -1;
  return 0;
}

int dev_fence(const ctx_group &g, void *stream)
{
  for (auto *x : g)
    if (dev_fence_queue(x, stream)) return -1;
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_fluxes_dev(mckpp_hip_handle h, int ntime, const double *const fields[8], int l_rest, double flsn, double el,
                         void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return fluxes_dev(lone(h), who, ntime, fields, l_rest, flsn, el, producer_stream); });
}

int mckpp_hip_flux_ring_put_dev(mckpp_hip_handle h, int rec, const double *const fields[8], void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return flux_ring_put_dev(lone(h), who, rec, fields, producer_stream); });
}

int mckpp_hip_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_dev_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return fetch_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_dev_fence(mckpp_hip_handle h, void *stream)
{
  return entry(__func__, h, [&]() -> int { return dev_fence(lone(h), stream); });
}

// ---------------------------------------------------------------------------
// State in from the caller's arrays (include/mckpp_hip_put.h): U, V, T, S set or incremented in place by one launch of
// k_put_planes.  A check, which queues nothing, and a part that queues in fluxes_dev_queue's order; a multi handle
// checks all its shards before any of them queues.  Nothing of the context's bookkeeping is touched: a put is an edit
// of the profile rows (and of the reference slots of cs that follow level 1), which the column kernel reads at the
// start of every step.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
// What planes[k] of a put says apart from its array, checked and resolved into the kernel's entry (`in` left null) - the
// one statement of it for put_check and for vaxis_put_check (include/mckpp_hip_vaxis.h), whose planes write levels
// 0 .. nzp1 - 1.  *row: the profile the plane writes (the overlap check's key); *elem: the size of an element.
int put_resolve(mckpp_hip_ctx *h, const char *who, int k, int field, int lev0, int nlev, int dtype, int op, int flags,
                double skip_value, mckpp_put_plane &e, int *row_out, size_t *elem_out)
{
  int row, lv0, lv1, ref;
  switch (field) {
    case MCKPP_OUT_U: row = P_U; lv0 = P_US0; lv1 = P_US1; ref = CS_UREF; break;
    case MCKPP_OUT_V: row = P_V; lv0 = P_VS0; lv1 = P_VS1; ref = CS_VREF; break;
    case MCKPP_OUT_T: row = P_T; lv0 = P_TS0; lv1 = P_TS1; ref = CS_TREF; break;
    case MCKPP_OUT_S_ANOM:
    case MCKPP_OUT_S: row = P_S; lv0 = P_SS0; lv1 = P_SS1; ref = h->c.L_SSref ? -1 : CS_SSURF; break;   // L_SSref: Ssurf stays SSref
    default:
      if (field < 0 || field >= MCKPP_OUT_COUNT) return fail("%s: planes[%d]: unknown output field %d", who, k, field);
      return fail("%s: planes[%d]: field %d is an output of the step, not state (MCKPP_OUT_U %d, _V %d, _T %d, _S_ANOM %d, _S %d)",
                  who, k, field, MCKPP_OUT_U, MCKPP_OUT_V, MCKPP_OUT_T, MCKPP_OUT_S_ANOM, MCKPP_OUT_S);
  }
  out_desc d;
  if (out_field(h, field, d)) return -1;
  if (plane_levels_check(who, k, lev0, nlev, field, d.nlev)) return -1;
  const size_t elem = plane_elem(who, k, dtype);
  if (!elem) return -1;
  if (op != MCKPP_PUT_SET && op != MCKPP_PUT_ADD)
    return fail("%s: planes[%d]: op %d (MCKPP_PUT_SET 0, MCKPP_PUT_ADD 1)", who, k, op);
  if (flags & ~(MCKPP_PUT_SKIP | MCKPP_PUT_TIME_LEVELS))
    return fail("%s: planes[%d]: flags %#x (a mask of MCKPP_PUT_SKIP 1, MCKPP_PUT_TIME_LEVELS 2)", who, k, (unsigned)flags);
  const bool skip = flags & MCKPP_PUT_SKIP, levels = flags & MCKPP_PUT_TIME_LEVELS;
  if (skip && std::isnan(skip_value))
    return fail("%s: planes[%d]: the skip value is NaN, which no element compares equal to", who, k);
  const bool add = op == MCKPP_PUT_ADD;
  e = mckpp_put_plane{nullptr, h->d_prof[row].get(), levels ? h->d_prof[lv0].get() : nullptr,
                      levels ? h->d_prof[lv1].get() : nullptr, skip_value, d.ld, d.off + lev0, nlev,
                      dtype == MCKPP_EXP_F32 ? 1 : 0, add ? 1 : 0, skip ? 1 : 0, (!add && d.add_sref) ? 1 : 0,
                      lev0 == 0 ? ref : -1, ref == CS_SSURF ? 1 : 0};
  *row_out = row;
  *elem_out = elem;
  return 0;
}

// The planes of a call have no order: planes[k], which writes profile `row`, may share no level of it with a plane
// before it (prof[j]: the profile planes[j] writes; prof[k] is set).  For the calls whose planes name their levels.
template <class P>
int put_overlap_check(const char *who, int k, const P *planes, int *prof, int row)
{
  const P &q = planes[k];
  for (int j = 0; j < k; ++j)
    if (prof[j] == row && q.lev0 < planes[j].lev0 + planes[j].nlev && planes[j].lev0 < q.lev0 + q.nlev)
      return fail("%s: planes[%d] and planes[%d] write the same field (%d, %d) at overlapping levels %d..%d and %d..%d: the "
                  "planes of a call have no order", who, k, j, q.field, planes[j].field, q.lev0, q.lev0 + q.nlev - 1,
                  planes[j].lev0, planes[j].lev0 + planes[j].nlev - 1);
  prof[k] = row;
  return 0;
}

// The planes of a put, checked and resolved into the kernel's table.  dev_form: `in` is device memory (*dev, where asked
// for: the device of the first plane's); otherwise host memory, and the table's `in` is set by put_host_queue.
int put_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_put_plane_c *planes, bool dev_form,
              std::vector<mckpp_put_plane> &tab, int *maxlev, int *dev)
{
  if (uploaded_check(h, who) || planes_count_check(who, nplanes, planes, MCKPP_PUT_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  tab.clear();
  *maxlev = 0;
  int prof[MCKPP_PUT_PLANES_MAX];
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_put_plane_c &q = planes[k];
    mckpp_put_plane e;
    int row;
    size_t elem;
    if (put_resolve(h, who, k, q.field, q.lev0, q.nlev, q.dtype, q.op, q.flags, q.skip_value, e, &row, &elem)) return -1;
    if (put_overlap_check(who, k, planes, prof, row)) return -1;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d].in", k);
    if (!dev_form) {
      if (!q.in) return fail("%s: %s is null", who, arg);
    } else if (dev_ptr_check(h, who, arg, q.in, (size_t)h->npts * (size_t)q.nlev * elem, k == 0 ? dev : nullptr)) {
      return -1;
    }
    e.in = q.in;
    tab.push_back(e);
    *maxlev = std::max(*maxlev, (int)q.nlev);
  }
  return 0;
}

// the table onto the device on the context's stream, a wait for `produced` (null: none), the launch, ev_read behind it
int put_queue(mckpp_hip_ctx *h, const std::vector<mckpp_put_plane> &tab, int maxlev, hipEvent_t produced)
{
  if (tab.empty() || h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->put_tab.put(tab, h->stream));
  if (produced) HIPCHK(hipStreamWaitEvent(h->stream, produced, 0));
  HIPCHK(mckpp_launch_put_planes(h->put_tab, (int)tab.size(), maxlev, h->d_ipt, h->ncol, h->npts, h->d_cs, h->stream));
  HIPCHK(h->ev_read.record(h->stream));
  return 0;
}

// the host form: every plane as it is into the context's staging (each at a multiple of 256 bytes) on the context's
// stream, the launch, and the wait that lets the caller rewrite its arrays and the staging be reused
int put_host_queue(mckpp_hip_ctx *h, std::vector<mckpp_put_plane> &tab, int maxlev)
{
  if (tab.empty() || h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  std::vector<size_t> at(tab.size()), bytes(tab.size());
  size_t total = 0;
  for (size_t k = 0; k < tab.size(); ++k) {
    bytes[k] = (size_t)h->npts * (size_t)tab[k].nlev * (tab[k].f32 ? sizeof(float) : sizeof(double));
    at[k] = total;
    total += (bytes[k] + 255) / 256 * 256;
  }
  HIPCHK(h->d_put_stage.reserve(total));
  for (size_t k = 0; k < tab.size(); ++k) {
    HIPCHK(hipMemcpyAsync(h->d_put_stage + at[k], tab[k].in, bytes[k], hipMemcpyHostToDevice, h->stream));
    tab[k].in = h->d_put_stage + at[k];
  }
  if (put_queue(h, tab, maxlev, nullptr)) return -1;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// mckpp_hip_put_dev / _put_host: the same planes for every shard, which writes its own columns only
int put_planes(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_put_plane_c *planes, bool dev_form,
               void *producer_stream)
{
  std::vector<std::vector<mckpp_put_plane>> tabs((size_t)g.n);
  int maxlev = 0, dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (put_check(g.ctx[d], who, nplanes, planes, dev_form, tabs[(size_t)d], &maxlev, dev_form ? &dev : nullptr)) return -1;
  if (dev_form) {
    if (dev < 0) return 0;   // (no plane)
    if (caller_event(g, dev, producer_stream)) return -1;
  }
  for (int d = 0; d < g.n; ++d)
    if (dev_form ? put_queue(g.ctx[d], tabs[(size_t)d], maxlev, *g.ev) : put_host_queue(g.ctx[d], tabs[(size_t)d], maxlev)) return -1;
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return put_planes(lone(h), who, nplanes, planes, true, producer_stream); });
}

int mckpp_hip_put_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_put_plane_c *planes)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return put_planes(lone(h), who, nplanes, planes, false, nullptr); });
}

// ---------------------------------------------------------------------------
// The caller's vertical axes (include/mckpp_hip_vaxis.h): axes defined per context, state in and the reference's
// initial profiles through the in table (k_vaxis_put_planes, k_vaxis_init_finish), fields out through the out table
// (k_vaxis_fetch_planes).  Checks queue nothing; the parts that queue keep put_queue's and fetch_dev_queue's order.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
// an axis table built on the host and copied to the device (the context's device is current); keep_branch, keep_kin
// (null: not kept): its branches and source levels, for the host
int vaxis_table(const char *who, int ns, const double *zs, int nt, const double *zt, dev_buf<mckpp_vaxis_ent> &d,
                std::vector<int32_t> *keep_branch = nullptr, std::vector<int32_t> *keep_kin = nullptr)
{
  std::vector<int32_t> branch((size_t)nt), kin((size_t)nt);
  std::vector<double> t((size_t)nt), dz((size_t)nt);
  if (mckpp_host_vaxis_map(ns, zs, nt, zt, branch.data(), kin.data(), t.data(), dz.data()))
    return fail("%s: the model's zm is not finite and strictly decreasing", who);
  std::vector<mckpp_vaxis_ent> tab((size_t)nt);
  for (int j = 0; j < nt; ++j) tab[(size_t)j] = mckpp_vaxis_ent{branch[(size_t)j], kin[(size_t)j], t[(size_t)j], dz[(size_t)j]};
  HIPCHK(d.alloc((size_t)nt));
  HIPCHK(hipMemcpy(d, tab.data(), (size_t)nt * sizeof(mckpp_vaxis_ent), hipMemcpyHostToDevice));
  if (keep_branch) *keep_branch = std::move(branch);
  if (keep_kin) *keep_kin = std::move(kin);
  return 0;
}

int vaxis_define(mckpp_hip_ctx *h, const char *who, int axis, int32_t n, const double *z)
{
  if (axis < 0 || axis >= MCKPP_VAXES) return fail("%s: axis %d (0..%d)", who, axis, MCKPP_VAXES - 1);
  if (n < 0 || n == 1 || n > MCKPP_VAXIS_LEVELS_MAX)
    return fail("%s: axis %d: n=%d levels (2..%d, or 0 to drop the axis)", who, axis, n, MCKPP_VAXIS_LEVELS_MAX);
  if (n > 0) {
    if (!z) return fail("%s: axis %d: z is null", who, axis);
    for (int k = 0; k < n; ++k) {
      if (!std::isfinite(z[k])) return fail("%s: axis %d: z[%d] is not finite", who, axis, k);
      if (k > 0 && !(z[k] < z[k - 1]))
        return fail("%s: axis %d: z[%d]=%.17g is not below z[%d]=%.17g: an axis holds heights, strictly decreasing like zm", who,
                    axis, k, z[k], k - 1, z[k - 1]);
    }
  }
  HIPCHK(hipSetDevice(h->device));
  mckpp_hip_ctx::vaxis next;
  if (n > 0) {
    next.z.assign(z, z + n);
    if (vaxis_table(who, n, z, h->nzp1, h->h_zm.data(), next.d_in)) return -1;
    if (vaxis_table(who, h->nzp1, h->h_zm.data(), n, z, next.d_out, &next.out_branch, &next.out_kin)) return -1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));   // (a launch in flight may read the tables this replaces)
  h->vax[axis] = std::move(next);
  return 0;
}

// the axis of planes[k] (or of member `what` of the profiles), defined; null, and the refusal, otherwise
const mckpp_hip_ctx::vaxis *vaxis_of(mckpp_hip_ctx *h, const char *who, const char *what, int axis)
{
  if (axis >= 0 && axis < MCKPP_VAXES && !h->vax[axis].z.empty()) return &h->vax[axis];
  fail("%s: %s: axis %d is not defined (mckpp_hip_vaxis_define; axes are 0..%d)", who, what, axis, MCKPP_VAXES - 1);
  return nullptr;
}

struct vaxis_puts {
  std::vector<mckpp_vaxis_put_plane> tab;
  std::vector<size_t> bytes;   // of each plane's `in`
};

// The planes of a put on caller axes, checked and resolved into the kernel's table: put_resolve's checks, then the axis.
int vaxis_put_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, bool dev_form,
                    vaxis_puts &r, int *dev)
{
  if (uploaded_check(h, who) || planes_count_check(who, nplanes, planes, MCKPP_VAXIS_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r.tab.clear();
  r.bytes.clear();
  int prof[MCKPP_VAXIS_PLANES_MAX];
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_vaxis_put_plane_c &q = planes[k];
    mckpp_vaxis_put_plane e{};
    int row;
    size_t elem;
    if (put_resolve(h, who, k, q.field, 0, h->nzp1, q.dtype, q.op, q.flags, q.skip_value, e.put, &row, &elem)) return -1;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d]", k);
    const mckpp_hip_ctx::vaxis *ax = vaxis_of(h, who, arg, q.axis);
    if (!ax) return -1;
    for (int j = 0; j < k; ++j)
      if (prof[j] == row)
        return fail("%s: planes[%d] and planes[%d] write the same field (%d, %d): a plane writes the whole profile, and the "
                    "planes of a call have no order", who, k, j, q.field, planes[j].field);
    prof[k] = row;
    const size_t bytes = (size_t)h->npts * ax->z.size() * elem;
    snprintf(arg, sizeof arg, "planes[%d].in", k);
    if (!dev_form) {
      if (!q.in) return fail("%s: %s is null", who, arg);
    } else if (dev_ptr_check(h, who, arg, q.in, bytes, k == 0 ? dev : nullptr)) {
      return -1;
    }
    e.put.in = q.in;
    e.skip = e.put.skip;   // decided on the input side, where the values the branch reads are: put_element's own is off
    e.put.skip = 0;
    e.tab = ax->d_in;
    r.tab.push_back(e);
    r.bytes.push_back(bytes);
  }
  return 0;
}

// the table onto the device on the context's stream, a wait for `produced` (null: none), the launch, ev_read behind it
int vaxis_put_queue(mckpp_hip_ctx *h, const std::vector<mckpp_vaxis_put_plane> &tab, hipEvent_t produced)
{
  if (tab.empty() || h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->vput_tab.put(tab, h->stream));
  if (produced) HIPCHK(hipStreamWaitEvent(h->stream, produced, 0));
  HIPCHK(mckpp_launch_vaxis_put_planes(h->vput_tab, (int)tab.size(), h->nzp1, h->d_ipt, h->ncol, h->npts, h->d_cs, h->stream));
  HIPCHK(h->ev_read.record(h->stream));
  return 0;
}

// the host forms: every plane as it is into the context's put staging (each at a multiple of 256 bytes) on the
// context's stream, ahead of the launch that reads it there
int vaxis_stage(mckpp_hip_ctx *h, vaxis_puts &r)
{
  HIPCHK(hipSetDevice(h->device));
  std::vector<size_t> at(r.tab.size());
  size_t total = 0;
  for (size_t k = 0; k < r.tab.size(); ++k) {
    at[k] = total;
    total += (r.bytes[k] + 255) / 256 * 256;
  }
  HIPCHK(h->d_put_stage.reserve(total));   // (every call that read the staging ended with a wait)
  for (size_t k = 0; k < r.tab.size(); ++k) {
    HIPCHK(hipMemcpyAsync(h->d_put_stage + at[k], r.tab[k].put.in, r.bytes[k], hipMemcpyHostToDevice, h->stream));
    r.tab[k].put.in = h->d_put_stage + at[k];
  }
  return 0;
}

int vaxis_put_host_queue(mckpp_hip_ctx *h, vaxis_puts &r)
{
  if (r.tab.empty() || h->ncol == 0) return 0;
  if (vaxis_stage(h, r) || vaxis_put_queue(h, r.tab, nullptr)) return -1;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The profiles of mckpp_hip_vaxis_init_profiles as four planes of k_vaxis_put_planes: plain sets - S as it is
// interpolated, Sref is formed from it afterwards -, U and V into U_init and V_init too, T raising the Kelvin word.
int vaxis_profiles_check(mckpp_hip_ctx *h, const char *who, const mckpp_vaxis_profiles_c *p, bool dev_form, vaxis_puts &r, int *dev)
{
  if (!p) return fail("%s: null argument", who);
  if (h->npts <= 0) return fail("%s: upload the state first", who);
  HIPCHK(hipSetDevice(h->device));
  const size_t elem = p->dtype == MCKPP_EXP_F64 ? sizeof(double) : p->dtype == MCKPP_EXP_F32 ? sizeof(float) : 0;
  if (!elem) return fail("%s: dtype %d (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", who, p->dtype);
  if (!std::isfinite(p->tk0)) return fail("%s: tk0 is not finite", who);
  struct { const char *name; const void *in; int axis, row, row2; } m[4] = {
    {"u", p->u, p->axis_vel, P_U, P_UINIT}, {"v", p->v, p->axis_vel, P_V, P_VINIT},
    {"temp", p->temp, p->axis_temp, P_T, -1}, {"sal", p->sal, p->axis_sal, P_S, -1}};
  r.tab.clear();
  r.bytes.clear();
  for (int k = 0; k < 4; ++k) {
    const mckpp_hip_ctx::vaxis *ax = vaxis_of(h, who, m[k].name, m[k].axis);
    if (!ax) return -1;
    const size_t bytes = (size_t)h->npts * ax->z.size() * elem;
    if (!dev_form) {
      if (!m[k].in) return fail("%s: %s is null", who, m[k].name);
    } else if (dev_ptr_check(h, who, m[k].name, m[k].in, bytes, k == 0 ? dev : nullptr)) {
      return -1;
    }
    mckpp_vaxis_put_plane e{};
    e.put = mckpp_put_plane{m[k].in, h->d_prof[m[k].row].get(), nullptr, nullptr, 0.0, h->ld, 0, h->nzp1,
                            p->dtype == MCKPP_EXP_F32 ? 1 : 0, 0, 0, 0, -1, 0};
    e.tab = ax->d_in;
    e.row2 = m[k].row2 >= 0 ? h->d_prof[m[k].row2].get() : nullptr;
    r.tab.push_back(e);
    r.bytes.push_back(bytes);
  }
  return 0;
}

// first half: the Kelvin word cleared, the four planes written (host form: staged first); *kelvin: the word, read back
int vaxis_profiles_write(mckpp_hip_ctx *h, vaxis_puts &r, bool dev_form, hipEvent_t produced, unsigned *kelvin)
{
  *kelvin = 0;
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (!dev_form && vaxis_stage(h, r)) return -1;
  if (!h->d_kelvin) HIPCHK(h->d_kelvin.alloc(1));
  for (auto &e : r.tab)
    if (e.put.row == h->d_prof[P_T].get()) e.kelvin = h->d_kelvin;   // the temperature plane raises the word
  HIPCHK(hipMemsetAsync(h->d_kelvin, 0, sizeof(unsigned), h->stream));
  if (vaxis_put_queue(h, r.tab, produced)) return -1;
  HIPCHK(hipMemcpyAsync(kelvin, h->d_kelvin, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// second half: the rule for `kelvin` - this context's word, or every shard's combined - and the references; waits
int vaxis_profiles_finish(mckpp_hip_ctx *h, double tk0, unsigned kelvin, bool combined)
{
  if (h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (combined) HIPCHK(hipMemcpyAsync(h->d_kelvin, &kelvin, sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
  HIPCHK(mckpp_launch_vaxis_init_finish(h->d_prof[P_T], h->d_prof[P_S], h->ld, h->nzp1, h->ncol, h->d_cs, h->d_kelvin, tk0,
                                        h->c.L_SSref ? 1 : 0, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the interface-axis fields (src/mckpp_xios_io.F90: 0..nz), which no caller axis of heights like zm describes
const char *vaxis_interface_name(int field)
{
  switch (field) {
    case MCKPP_OUT_WU: return "wu";
    case MCKPP_OUT_WV: return "wv";
    case MCKPP_OUT_WT: return "wT";
    case MCKPP_OUT_WS: return "wS";
    case MCKPP_OUT_WB: return "wB";
    case MCKPP_OUT_WTNT: return "wTnt";
    case MCKPP_OUT_DIFM: return "difm";
    case MCKPP_OUT_DIFT: return "dift";
    case MCKPP_OUT_DIFS: return "difs";
    default: return nullptr;
  }
}

// What planes[k] of a fetch on a caller axis says of its field and its axis, checked - the one statement of it for
// vaxis_fetch_check and for hv_fetch_check (include/mckpp_hip_hv.h).  d: the field on the device; the axis, or null
const mckpp_hip_ctx::vaxis *vaxis_fetch_resolve(mckpp_hip_ctx *h, const char *who, int k, int field, int axis, out_desc &d)
{
  if (field < 0 || field >= MCKPP_OUT_COUNT) return fail("%s: planes[%d]: unknown output field %d", who, k, field), nullptr;
  if (const char *name = vaxis_interface_name(field))
    return fail("%s: planes[%d]: field %d (%s) lives on the interface axis 0..nz, not on the levels zm(1:nzp1) a caller's axis "
                "is interpolated from", who, k, field, name), nullptr;
  if (out_field(h, field, d)) return nullptr;
  if (d.nlev == 1)
    return fail("%s: planes[%d]: field %d%s is two-dimensional: it has no vertical axis to interpolate", who, k, field,
                field == MCKPP_OUT_HMIX ? " (hmix)" : ""), nullptr;
  char arg[32];
  snprintf(arg, sizeof arg, "planes[%d]", k);
  return vaxis_of(h, who, arg, axis);
}

// The planes of a fetch on caller axes, checked and resolved into the kernel's table; *any_fill: a plane fills the land
int vaxis_fetch_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes,
                      std::vector<mckpp_vaxis_fetch_plane> &tab, int *maxlev, bool *any_fill, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_VAXIS_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  tab.clear();
  *maxlev = 0;
  *any_fill = false;
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_vaxis_dev_plane_c &q = planes[k];
    out_desc d;
    const mckpp_hip_ctx::vaxis *ax = vaxis_fetch_resolve(h, who, k, q.field, q.axis, d);
    if (!ax) return -1;
    char arg[32];
    const size_t elem = plane_elem(who, k, q.dtype);
    const int n = (int)ax->z.size();
    snprintf(arg, sizeof arg, "planes[%d].out", k);
    if (!elem || dev_ptr_check(h, who, arg, q.out, (size_t)h->npts * (size_t)n * elem, k == 0 ? dev : nullptr)) return -1;
    tab.push_back(mckpp_vaxis_fetch_plane{mckpp_fetch_plane{d.src, q.out, q.land_value, d.ld, d.off, n, d.add_sref,
                                                            q.dtype == MCKPP_EXP_F32 ? 1 : 0, q.fill_land ? 1 : 0},
                                          ax->d_out});
    *maxlev = std::max(*maxlev, n);
    *any_fill = *any_fill || q.fill_land;
  }
  return 0;
}

int vaxis_fetch_queue(mckpp_hip_ctx *h, const std::vector<mckpp_vaxis_fetch_plane> &tab, int maxlev, bool any_fill,
                      hipEvent_t before, void *consumer_stream)
{
  if (tab.empty()) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->vfetch_tab.put(tab, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(mckpp_launch_vaxis_fetch_planes(h->vfetch_tab, (int)tab.size(), maxlev, h->d_ipt, h->ncol, h->npts, h->d_cs,
                                         any_fill ? h->d_land.get() : nullptr, any_fill ? h->nland : 0, h->stream));
  HIPCHK(h->ev_delivered.record(h->stream));
  HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_delivered, 0));
  return 0;
}

// mckpp_hip_vaxis_put_dev / _put_host: the same planes for every shard, which touches its own columns only
int vaxis_put(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, bool dev_form,
              void *producer_stream)
{
  std::vector<vaxis_puts> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (vaxis_put_check(g.ctx[d], who, nplanes, planes, dev_form, rs[(size_t)d], dev_form ? &dev : nullptr)) return -1;
  if (dev_form) {
    if (dev < 0) return 0;   // (no plane)
    if (caller_event(g, dev, producer_stream)) return -1;
  }
  for (int d = 0; d < g.n; ++d)
    if (dev_form ? vaxis_put_queue(g.ctx[d], rs[(size_t)d].tab, *g.ev) : vaxis_put_host_queue(g.ctx[d], rs[(size_t)d])) return -1;
  return 0;
}

// mckpp_hip_vaxis_init_profiles_dev / _host: every shard writes its columns and reports its Kelvin word; the host
// combines them - the call waits, like the upload it follows - and every shard finishes under the combined word
int vaxis_init_profiles(const ctx_group &g, const char *who, const mckpp_vaxis_profiles_c *p, bool dev_form, void *producer_stream)
{
  std::vector<vaxis_puts> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (vaxis_profiles_check(g.ctx[d], who, p, dev_form, rs[(size_t)d], dev_form ? &dev : nullptr)) return -1;
  if (dev_form && caller_event(g, dev, producer_stream)) return -1;
  unsigned any = 0;
  for (int d = 0; d < g.n; ++d) {
    unsigned kelvin = 0;
    if (vaxis_profiles_write(g.ctx[d], rs[(size_t)d], dev_form, dev_form ? (hipEvent_t)*g.ev : nullptr, &kelvin)) return -1;
    any |= kelvin;
  }
  for (auto *x : g)   // (a lone context's word is on its device already: only a multi handle's is copied back)
    if (vaxis_profiles_finish(x, p->tk0, any, g.kind == 2)) return -1;
  return 0;
}

// mckpp_hip_vaxis_fetch_dev: fetch_dev's order
int vaxis_fetch_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes, void *consumer_stream)
{
  std::vector<std::vector<mckpp_vaxis_fetch_plane>> tabs((size_t)g.n);
  int maxlev = 0, dev = -1;
  bool any_fill = false;
  for (int d = 0; d < g.n; ++d)
    if (vaxis_fetch_check(g.ctx[d], who, nplanes, planes, tabs[(size_t)d], &maxlev, &any_fill, &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  if (any_fill) {
    for (int d = 1; d < g.n; ++d)
      for (auto &e : tabs[(size_t)d]) e.f.fill_land = 0;
    if (group_land(g, who)) return -1;
  }
  if (caller_event(g, dev, consumer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (vaxis_fetch_queue(g.ctx[d], tabs[(size_t)d], maxlev, any_fill && d == 0, *g.ev, consumer_stream)) return -1;
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_vaxis_define(mckpp_hip_handle h, int axis, int32_t n, const double *z)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_define(h, who, axis, n, z); });
}

int mckpp_hip_vaxis_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_put(lone(h), who, nplanes, planes, true, producer_stream); });
}

int mckpp_hip_vaxis_put_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_put(lone(h), who, nplanes, planes, false, nullptr); });
}

int mckpp_hip_vaxis_init_profiles_dev(mckpp_hip_handle h, const mckpp_vaxis_profiles_c *p, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_init_profiles(lone(h), who, p, true, producer_stream); });
}

int mckpp_hip_vaxis_init_profiles_host(mckpp_hip_handle h, const mckpp_vaxis_profiles_c *p)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_init_profiles(lone(h), who, p, false, nullptr); });
}

int mckpp_hip_vaxis_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vaxis_fetch_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

// ---------------------------------------------------------------------------
// The caller's horizontal grids (include/mckpp_hip_hgrid.h): grids and their weight tables per context, forcing in
// through the in table (k_hgrid_fluxes, k_hgrid_flux_gather - queued by fluxes_dev_queue and ring_put_dev_queue, so
// streams, events and ring bookkeeping are those calls'), fields out through the out table (k_fetch_planes into the
// staging plane, then k_hgrid_out).  Checks queue nothing.  The device tables are built from the host's on first use
// (mckpp_host_hgrid_slices) and belong to the resident state.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
using hgrid_dev = mckpp_ctx_resident::hgrid_dev;

int hgrid_copy(const char *who, const char *name, int64_t nrows, int64_t nsrc, const mckpp_hgrid_table_c *t,
               mckpp_hip_ctx::hgrid_csr &c)
{
  if (!t) return 0;
  char msg[256];
  if (mckpp_host_hgrid_check(name, nrows, nsrc, t, msg, (int64_t)sizeof msg)) return fail("%s: %s", who, msg);
  const int64_t nnz = t->ptr[nrows];
  c.ptr.assign(t->ptr, t->ptr + nrows + 1);
  if (nnz > 0) {
    c.idx.assign(t->idx, t->idx + nnz);
    c.w.assign(t->w, t->w + nnz);
  }
  return 0;
}

int hgrid_define(mckpp_hip_ctx *h, const char *who, int grid, int64_t n, const mckpp_hgrid_table_c *in, const mckpp_hgrid_table_c *out)
{
  if (grid < 0 || grid >= MCKPP_HGRIDS) return fail("%s: grid %d (0..%d)", who, grid, MCKPP_HGRIDS - 1);
  if (n < 0 || n > INT32_MAX) return fail("%s: grid %d: n=%lld points (0 drops the grid)", who, grid, (long long)n);
  mckpp_hip_ctx::hgrid next;
  if (n > 0) {
    if (h->npts <= 0) return fail("%s: upload the state first: the tables are checked against the grid's size", who);
    next.n = n;
    next.npts = h->npts;
    if (hgrid_copy(who, "in", h->npts, n, in, next.in)) return -1;
    if (hgrid_copy(who, "out", n, h->npts, out, next.out)) return -1;
  }
  HIPCHK(hipSetDevice(h->device));
  // a launch in flight on the context's stream or on the flux stream may read the device tables of the grid this replaces
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->flux_stream));
  h->hg[grid] = std::move(next);
  h->hgd[grid].in = hgrid_dev{};
  h->hgd[grid].out = hgrid_dev{};
  for (auto &w : h->wsched) w.hout[grid] = hgrid_dev{};   // ... and the listed schedules' out tables on it (mckpp_hip_remap.h)
  return 0;
}

// grid `grid`, defined for the present npts; null, and the refusal naming `what`, otherwise
const mckpp_hip_ctx::hgrid *hgrid_of(mckpp_hip_ctx *h, const char *who, const char *what, int grid)
{
  if (grid < 0 || grid >= MCKPP_HGRIDS || h->hg[grid].n == 0) {
    fail("%s: %s: grid %d is not defined (mckpp_hip_hgrid_define; grids are 0..%d)", who, what, grid, MCKPP_HGRIDS - 1);
    return nullptr;
  }
  if (h->hg[grid].npts != h->npts) {
    fail("%s: %s: grid %d was defined for npts=%lld, the state has %lld: define it again", who, what, grid,
         (long long)h->hg[grid].npts, (long long)h->npts);
    return nullptr;
  }
  return &h->hg[grid];
}

mckpp_hgrid_ell hgrid_ell(const hgrid_dev &d) { return mckpp_hgrid_ell{d.off, d.len, d.idx, d.w, d.nrows}; }

// a device table: list rows rows[0..nlist-1] (null: all) of t, without the entries keep (null: none) does not mark
int hgrid_build(mckpp_hip_ctx *h, hgrid_dev &d, int64_t nlist, const int64_t *rows, const mckpp_hgrid_table_c &t,
                const unsigned char *keep, int kind)
{
  const int64_t nslices = (nlist + 63) / 64;
  std::vector<int64_t> off((size_t)nslices + 1);
  std::vector<int32_t> len((size_t)std::max<int64_t>(nlist, 1));
  const int64_t padded = mckpp_host_hgrid_slices(nlist, rows, &t, keep, off.data(), len.data(), nullptr, nullptr);
  if (padded < 0) return fail("mckpp_host_hgrid_slices: a null argument");
  std::vector<int32_t> idx((size_t)std::max<int64_t>(padded, 1));
  std::vector<double> w((size_t)std::max<int64_t>(padded, 1));
  (void)mckpp_host_hgrid_slices(nlist, rows, &t, keep, off.data(), len.data(), idx.data(), w.data());
  HIPCHK(hipSetDevice(h->device));
  hgrid_dev next;
  HIPCHK(next.off.alloc(off.size()));
  HIPCHK(next.len.alloc(len.size()));
  HIPCHK(next.idx.alloc(idx.size()));
  HIPCHK(next.w.alloc(w.size()));
  HIPCHK(hipMemcpy(next.off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(next.len, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(next.idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(next.w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
  next.nrows = nlist;
  next.padded = padded;
  next.kind = kind;
  for (int64_t j = 0; j < nlist && next.empty_point < 0; ++j)
    if (len[(size_t)j] == 0) next.empty_point = rows ? rows[j] : j;
  if (d.off) {   // a launch in flight on the context's stream or on the flux stream may read the table this replaces
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->flux_stream));
  }
  d = std::move(next);
  return 0;
}

// the in table of the resident columns, built where it is not
int hgrid_in_build(mckpp_hip_ctx *h, int grid)
{
  hgrid_dev &d = h->hgd[grid].in;
  if (d.kind != 0) return 0;
  std::vector<int64_t> rows(h->ipt.begin(), h->ipt.end());
  return hgrid_build(h, d, (int64_t)rows.size(), rows.data(), h->hg[grid].in.view(), nullptr, 1);
}

// the root's out table of `grid` for the points the group holds (kind as d_land's), built where it is not that
int group_hgrid_out(const ctx_group &g, const char *who, int grid)
{
  mckpp_hip_ctx *root = g.root();
  hgrid_dev &d = root->hgd[grid].out;
  if (d.kind == g.kind) return 0;
  std::vector<unsigned char> covered;
  if (group_columns(g, who, covered)) return -1;
  return hgrid_build(root, d, root->hg[grid].n, nullptr, root->hg[grid].out.view(), covered.data(), g.kind);
}

// What a call of the in direction needs before it queues: the grid, its in table, the eight arrays of n doubles, and
// no resident column with an empty row.  *t: the device table; *dev (where asked for): the device of the arrays.
int hgrid_in_check(mckpp_hip_ctx *h, const char *who, int grid, const double *const fields[8], mckpp_hgrid_ell *t, int *dev)
{
  if (!fields) return fail("%s: null argument", who);
  if (h->npts <= 0) return fail("%s: upload the state first", who);
  const mckpp_hip_ctx::hgrid *g = hgrid_of(h, who, "grid", grid);
  if (!g) return -1;
  if (g->in.ptr.empty())
    return fail("%s: grid %d has no in table (caller -> model): mckpp_hip_hgrid_define was given none", who, grid);
  HIPCHK(hipSetDevice(h->device));
  for (int m = 0; m < 8; ++m) {
    char arg[48];
    snprintf(arg, sizeof arg, "fields[%d] (%s)", m, flux_field_names[m]);
    if (dev_ptr_check(h, who, arg, fields[m], (size_t)g->n * sizeof(double), m == 0 ? dev : nullptr)) return -1;
  }
  if (hgrid_in_build(h, grid)) return -1;
  const hgrid_dev &d = h->hgd[grid].in;
  if (d.empty_point >= 0)
    return fail("%s: grid %d: the in row of point %lld, a resident column, is empty: nothing to form its forcing from", who,
                grid, (long long)d.empty_point);
  *t = hgrid_ell(d);
  return 0;
}

// The out planes of a delivery on caller grids - mckpp_hip_hgrid_fetch_dev's, and those of mckpp_hip_remap_records_dev
// (include/mckpp_hip_remap.h).  Stage 1, the call's own, writes the model's values of plane k at[k] doubles into the
// staging block; stage 2 is these planes of k_hgrid_out (stage and table set when they are queued).
struct hgrid_outs {
  std::vector<mckpp_hgrid_plane> second;
  std::vector<int> grid;
  std::vector<size_t> at;
  std::vector<std::pair<const char *, const char *>> span;   // [plane] the bytes of its `out`
  size_t elems = 0;
  int maxlev = 0;
  int64_t maxn = 0;
};

// What planes[k] says of its caller grid and its array, checked and resolved: the grid and its out table, the norm, the
// array (*dev, where asked for: its device), which overlaps no array of a plane before it.  elem: the size of an element.
template <class P>
int hgrid_out_resolve(mckpp_hip_ctx *h, const char *who, int k, const P &q, size_t elem, int *dev, hgrid_outs &r)
{
  char arg[32];
  snprintf(arg, sizeof arg, "planes[%d]", k);
  const mckpp_hip_ctx::hgrid *g = hgrid_of(h, who, arg, q.grid);
  if (!g) return -1;
  if (g->out.ptr.empty())
    return fail("%s: planes[%d]: grid %d has no out table (model -> caller): mckpp_hip_hgrid_define was given none", who, k,
                q.grid);
  if (q.norm != MCKPP_HGRID_NORM_NONE && q.norm != MCKPP_HGRID_NORM_USED)
    return fail("%s: planes[%d]: norm %d (MCKPP_HGRID_NORM_NONE 0, MCKPP_HGRID_NORM_USED 1)", who, k, q.norm);
  const size_t bytes = (size_t)g->n * (size_t)q.nlev * elem;
  snprintf(arg, sizeof arg, "planes[%d].out", k);
  if (dev_ptr_check(h, who, arg, q.out, bytes, dev)) return -1;
  const char *b = static_cast<const char *>(q.out);
  for (int j = 0; j < k; ++j)
    if (b < r.span[(size_t)j].second && r.span[(size_t)j].first < b + bytes)
      return fail("%s: planes[%d].out and planes[%d].out overlap: the planes of a call have no order", who, k, j);
  r.span.emplace_back(b, b + bytes);
  r.second.push_back(mckpp_hgrid_plane{nullptr, q.out, q.land_value, mckpp_hgrid_ell{}, h->npts, q.nlev,
                                       q.dtype == MCKPP_EXP_F32 ? 1 : 0, q.norm, q.fill_land ? 1 : 0});
  r.grid.push_back(q.grid);
  r.at.push_back(r.elems);
  r.elems += (size_t)h->npts * (size_t)q.nlev;
  r.maxlev = std::max(r.maxlev, (int)q.nlev);
  r.maxn = std::max(r.maxn, g->n);
  return 0;
}

// The planes of mckpp_hip_hgrid_fetch_dev: stage 1 as planes of k_fetch_planes (`out` set when it is queued)
struct hgrid_fetch {
  std::vector<mckpp_fetch_plane> first;
  hgrid_outs o;
};

int hgrid_fetch_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_hgrid_plane_c *planes, hgrid_fetch &r, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_HGRID_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = hgrid_fetch{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_hgrid_plane_c &q = planes[k];
    out_desc d;
    if (out_field(h, q.field, d)) return -1;
    if (plane_levels_check(who, k, q.lev0, q.nlev, q.field, d.nlev)) return -1;
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem || hgrid_out_resolve(h, who, k, q, elem, k == 0 ? dev : nullptr, r.o)) return -1;
    r.first.push_back(mckpp_fetch_plane{d.src, nullptr, 0.0, d.ld, d.off + q.lev0, q.nlev, d.add_sref, 0, 0});
  }
  return 0;
}

// the staging block with room for `elems` doubles; whoever regrows it waits first, as ensure_stage does
int hgrid_stage(mckpp_hip_ctx *h, size_t elems)
{
  if (elems <= h->d_hstage.size()) return 0;
  HIPCHK(hipSetDevice(h->device));
  // (both stages of an earlier call, which read and write the block, are on this context's stream)
  if (h->d_hstage) HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(h->d_hstage.reserve(elems));
  return 0;
}

// stage 1 on this context's stream, behind `before`: its columns' values into `stage`
int hgrid_fetch_first(mckpp_hip_ctx *h, hgrid_fetch &r, double *stage, hipEvent_t before)
{
  HIPCHK(hipSetDevice(h->device));
  for (size_t k = 0; k < r.first.size(); ++k) r.first[k].out = stage + r.o.at[k];
  HIPCHK(h->fetch_tab.put(r.first, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(mckpp_launch_fetch_planes(h->fetch_tab, (int)r.first.size(), r.o.maxlev, h->d_ipt, h->ncol, h->npts, h->d_cs, nullptr, 0,
                                   h->stream));
  return 0;
}

// The two-stage delivery of the root's out planes `o`, whose tables are set: first(d, stage, before) queues stage 1 of
// shard d on its stream, behind `before`, into the root's staging block; the root's stage 2 runs behind every shard's
// stage 1, from the staging through the tables, and the consumer waits for it.  dev: the device of the call's first array.
template <class First>
int two_stage_deliver(const ctx_group &g, const char *who, hgrid_outs &o, int dev, void *consumer_stream, First first)
{
  mckpp_hip_ctx *root = g.root();
  if (hgrid_stage(root, o.elems)) return -1;
  double *stage = root->d_hstage;
  for (int d = 1; d < g.n; ++d) {   // every shard's device reaches the root's staging (peer access, once per pair)
    HIPCHK(hipSetDevice(g.ctx[d]->device));
    if (dev_ptr_check(g.ctx[d], who, "the staging plane of shard 0", stage, o.elems * sizeof(double))) return -1;
  }
  if (caller_event(g, dev, consumer_stream)) return -1;
  for (int d = 0; d < g.n; ++d) {
    mckpp_hip_ctx *x = g.ctx[d];
    if (d > 0) {
      HIPCHK(hipSetDevice(x->device));
      // the staging is the root's: behind the second stage of the call before, which read it on the root's stream
      if (root->ev_delivered) HIPCHK(hipStreamWaitEvent(x->stream, root->ev_delivered, 0));
    }
    if (first(d, stage, (hipEvent_t)*g.ev)) return -1;
    if (d > 0) {   // ... and the root's second stage behind this shard's first
      HIPCHK(x->ev_delivered.record(x->stream));
      HIPCHK(hipSetDevice(root->device));
      HIPCHK(hipStreamWaitEvent(root->stream, x->ev_delivered, 0));
    }
  }
  HIPCHK(hipSetDevice(root->device));
  for (size_t k = 0; k < o.second.size(); ++k) o.second[k].stage = stage + o.at[k];
  HIPCHK(root->hgrid_tab.put(o.second, root->stream));
  HIPCHK(mckpp_launch_hgrid_out(root->hgrid_tab, (int)o.second.size(), o.maxlev, o.maxn, root->stream));
  HIPCHK(root->ev_delivered.record(root->stream));
  HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), root->ev_delivered, 0));
  return 0;
}

// mckpp_hip_hgrid_fetch_dev: every shard's first stage into the root's staging, the root's second stage over the points
// the group holds, so the sums of a multi handle are those of one context, entry for entry
int hgrid_fetch_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_hgrid_plane_c *planes, void *consumer_stream)
{
  std::vector<hgrid_fetch> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (hgrid_fetch_check(g.ctx[d], who, nplanes, planes, rs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  hgrid_outs &o = rs[0].o;
  for (int grid : o.grid)
    if (group_hgrid_out(g, who, grid)) return -1;
  for (size_t k = 0; k < o.second.size(); ++k) o.second[k].t = hgrid_ell(g.root()->hgd[o.grid[k]].out);
  return two_stage_deliver(g, who, o, dev, consumer_stream, [&](int d, double *stage, hipEvent_t before) {
    return hgrid_fetch_first(g.ctx[d], rs[(size_t)d], stage, before);
  });
}

int hgrid_info(mckpp_hip_ctx *h, const char *who, int grid, int64_t info[6], bool keep_out_kind)
{
  if (!info) return fail("%s: null argument", who);
  const mckpp_hip_ctx::hgrid *g = hgrid_of(h, who, "grid", grid);
  if (!g) return -1;
  info[0] = g->n;
  info[5] = 0;
  for (int dir = 0; dir < 2; ++dir) {
    const mckpp_hip_ctx::hgrid_csr &c = dir ? g->out : g->in;
    info[1 + dir] = c.ptr.empty() ? -1 : c.ptr.back();
    info[3 + dir] = 0;
    for (size_t r = 0; r + 1 < c.ptr.size(); ++r) info[5] = std::max(info[5], c.ptr[r + 1] - c.ptr[r]);
  }
  if (!g->in.ptr.empty()) {
    if (hgrid_in_build(h, grid)) return -1;
    info[3] = h->hgd[grid].in.padded;
  }
  if (!g->out.ptr.empty()) {
    if (!(keep_out_kind && h->hgd[grid].out.kind == 2) && group_hgrid_out(lone(h), who, grid)) return -1;
    info[4] = h->hgd[grid].out.padded;
  }
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_hgrid_define(mckpp_hip_handle h, int grid, int64_t n, const mckpp_hgrid_table_c *in, const mckpp_hgrid_table_c *out)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return hgrid_define(h, who, grid, n, in, out); });
}

int mckpp_hip_hgrid_info(mckpp_hip_handle h, int grid, int64_t info[6])
{
  return entry(__func__, h, [&, who = __func__]() -> int { return hgrid_info(h, who, grid, info, false); });
}

int mckpp_hip_hgrid_fluxes_dev(mckpp_hip_handle h, int grid, int ntime, const double *const fields[8], int l_rest, double flsn,
                               double el, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  return fluxes_dev(lone(h), who, ntime, fields, l_rest, flsn, el, producer_stream, &grid);
  });
}

int mckpp_hip_hgrid_flux_ring_put_dev(mckpp_hip_handle h, int grid, int rec, const double *const fields[8], void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return flux_ring_put_dev(lone(h), who, rec, fields, producer_stream, &grid); });
}

int mckpp_hip_hgrid_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hgrid_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return hgrid_fetch_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

// ---------------------------------------------------------------------------
// Output windows accumulated inside the step launches (mckpp_hip_window_schedule): k_column_ps samples every field
// of every schedule after each column's step, into the record of the step's window (see mckpp_win_t).  The host
// keeps the bookkeeping: which steps have run under a schedule, so which records are complete, and which are
// released; a launch that would break it fails before anything is launched.
// ---------------------------------------------------------------------------

// the schedule's export goes (nothing of it is in flight: its fetches end with a wait for the transfer stream, and the
// callers have waited for the context's)
static void exp_drop(mckpp_hip_ctx::win_sched &w) { w.ex = mckpp_hip_ctx::win_sched::win_export{}; }

// ... and so does the schedule, its export with it (the callers have waited for the context's stream)
static void win_cancel(mckpp_hip_ctx *h, int s) { h->wsched[s] = mckpp_hip_ctx::win_sched{}; }

static int win_cancel_all(mckpp_hip_ctx *h)
{
  bool any = false;
  for (auto &w : h->wsched) any = any || !w.fields.empty();
  if (!any) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still write the records
  for (int s = 0; s < MCKPP_WIN_SCHEDULES; ++s) win_cancel(h, s);
  h->nwin = 0;
  return 0;
}

// the device table the step launches read: every field of every schedule
static int win_table(mckpp_hip_ctx *h)
{
  std::vector<mckpp_win> t;
  for (auto &w : h->wsched)
    for (size_t i = 0; i < w.fields.size(); ++i) {
      out_desc d;
      if (out_field(h, w.fields[i], d)) return -1;
      mckpp_win e{};
      e.src = d.src; e.acc = w.acc[i]; e.row = w.d_colrow; e.plane = (long long)w.nrow * w.ld_out[i];
      e.ld = d.ld; e.off = d.off + w.lev_off[i]; e.nlev = w.nlev[i]; e.add_sref = d.add_sref; e.ld_out = w.ld_out[i];
      e.ops = (int)w.ops[i]; e.nops = __builtin_popcount(w.ops[i]);
      e.origin = (int)w.origin; e.period = (int)w.period; e.nrec = w.nrec;
      t.push_back(e);
    }
  h->nwin = 0;
  if (t.empty() || h->ncol == 0) return 0;
  if (!h->d_win) HIPCHK(h->d_win.alloc(MCKPP_WIN_ENTRIES));
  HIPCHK(hipMemcpy(h->d_win, t.data(), t.size() * sizeof(mckpp_win), hipMemcpyHostToDevice));
  h->nwin = (int)t.size();
  return 0;
}

// the first record a schedule can complete when its first step is nt0
static int64_t win_first_kept(const mckpp_hip_ctx::win_sched &w, int64_t nt0)
{
  return nt0 <= w.origin ? 0 : (nt0 - w.origin + w.period - 1) / w.period;
}

// the last record all of whose steps have run under the schedule (-1: none)
static int64_t win_last_complete(const mckpp_hip_ctx::win_sched &w)
{
  if (w.next_nt < 0 || w.next_nt < w.origin) return -1;
  return (w.next_nt - w.origin) / w.period - 1;
}

static int win_check_launch(mckpp_hip_ctx *h, int nt0, int nsteps, const char *who)
{
  const int64_t last = (int64_t)nt0 + nsteps - 1;
  for (int s = 0; s < MCKPP_WIN_SCHEDULES; ++s) {
    const auto &w = h->wsched[s];
    if (w.fields.empty()) continue;
    if (w.next_nt >= 0 && nt0 != w.next_nt)
      return fail("%s: steps %d..%lld, but output schedule %d has run up to step %lld: the steps under a schedule follow "
                  "on from one another (the next launch starts at step %lld)", who, nt0, (long long)last, s,
                  (long long)w.next_nt - 1, (long long)w.next_nt);
    for (int f : w.fields)
      if (win_is_diag(f) && !h->diag)
        return fail("%s: output schedule %d has field %d, a diagnostic, and diagnostics are switched off", who, s, f);
    if (last < w.origin) continue;
    const int64_t kept = w.first_nt < 0 ? win_first_kept(w, nt0) : w.first_kept;
    const int64_t wl = (last - w.origin) / w.period;
    if (wl >= kept + w.nrec)
      return fail("%s: steps %d..%lld reach record %lld of output schedule %d (steps %lld..%lld), but its ring of %d "
                  "records holds records %lld..%lld: fetch and release records first", who, nt0, (long long)last,
                  (long long)wl, s, (long long)(w.origin + wl * w.period), (long long)(w.origin + (wl + 1) * w.period - 1),
                  w.nrec, (long long)kept, (long long)(kept + w.nrec - 1));
  }
  return 0;
}

static void win_advance(mckpp_hip_ctx *h, int nt0, int nsteps)
{
  for (auto &w : h->wsched) {
    if (w.fields.empty()) continue;
    if (w.first_nt < 0) { w.first_nt = nt0; w.first_kept = win_first_kept(w, nt0); }
    w.next_nt = (int64_t)nt0 + nsteps;
  }
}

// the levels a field keeps under a level range (znlev 0: the whole axis; a two-dimensional field: its one value)
static void win_levels(int axis, int lev0, int znlev, int &off, int &nlev)
{
  off = 0; nlev = axis;
  if (axis > 1 && znlev > 0) { off = lev0; nlev = znlev; }
}

// A row of a record plane: one double for a single level, else the smallest multiple of 8 doubles (a 64-byte line)
// that holds the levels; an unzoomed schedule keeps the rows of the state, ld doubles.
static int win_ld_out(const mckpp_hip_ctx *h, bool zoomed, int nlev)
{
  return nlev == 1 ? 1 : zoomed ? (nlev + 7) / 8 * 8 : h->ld;
}

// The body of mckpp_hip_window_schedule and mckpp_hip_window_schedule_zoom: a schedule is set here and nowhere else.
static int win_set(mckpp_hip_ctx *h, const char *who, int sched, int nt_origin, int period, int nrec, const int32_t *fields,
                   const uint32_t *ops, int32_t nfields, const mckpp_win_zoom_c *zoom)
{
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  if (nfields < 0 || (nfields > 0 && (!fields || !ops))) return fail("%s: bad argument (nfields=%d)", who, nfields);
  std::vector<int> colrow, rowpos, norow;   // of a point list
  if (nfields > 0) {   // everything is checked before the schedule in place is touched
    if (nt_origin < 1 || period < 1 || nrec < 1)
      return fail("%s: nt_origin=%d period=%d nrec=%d (each at least 1)", who, nt_origin, period, nrec);
    if (h->npts <= 0) return fail("%s: upload the state first (the records are sized to the resident columns)", who);
    int others = 0;
    for (int s = 0; s < MCKPP_WIN_SCHEDULES; ++s) if (s != sched) others += (int)h->wsched[s].fields.size();
    if (others + nfields > MCKPP_WIN_ENTRIES)
      return fail("%s: %d fields, and the other schedules hold %d: at most %d in all", who, nfields, others, MCKPP_WIN_ENTRIES);
    for (int i = 0; i < nfields; ++i) {
      const int f = fields[i];
      if (f < 0 || f >= MCKPP_OUT_COUNT) return fail("%s: unknown output field %d", who, f);
      if (ops[i] == 0 || (ops[i] & ~0xFu))
        return fail("%s: field %d: operations 0x%x (a non-empty mask of MCKPP_WIN_MEAN 1, _MIN 2, _MAX 4, _LAST 8)", who, f, ops[i]);
      for (int j = 0; j < i; ++j)
        if (fields[j] == f) return fail("%s: field %d twice in one schedule", who, f);
      out_desc d;
      if (out_field(h, f, d)) return -1;   // (the message of window_accumulate: a correction field without the rows)
      if (win_is_diag(f) && !h->diag) return fail("%s: field %d is a diagnostic, and diagnostics are switched off", who, f);
    }
    if (zoom) {
      if (zoom->nlev < 0 || zoom->lev0 < 0 || (int64_t)zoom->lev0 + zoom->nlev > h->nzp1 || (zoom->nlev == 0 && zoom->lev0 != 0))
        return fail("%s: zoom: levels lev0=%d nlev=%d (a range within 0..%d; 0, 0: the whole axis)", who, zoom->lev0, zoom->nlev, h->nzp1);
      if (zoom->points) {
        if (zoom->npoints < 1) return fail("%s: zoom: npoints=%lld with a point list (at least 1)", who, (long long)zoom->npoints);
        std::vector<int64_t> at((size_t)h->npts, -1);   // point -> its position in the list
        for (int64_t i = 0; i < zoom->npoints; ++i) {
          const int64_t pt = zoom->points[i];
          if (pt < 0 || pt >= h->npts)
            return fail("%s: zoom: point %lld at position %lld is outside 0..%lld", who, (long long)pt, (long long)i, (long long)h->npts - 1);
          if (at[(size_t)pt] >= 0)
            return fail("%s: zoom: point %lld twice, at positions %lld and %lld", who, (long long)pt, (long long)at[(size_t)pt], (long long)i);
          at[(size_t)pt] = i;
        }
        // rows in list order: the listed points that are resident columns
        std::vector<int> colof((size_t)h->npts, -1);
        for (int64_t c = 0; c < h->ncol; ++c) colof[(size_t)h->ipt[(size_t)c]] = (int)c;
        colrow.assign((size_t)h->ncol, -1);
        for (int64_t i = 0; i < zoom->npoints; ++i) {
          const int c = colof[(size_t)zoom->points[i]];
          if (c < 0) { norow.push_back((int)i); continue; }
          colrow[(size_t)c] = (int)rowpos.size();
          rowpos.push_back((int)i);
        }
      }
    }
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));   // no launch in flight may still read the table or write the records
  win_cancel(h, sched);
  if (nfields > 0) {
    mckpp_hip_ctx::win_sched w;   // built here, moved in when every ring is there
    w.origin = nt_origin; w.period = period; w.nrec = nrec;
    w.zoomed = zoom != nullptr;
    w.listed = zoom && zoom->points;
    w.npoints = w.listed ? zoom->npoints : h->npts;
    w.nrow = w.listed ? (int64_t)rowpos.size() : h->ncol;
    if (zoom) { w.lev0 = zoom->lev0; w.znlev = zoom->nlev; }
    hipError_t e = hipSuccess;
    size_t bytes = 0;
    int failed = -1;
    if (w.listed && h->ncol > 0) {
      bytes = (colrow.size() + rowpos.size()) * sizeof(int);
      e = w.d_colrow.alloc(colrow.size());
      if (e == hipSuccess) e = hipMemcpy(w.d_colrow, colrow.data(), colrow.size() * sizeof(int), hipMemcpyHostToDevice);
      if (e == hipSuccess && w.nrow > 0) e = w.d_rowpos.alloc(rowpos.size());
      if (e == hipSuccess && w.nrow > 0) e = hipMemcpy(w.d_rowpos, rowpos.data(), rowpos.size() * sizeof(int), hipMemcpyHostToDevice);
      std::vector<int> rowpt;
      for (int p : rowpos) rowpt.push_back(zoom->points[p]);
      bytes += rowpt.size() * sizeof(int);
      if (e == hipSuccess && w.nrow > 0) e = w.d_rowpt.alloc(rowpt.size());
      if (e == hipSuccess && w.nrow > 0) e = hipMemcpy(w.d_rowpt, rowpt.data(), rowpt.size() * sizeof(int), hipMemcpyHostToDevice);
      w.rowpt = std::move(rowpt);
    }
    if (e == hipSuccess && !norow.empty()) {
      bytes += norow.size() * sizeof(int);
      e = w.d_norow.alloc(norow.size());
      if (e == hipSuccess) e = hipMemcpy(w.d_norow, norow.data(), norow.size() * sizeof(int), hipMemcpyHostToDevice);
    }
    w.nnorow = (int64_t)norow.size();
    w.rowpos = std::move(rowpos);
    for (int i = 0; i < nfields && e == hipSuccess; ++i) {
      out_desc d;
      out_field(h, fields[i], d);
      int off = 0, nlev = 0;
      win_levels(d.nlev, w.lev0, w.znlev, off, nlev);
      const int ld_out = win_ld_out(h, w.zoomed, nlev);
      const size_t elems = (size_t)nrec * (size_t)__builtin_popcount(ops[i]) * (size_t)w.nrow * (size_t)ld_out;
      bytes = elems * sizeof(double);
      dev_buf<double> p;
      if (bytes > 0) e = p.alloc(elems);
      if (e != hipSuccess) failed = fields[i];
      w.fields.push_back(fields[i]); w.ops.push_back(ops[i]); w.ld_out.push_back(ld_out); w.acc.push_back(std::move(p));
      w.nlev.push_back(nlev); w.lev_off.push_back(off);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      win_table(h);   // (of the other schedules)
      if (failed < 0)
        return fail("%s: cannot set up the %zu bytes of the zoom's tables on the device (%s); the schedule is not set", who, bytes,
                    hipGetErrorString(e));
      return fail("%s: cannot allocate %zu bytes of device memory for the %d records of field %d (%s); the schedule is "
                  "not set", who, bytes, nrec, failed, hipGetErrorString(e));
    }
    h->wsched[sched] = std::move(w);
  }
  return win_table(h);
}

int mckpp_hip_window_schedule(mckpp_hip_handle h, int sched, int nt_origin, int period, int nrec, const int32_t *fields,
                              const uint32_t *ops, int32_t nfields)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  return win_set(h, who, sched, nt_origin, period, nrec, fields, ops, nfields, nullptr);
  });
}

int mckpp_hip_window_schedule_zoom(mckpp_hip_handle h, int sched, int nt_origin, int period, int nrec, const int32_t *fields,
                                   const uint32_t *ops, int32_t nfields, const mckpp_win_zoom_c *zoom)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  return win_set(h, who, sched, nt_origin, period, nrec, fields, ops, nfields, zoom);
  });
}

// the device bytes of a schedule's record ring (without its export and without the small tables of a point list)
static int64_t win_ring_bytes(const mckpp_hip_ctx::win_sched &w)
{
  int64_t b = 0;
  for (size_t i = 0; i < w.fields.size(); ++i)
    b += (int64_t)w.nrec * __builtin_popcount(w.ops[i]) * w.nrow * w.ld_out[i] * (int64_t)sizeof(double);
  return b;
}

int mckpp_hip_window_zoom(mckpp_hip_handle h, int sched, int64_t *npoints, int32_t *lev0, int32_t *nlev, int64_t *ring_bytes)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  const auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  if (npoints) *npoints = w.npoints;
  if (lev0) *lev0 = w.znlev > 0 ? w.lev0 : 0;
  if (nlev) *nlev = w.znlev > 0 ? w.znlev : h->nzp1;
  if (ring_bytes) *ring_bytes = win_ring_bytes(w);
  return 0;
  });
}

// XIOS zoom_domain: the box ibegin .. ibegin + ni - 1, jbegin .. jbegin + nj - 1 (0-based) of an nx x ny grid as point
// numbers of the 3-D ordering, i fastest: ni * nj of them
int mckpp_host_zoom_box(int64_t nx, int64_t ny, int64_t ibegin, int64_t ni, int64_t jbegin, int64_t nj, int32_t *points)
{
  return entry(__func__, [&, who = __func__]() -> int {
  if (!points) return fail("%s: null argument", who);
  if (nx < 1 || ny < 1 || nx * ny > INT32_MAX) return fail("%s: grid %lld x %lld", who, (long long)nx, (long long)ny);
  if (ni < 1 || nj < 1 || ibegin < 0 || jbegin < 0 || ibegin + ni > nx || jbegin + nj > ny)
    return fail("%s: box i %lld..%lld, j %lld..%lld is not within the grid of %lld x %lld points", who, (long long)ibegin,
                (long long)(ibegin + ni - 1), (long long)jbegin, (long long)(jbegin + nj - 1), (long long)nx, (long long)ny);
  int64_t n = 0;
  for (int64_t j = jbegin; j < jbegin + nj; ++j)
    for (int64_t i = ibegin; i < ibegin + ni; ++i) points[n++] = (int32_t)(j * nx + i);
  return 0;
  });
}

// row -> position on the record's point axis: on the device, and on the host
static const int *win_map(const mckpp_hip_ctx *h, const mckpp_hip_ctx::win_sched &w) { return w.listed ? w.d_rowpos.get() : h->d_ipt.get(); }
static const std::vector<int> &win_host_map(const mckpp_hip_ctx *h, const mckpp_hip_ctx::win_sched &w) { return w.listed ? w.rowpos : h->ipt; }

// the rows [nrow][ld_out] of operation `op` of field i of the schedule in the ring slot of record `rec` (no row: null)
static const double *win_plane_rows(const mckpp_hip_ctx::win_sched &w, size_t i, int64_t rec, int op)
{
  const size_t nops = (size_t)__builtin_popcount(w.ops[i]), j = (size_t)__builtin_popcount(w.ops[i] & ((1u << op) - 1u));
  const size_t n = (size_t)w.nrow * (size_t)w.ld_out[i];
  return w.nrow > 0 ? w.acc[i] + ((size_t)(rec % w.nrec) * nops + j) * n : nullptr;
}

// may record `rec` of the schedule be fetched - all of it (plane false), or its plane of `field` and `op`, whose index
// among the schedule's fields comes back in *fi?  Otherwise an error that names the record's steps.
static int win_record_check(mckpp_hip_ctx *h, const char *who, int sched, int64_t rec, bool plane, int field, int op, size_t *fi)
{
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  const auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  size_t i = 0;
  if (plane) {
    if (op < 0 || op > 3) return fail("%s: op %d (0 mean, 1 min, 2 max, 3 last)", who, op);
    while (i < w.fields.size() && w.fields[i] != field) ++i;
    if (i == w.fields.size()) return fail("%s: field %d is not in schedule %d", who, field, sched);
    if (!((w.ops[i] >> op) & 1u)) return fail("%s: schedule %d keeps no op %d of field %d (operations 0x%x)", who, sched, op, field, w.ops[i]);
  }
  if (fi) *fi = i;
  if (rec < 0) return fail("%s: record %lld", who, (long long)rec);
  const long long a = w.origin + rec * w.period, b = a + w.period - 1;
  if (w.first_nt >= 0 && a < w.first_nt)
    return fail("%s: record %lld of schedule %d (steps %lld..%lld) is incomplete: its first steps ran before the schedule "
                "was set (its first step was %lld)", who, (long long)rec, sched, a, b, (long long)w.first_nt);
  if (rec < w.first_kept) return fail("%s: record %lld of schedule %d (steps %lld..%lld) has been released", who, (long long)rec, sched, a, b);
  if (w.next_nt < 0 || b >= w.next_nt)
    return fail("%s: record %lld of schedule %d (steps %lld..%lld) is incomplete: steps have run up to %lld", who,
                (long long)rec, sched, a, b, (long long)(w.next_nt < 0 ? w.origin - 1 : w.next_nt - 1));
  return 0;
}

// the record's plane of one field and operation on the device (the mean formed into the staging buffer), or an error
// that names the record's steps
static int win_record(mckpp_hip_ctx *h, const char *who, int sched, int64_t rec, int field, int op,
                      const double **src_out, int *ld_out, int *nlev)
{
  size_t i = 0;
  if (win_record_check(h, who, sched, rec, true, field, op, &i)) return -1;
  const auto &w = h->wsched[sched];
  out_desc d;
  if (out_field(h, field, d)) return -1;
  *ld_out = w.ld_out[i];
  *nlev = w.nlev[i];
  *src_out = nullptr;
  if (w.nrow == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  const size_t n = (size_t)w.nrow * w.ld_out[i];
  const double *src = win_plane_rows(w, i, rec, op);
  if (op == 0) {   // the mean: window_fetch's sum / count, the count a whole window's
    if (ensure_stage(h, n)) return -1;
    HIPCHK(mckpp_launch_window_mean(src, h->d_stage, n, (double)w.period, h->stream));
    src = h->d_stage;
  }
  *src_out = src;
  return 0;
}

int mckpp_hip_window_record_fetch(mckpp_hip_handle h, int sched, int64_t rec, int field, int op, double *out)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!out) return fail("%s: null argument", who);
  const double *src = nullptr;
  int ld_out = 0, nlev = 0;
  if (win_record(h, who, sched, rec, field, op, &src, &ld_out, &nlev)) return -1;
  const auto &w = h->wsched[sched];
  if (w.nrow == 0) return 0;   // (no listed point is a resident column: `out` stays as it is)
  if (down_rows_map(h, src, ld_out, 0, nlev, out, win_map(h, w), w.nrow, w.npoints)) return -1;
  return xfer_finish(h);
  });
}

int mckpp_hip_window_record_release(mckpp_hip_handle h, int sched, int64_t upto_rec)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  const int64_t lc = win_last_complete(w);
  if (upto_rec > lc)
    return fail("%s: record %lld of schedule %d (steps %lld..%lld) is not complete (complete are up to record %lld)", who,
                (long long)upto_rec, sched, (long long)(w.origin + upto_rec * w.period),
                (long long)(w.origin + (upto_rec + 1) * w.period - 1), (long long)lc);
  if (upto_rec + 1 > w.first_kept) w.first_kept = upto_rec + 1;
  return 0;
  });
}

int mckpp_hip_window_records(mckpp_hip_handle h, int sched, int64_t *first_kept, int64_t *last_complete)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  const auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  if (first_kept) *first_kept = w.first_kept;
  if (last_complete) *last_complete = win_last_complete(w);
  return 0;
  });
}

// ---------------------------------------------------------------------------
// Records into the caller's device arrays (include/mckpp_hip_device_records.h): a check, which queues nothing, and a
// part that queues in fetch_dev_queue's order; a multi handle checks all its shards before any of them queues.  The
// mean is formed by the delivery's kernel (k_record_planes), not through d_stage: nothing here waits for the device.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
// the planes of a delivery resolved into the kernel's table, but for their non-row lists; [plane] its schedule
struct rec_planes {
  std::vector<mckpp_rec_plane> tab;
  std::vector<int> sched;
  int maxlev = 0;
};

// planes[k] of a call that names a plane of a completed record (schedule, record, field, operation, levels): may it be
// fetched, are its levels among those the schedule keeps?  Resolved into what the kernels' entries of such a plane
// share, mckpp_rec_plane's and mckpp_red_plane's; *fi: the field's index in the schedule.  The schedule, or null and the
// refusal.
template <class P, class E>
const mckpp_hip_ctx::win_sched *record_plane(mckpp_hip_ctx *h, const char *who, int k, const P &q, E &e, size_t *fi = nullptr)
{
  char at[96];
  snprintf(at, sizeof at, "%s: planes[%d]", who, k);
  size_t i = 0;
  if (win_record_check(h, at, q.sched, q.rec, true, q.field, q.op, &i)) return nullptr;
  const auto &w = h->wsched[q.sched];
  if (plane_levels_check(who, k, q.lev0, q.nlev, q.field, w.nlev[i], q.sched)) return nullptr;
  e.src = win_plane_rows(w, i, q.rec, q.op);
  e.period = (double)w.period;
  e.nrow = w.nrow;
  e.ld = w.ld_out[i]; e.off = q.lev0; e.nlev = q.nlev;
  e.mean = q.op == 0;
  if (fi) *fi = i;
  return &w;
}

int records_dev_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_dev_record_plane_c *planes, rec_planes &r,
                      int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_DEV_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = rec_planes{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_dev_record_plane_c &q = planes[k];
    mckpp_rec_plane e{};
    const auto *w = record_plane(h, who, k, q, e);
    if (!w) return -1;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d].out", k);
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem || dev_ptr_check(h, who, arg, q.out, (size_t)w->npoints * (size_t)q.nlev * elem, k == 0 ? dev : nullptr)) return -1;
    e.out = q.out;
    e.map = win_map(h, *w);
    e.land_value = q.land_value;
    e.npoints = w->npoints;
    e.f32 = q.dtype == MCKPP_EXP_F32; e.fill = q.fill_land != 0;
    r.tab.push_back(e);
    r.sched.push_back(q.sched);
    r.maxlev = std::max(r.maxlev, (int)q.nlev);
  }
  return 0;
}

// the root's list of the positions of schedule `sched`'s point axis that the group has no row for - the grid's land
// list, or the point list's own (win_sched::d_norow) -, where it is not that already
int group_norow(const ctx_group &g, const char *who, int sched)
{
  mckpp_hip_ctx *root = g.root();
  auto &w = root->wsched[sched];
  if (!w.listed) return group_land(g, who);
  if (w.norow_kind == g.kind) return 0;
  std::vector<unsigned char> held((size_t)w.npoints, 0);
  for (auto *x : g)
    for (int p : x->wsched[sched].rowpos) held[(size_t)p] = 1;
  return fill_list_set(root, w.d_norow, w.nnorow, w.norow_kind, held, g.kind);
}

// The non-row list of plane `e` of schedule `sched`, stated once for the deliveries at a record's points (k_record_planes,
// k_vaxis_record_planes).  fill: this context writes the land values the planes ask for (the root does, from the lists
// group_norow has brought up to date; another shard of a multi handle writes none).  The plane's 64-entry tiles, rows and
// - where it fills - non-row positions together.
int64_t rec_plane_fill(mckpp_hip_ctx *h, mckpp_rec_plane &e, int sched, bool fill)
{
  const auto &w = h->wsched[sched];
  e.fill = e.fill && fill;
  if (e.fill && w.listed) { e.norow = w.d_norow; e.nnorow = w.nnorow; }
  else if (e.fill) { e.norow = h->d_land; e.nnorow = h->nland; }
  return (e.nrow + 63) / 64 + (e.nnorow + 63) / 64;
}

int records_dev_queue(mckpp_hip_ctx *h, rec_planes &r, bool fill, hipEvent_t before, void *consumer_stream)
{
  if (r.tab.empty()) return 0;
  HIPCHK(hipSetDevice(h->device));
  int64_t xtiles = 0;
  for (size_t k = 0; k < r.tab.size(); ++k) xtiles = std::max(xtiles, rec_plane_fill(h, r.tab[k], r.sched[k], fill));
  HIPCHK(h->rec_tab.put(r.tab, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(mckpp_launch_record_planes(h->rec_tab, (int)r.tab.size(), r.maxlev, xtiles, h->stream));
  HIPCHK(h->ev_delivered.record(h->stream));
  HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_delivered, 0));
  return 0;
}

// mckpp_hip_records_dev: a shard writes its own rows of every plane, the root the land values - at the grid points, or
// the positions of a schedule's point list, that the group has no row for
int records_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_dev_record_plane_c *planes, void *consumer_stream)
{
  std::vector<rec_planes> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (records_dev_check(g.ctx[d], who, nplanes, planes, rs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  const rec_planes &r0 = rs[0];
  for (size_t k = 0; k < r0.tab.size(); ++k)
    if (r0.tab[k].fill && group_norow(g, who, r0.sched[k])) return -1;
  if (caller_event(g, dev, consumer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (records_dev_queue(g.ctx[d], rs[(size_t)d], d == 0, *g.ev, consumer_stream)) return -1;
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_records_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_dev_record_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return records_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

// ---------------------------------------------------------------------------
// The caller's horizontal grids, second half (include/mckpp_hip_remap.h): a completed record's planes out through the
// out table, U, V, T, S in through the in table.  Both are the existing calls' parts put together: a record plane is
// resolved by what resolves a plane of mckpp_hip_records_dev and a grid by what mckpp_hip_hgrid_fetch_dev uses, stage 1
// is k_record_planes into the hgrid staging (by point number, no fill), stage 2 k_hgrid_out; a put plane is resolved by
// put_resolve and queued in put_queue's order, with k_remap_put_planes as the launch.  Checks queue nothing.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
// The planes of a delivery of records on caller grids: stage 1 as planes of its kernel (`out` set when it is queued),
// [plane] its schedule.  mckpp_hip_remap_records_dev's stage 1 is k_record_planes, mckpp_hip_vrecords_hv_dev's
// (include/mckpp_hip_vrecords.h) k_vaxis_record_planes; what differs between the two is stated by the overloads below.
template <class Plane>
struct grid_recs {
  std::vector<Plane> first;
  std::vector<int> sched;
  hgrid_outs o;
};
using remap_recs = grid_recs<mckpp_rec_plane>;
using hv_recs = grid_recs<mckpp_vrec_plane>;

// a stage-1 plane's rows and geometry; its table onto the device and its launch, on the context's stream
mckpp_rec_plane &rows_of(mckpp_rec_plane &e) { return e; }
mckpp_rec_plane &rows_of(mckpp_vrec_plane &e) { return e.r; }
hipError_t rows_put(mckpp_hip_ctx *h, const std::vector<mckpp_rec_plane> &t) { return h->rec_tab.put(t, h->stream); }
hipError_t rows_put(mckpp_hip_ctx *h, const std::vector<mckpp_vrec_plane> &t) { return h->vrec_tab.put(t, h->stream); }
hipError_t rows_launch(mckpp_hip_ctx *h, const std::vector<mckpp_rec_plane> &t, int maxlev, int64_t xtiles)
{
  return mckpp_launch_record_planes(h->rec_tab, (int)t.size(), maxlev, xtiles, h->stream);
}
hipError_t rows_launch(mckpp_hip_ctx *h, const std::vector<mckpp_vrec_plane> &t, int maxlev, int64_t xtiles)
{
  return mckpp_launch_vaxis_record_planes(h->vrec_tab, (int)t.size(), maxlev, xtiles, h->stream);
}

int remap_records_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_remap_record_plane_c *planes, remap_recs &r,
                        int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_REMAP_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = remap_recs{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_remap_record_plane_c &q = planes[k];
    mckpp_rec_plane e{};   // into the staging by point number; what is no row is never written and never read
    const auto *w = record_plane(h, who, k, q, e);
    if (!w) return -1;
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem || hgrid_out_resolve(h, who, k, q, elem, k == 0 ? dev : nullptr, r.o)) return -1;
    e.map = w->listed ? w->d_rowpt.get() : h->d_ipt.get();
    e.npoints = h->npts;
    r.first.push_back(e);
    r.sched.push_back(q.sched);
  }
  return 0;
}

// the table stage 2 reads for a plane of schedule `sched` on grid `grid`: a listed schedule's own on the grid, else the
// grid's
hgrid_dev &remap_out_table(mckpp_hip_ctx *h, int sched, int grid)
{
  auto &w = h->wsched[sched];
  return w.listed ? w.hout[grid] : h->hgd[grid].out;
}

// the root's out table for a plane of a delivery, for the rows the group holds of the plane's schedule (kind as
// group_hgrid_out's), built where it is not that
int group_remap_out(const ctx_group &g, const char *who, int sched, int grid)
{
  mckpp_hip_ctx *root = g.root();
  if (!root->wsched[sched].listed) return group_hgrid_out(g, who, grid);
  hgrid_dev &d = remap_out_table(root, sched, grid);
  if (d.kind == g.kind) return 0;
  std::vector<unsigned char> covered((size_t)root->npts, 0);
  for (auto *x : g)
    for (int p : x->wsched[sched].rowpt) covered[(size_t)p] = 1;
  return hgrid_build(root, d, root->hg[grid].n, nullptr, root->hg[grid].out.view(), covered.data(), g.kind);
}

// stage 1 on this context's stream, behind `before`: its rows' values into `stage`
template <class Plane>
int grid_records_first(mckpp_hip_ctx *h, grid_recs<Plane> &r, double *stage, hipEvent_t before)
{
  HIPCHK(hipSetDevice(h->device));
  int64_t xtiles = 0;
  for (size_t k = 0; k < r.first.size(); ++k) {
    rows_of(r.first[k]).out = stage + r.o.at[k];
    xtiles = std::max<int64_t>(xtiles, (rows_of(r.first[k]).nrow + 63) / 64);
  }
  HIPCHK(rows_put(h, r.first));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(rows_launch(h, r.first, r.o.maxlev, xtiles));
  return 0;
}

// Records onto caller grids, whatever the first stage: hgrid_fetch_dev's order - every shard's rows into the root's
// staging, the root's second stage behind them, through tables whose used entries are the rows of any shard.
// check(h, r, dev): the planes of the call checked and resolved for context h.
template <class Plane, class Check>
int grid_records_dev(const ctx_group &g, const char *who, void *consumer_stream, Check check)
{
  std::vector<grid_recs<Plane>> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (check(g.ctx[d], rs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  grid_recs<Plane> &r0 = rs[0];
  for (size_t k = 0; k < r0.first.size(); ++k)
    if (group_remap_out(g, who, r0.sched[k], r0.o.grid[k])) return -1;
  for (size_t k = 0; k < r0.first.size(); ++k) r0.o.second[k].t = hgrid_ell(remap_out_table(g.root(), r0.sched[k], r0.o.grid[k]));
  return two_stage_deliver(g, who, r0.o, dev, consumer_stream, [&](int d, double *stage, hipEvent_t before) {
    return grid_records_first(g.ctx[d], rs[(size_t)d], stage, before);
  });
}

// mckpp_hip_remap_records_dev
int remap_records_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_remap_record_plane_c *planes,
                      void *consumer_stream)
{
  return grid_records_dev<mckpp_rec_plane>(g, who, consumer_stream, [&](mckpp_hip_ctx *h, remap_recs &r, int *dev) {
    return remap_records_check(h, who, nplanes, planes, r, dev);
  });
}

struct remap_puts {
  std::vector<mckpp_remap_put_plane> tab;
  int maxlev = 0;
};

// The planes of a put on caller grids, checked and resolved into the kernel's table (the device tables `t` set when it
// is queued): put_resolve's checks and put_check's overlap rule, then the grid and its in table.
int remap_put_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_remap_put_plane_c *planes, remap_puts &r, int *dev)
{
  if (uploaded_check(h, who) || planes_count_check(who, nplanes, planes, MCKPP_REMAP_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = remap_puts{};
  int prof[MCKPP_REMAP_PLANES_MAX];
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_remap_put_plane_c &q = planes[k];
    mckpp_remap_put_plane e{};
    int row;
    size_t elem;
    if (put_resolve(h, who, k, q.field, q.lev0, q.nlev, q.dtype, q.op, q.flags, q.skip_value, e.put, &row, &elem)) return -1;
    if (put_overlap_check(who, k, planes, prof, row)) return -1;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d]", k);
    const mckpp_hip_ctx::hgrid *g = hgrid_of(h, who, arg, q.grid);
    if (!g) return -1;
    if (g->in.ptr.empty())
      return fail("%s: planes[%d]: grid %d has no in table (caller -> model): mckpp_hip_hgrid_define was given none", who, k,
                  q.grid);
    snprintf(arg, sizeof arg, "planes[%d].in", k);
    if (dev_ptr_check(h, who, arg, q.in, (size_t)g->n * (size_t)q.nlev * elem, k == 0 ? dev : nullptr)) return -1;
    e.put.in = q.in;
    e.skip = e.put.skip;   // decided on the input side, where the values the entries read are: put_element's own is off
    e.put.skip = 0;
    e.n = g->n;
    if (hgrid_in_build(h, q.grid)) return -1;   // (on first use, as hgrid_in_check does; an empty row is no refusal here)
    e.t = hgrid_ell(h->hgd[q.grid].in);
    r.tab.push_back(e);
    r.maxlev = std::max(r.maxlev, (int)q.nlev);
  }
  return 0;
}

// put_queue's order with the remap's launch
int remap_put_queue(mckpp_hip_ctx *h, const remap_puts &r, hipEvent_t produced)
{
  if (r.tab.empty() || h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->rput_tab.put(r.tab, h->stream));
  if (produced) HIPCHK(hipStreamWaitEvent(h->stream, produced, 0));
  HIPCHK(mckpp_launch_remap_put_planes(h->rput_tab, (int)r.tab.size(), r.maxlev, h->ncol, h->d_cs, h->stream));
  HIPCHK(h->ev_read.record(h->stream));
  return 0;
}

// mckpp_hip_remap_put_dev: put_planes' order, every shard through its own in table
int remap_put_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_remap_put_plane_c *planes, void *producer_stream)
{
  std::vector<remap_puts> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (remap_put_check(g.ctx[d], who, nplanes, planes, rs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  if (caller_event(g, dev, producer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (remap_put_queue(g.ctx[d], rs[(size_t)d], *g.ev)) return -1;
  return 0;
}

// ---------------------------------------------------------------------------
// A caller grid and a caller axis in one call (include/mckpp_hip_hv.h), the parts above put together.  Fields out: a
// plane's field and axis are resolved by vaxis_fetch_resolve and its grid, norm and array by hgrid_out_resolve, with the
// axis's n as the plane's levels; stage 1 is k_vaxis_fetch_planes into the hgrid staging (doubles, no land fill), stage 2
// k_hgrid_out through two_stage_deliver.  State in: put_resolve over the whole profile and vaxis_put_check's rules of
// axis and planes, remap_put_check's of grid and array; put_queue's order with k_hv_put_planes as the launch.
// ---------------------------------------------------------------------------
struct hv_fetch {
  std::vector<mckpp_vaxis_fetch_plane> first;   // (`f.out` set when it is queued)
  hgrid_outs o;
};

int hv_fetch_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_hv_plane_c *planes, hv_fetch &r, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_HV_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = hv_fetch{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_hv_plane_c &q = planes[k];
    out_desc d;
    const mckpp_hip_ctx::vaxis *ax = vaxis_fetch_resolve(h, who, k, q.field, q.axis, d);
    if (!ax) return -1;
    const int n = (int)ax->z.size();
    // the plane as hgrid_out_resolve reads one: its levels are the caller axis'
    const struct { int32_t grid, norm, nlev, dtype, fill_land; double land_value; void *out; } v{
        q.grid, q.norm, n, q.dtype, q.fill_land, q.land_value, q.out};
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem || hgrid_out_resolve(h, who, k, v, elem, k == 0 ? dev : nullptr, r.o)) return -1;
    r.first.push_back(mckpp_vaxis_fetch_plane{mckpp_fetch_plane{d.src, nullptr, 0.0, d.ld, d.off, n, d.add_sref, 0, 0}, ax->d_out});
  }
  return 0;
}

// stage 1 on this context's stream, behind `before`: its columns' profiles on the caller's levels into `stage`
int hv_fetch_first(mckpp_hip_ctx *h, hv_fetch &r, double *stage, hipEvent_t before)
{
  HIPCHK(hipSetDevice(h->device));
  for (size_t k = 0; k < r.first.size(); ++k) r.first[k].f.out = stage + r.o.at[k];
  HIPCHK(h->vfetch_tab.put(r.first, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, before, 0));   // what the consumer had queued on the arrays
  HIPCHK(mckpp_launch_vaxis_fetch_planes(h->vfetch_tab, (int)r.first.size(), r.o.maxlev, h->d_ipt, h->ncol, h->npts, h->d_cs,
                                         nullptr, 0, h->stream));
  return 0;
}

// mckpp_hip_hv_fetch_dev: hgrid_fetch_dev's order with another first stage
int hv_fetch_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_hv_plane_c *planes, void *consumer_stream)
{
  std::vector<hv_fetch> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (hv_fetch_check(g.ctx[d], who, nplanes, planes, rs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  hgrid_outs &o = rs[0].o;
  for (int grid : o.grid)
    if (group_hgrid_out(g, who, grid)) return -1;
  for (size_t k = 0; k < o.second.size(); ++k) o.second[k].t = hgrid_ell(g.root()->hgd[o.grid[k]].out);
  return two_stage_deliver(g, who, o, dev, consumer_stream, [&](int d, double *stage, hipEvent_t before) {
    return hv_fetch_first(g.ctx[d], rs[(size_t)d], stage, before);
  });
}

// The planes of a put on a caller grid and a caller axis, checked and resolved into the kernel's table
int hv_put_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_hv_put_plane_c *planes,
                 std::vector<mckpp_hv_put_plane> &tab, int *dev)
{
  if (uploaded_check(h, who) || planes_count_check(who, nplanes, planes, MCKPP_HV_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  tab.clear();
  int prof[MCKPP_HV_PLANES_MAX];
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_hv_put_plane_c &q = planes[k];
    mckpp_hv_put_plane e{};
    int row;
    size_t elem;
    if (put_resolve(h, who, k, q.field, 0, h->nzp1, q.dtype, q.op, q.flags, q.skip_value, e.put, &row, &elem)) return -1;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d]", k);
    const mckpp_hip_ctx::vaxis *ax = vaxis_of(h, who, arg, q.axis);
    if (!ax) return -1;
    for (int j = 0; j < k; ++j)
      if (prof[j] == row)
        return fail("%s: planes[%d] and planes[%d] write the same field (%d, %d): a plane writes the whole profile, and the "
                    "planes of a call have no order", who, k, j, q.field, planes[j].field);
    prof[k] = row;
    const mckpp_hip_ctx::hgrid *g = hgrid_of(h, who, arg, q.grid);
    if (!g) return -1;
    if (g->in.ptr.empty())
      return fail("%s: planes[%d]: grid %d has no in table (caller -> model): mckpp_hip_hgrid_define was given none", who, k,
                  q.grid);
    snprintf(arg, sizeof arg, "planes[%d].in", k);
    if (dev_ptr_check(h, who, arg, q.in, (size_t)g->n * ax->z.size() * elem, k == 0 ? dev : nullptr)) return -1;
    e.put.in = q.in;
    e.skip = e.put.skip;   // decided on the input side, where the values the entries read are: put_element's own is off
    e.put.skip = 0;
    e.n = g->n;
    e.n_axis = (int)ax->z.size();
    e.tab = ax->d_in;
    if (hgrid_in_build(h, q.grid)) return -1;   // (on first use; an empty row is no refusal here)
    e.t = hgrid_ell(h->hgd[q.grid].in);
    tab.push_back(e);
  }
  return 0;
}

// put_queue's order with the launch of k_hv_put_planes
int hv_put_queue(mckpp_hip_ctx *h, const std::vector<mckpp_hv_put_plane> &tab, hipEvent_t produced)
{
  if (tab.empty() || h->ncol == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->hvput_tab.put(tab, h->stream));
  if (produced) HIPCHK(hipStreamWaitEvent(h->stream, produced, 0));
  HIPCHK(mckpp_launch_hv_put_planes(h->hvput_tab, (int)tab.size(), h->nzp1, h->ncol, h->d_cs, h->stream));
  HIPCHK(h->ev_read.record(h->stream));
  return 0;
}

// mckpp_hip_hv_put_dev: put_planes' order, every shard through its own in table
int hv_put_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_hv_put_plane_c *planes, void *producer_stream)
{
  std::vector<std::vector<mckpp_hv_put_plane>> tabs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (hv_put_check(g.ctx[d], who, nplanes, planes, tabs[(size_t)d], &dev)) return -1;
  if (dev < 0) return 0;   // (no plane)
  if (caller_event(g, dev, producer_stream)) return -1;
  for (int d = 0; d < g.n; ++d)
    if (hv_put_queue(g.ctx[d], tabs[(size_t)d], *g.ev)) return -1;
  return 0;
}

// ---------------------------------------------------------------------------
// Completed records on a caller axis (include/mckpp_hip_vrecords.h), the parts above put together once more.  A plane's
// field and axis are resolved by vaxis_fetch_resolve, its record by win_record_check, and the axis is held against the
// levels the schedule keeps by mckpp_host_vrecords_rule; the launch is k_vaxis_record_planes, queued in
// records_dev_queue's order.  The host form sends the same launch into the root's put staging and copies from there.  On
// a caller grid it is stage 1 of remap_records_dev's two stages, with the axis's n as the plane's levels.
// ---------------------------------------------------------------------------
// What planes[k] says of its field, its axis and its record, checked and resolved into the kernel's entry but for where
// it goes (out, map, npoints, the fill).  The schedule, or null and the refusal.
template <class P>
const mckpp_hip_ctx::win_sched *vrec_resolve(mckpp_hip_ctx *h, const char *who, int k, const P &q, mckpp_vrec_plane &e)
{
  out_desc d;
  const mckpp_hip_ctx::vaxis *ax = vaxis_fetch_resolve(h, who, k, q.field, q.axis, d);
  if (!ax) return nullptr;
  char at[96];
  snprintf(at, sizeof at, "%s: planes[%d]", who, k);
  size_t i = 0;
  if (win_record_check(h, at, q.sched, q.rec, true, q.field, q.op, &i)) return nullptr;
  const auto &w = h->wsched[q.sched];
  const int n = (int)ax->z.size();
  int32_t j = 0, lev = 0;
  if (mckpp_host_vrecords_rule(n, ax->out_branch.data(), ax->out_kin.data(), w.lev_off[i], w.nlev[i], &j, &lev) != 0)
    return fail("%s: planes[%d]: caller level %d of axis %d (z=%.17g) reads model level %d, and schedule %d keeps levels "
                "%d..%d of field %d: every model level the axis reads must be a kept level", who, k, (int)j, q.axis, ax->z[(size_t)j],
                (int)lev, q.sched, w.lev_off[i], w.lev_off[i] + w.nlev[i] - 1, q.field), nullptr;
  e.r.src = win_plane_rows(w, i, q.rec, q.op);
  e.r.period = (double)w.period;
  e.r.nrow = w.nrow;
  e.r.ld = w.ld_out[i]; e.r.off = 0; e.r.nlev = n;
  e.r.mean = q.op == 0;
  e.tab = ax->d_out;
  e.lev0 = w.lev_off[i];
  return &w;
}

// the planes of a delivery on caller axes resolved into the kernel's table, but for their non-row lists; [plane] its
// schedule and - the host form - the bytes of its array
struct vrec_planes {
  std::vector<mckpp_vrec_plane> tab;
  std::vector<int> sched;
  std::vector<size_t> bytes;
  int maxlev = 0;
};

int vrec_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes, bool dev_form,
               vrec_planes &r, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_VRECORDS_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = vrec_planes{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_vaxis_record_plane_c &q = planes[k];
    mckpp_vrec_plane e{};
    const auto *w = vrec_resolve(h, who, k, q, e);
    if (!w) return -1;
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem) return -1;
    const size_t bytes = (size_t)w->npoints * (size_t)e.r.nlev * elem;
    char arg[32];
    snprintf(arg, sizeof arg, "planes[%d].out", k);
    if (!dev_form) {
      if (!q.out) return fail("%s: %s is null", who, arg);
    } else if (dev_ptr_check(h, who, arg, q.out, bytes, k == 0 ? dev : nullptr)) {
      return -1;
    }
    e.r.out = q.out;
    e.r.map = win_map(h, *w);
    e.r.land_value = q.land_value;
    e.r.npoints = w->npoints;
    e.r.f32 = q.dtype == MCKPP_EXP_F32; e.r.fill = q.fill_land != 0;
    r.tab.push_back(e);
    r.sched.push_back(q.sched);
    r.bytes.push_back(bytes);
    r.maxlev = std::max(r.maxlev, e.r.nlev);
  }
  return 0;
}

// The table onto this context's device and the launch, on its stream.  fill: this context writes the land values the
// planes ask for (records_dev_queue's rule: the root does, from the lists group_norow has brought up to date).
int vrec_launch(mckpp_hip_ctx *h, vrec_planes &r, bool fill, hipEvent_t before)
{
  int64_t xtiles = 0;
  for (size_t k = 0; k < r.tab.size(); ++k) xtiles = std::max(xtiles, rec_plane_fill(h, r.tab[k].r, r.sched[k], fill));
  HIPCHK(rows_put(h, r.tab));
  if (before) HIPCHK(hipStreamWaitEvent(h->stream, before, 0));
  HIPCHK(rows_launch(h, r.tab, r.maxlev, xtiles));
  HIPCHK(h->ev_delivered.record(h->stream));
  return 0;
}

// The host form's delivery: every plane into the root's put staging (each at a multiple of 256 bytes) - a plane that
// keeps what its array held at the positions without a row goes up first -, every shard's rows behind that, and one copy
// per plane into the caller's array, pinned once, behind all of them on the root's stream; the call waits for it.
int vrec_host_deliver(const ctx_group &g, const char *who, std::vector<vrec_planes> &rs, const mckpp_vaxis_record_plane_c *planes)
{
  mckpp_hip_ctx *root = g.root();
  vrec_planes &r0 = rs[0];
  std::vector<size_t> at(r0.tab.size());
  size_t total = 0;
  for (size_t k = 0; k < r0.tab.size(); ++k) {
    at[k] = total;
    total += (r0.bytes[k] + 255) / 256 * 256;
  }
  HIPCHK(hipSetDevice(root->device));
  HIPCHK(root->d_put_stage.reserve(total));   // (every call that used the staging ended with a wait)
  char *stage = root->d_put_stage;
  for (int d = 1; d < g.n; ++d) {   // every shard's device reaches the root's staging (peer access, once per pair)
    HIPCHK(hipSetDevice(g.ctx[d]->device));
    if (dev_ptr_check(g.ctx[d], who, "the staging block of shard 0", stage, total)) return -1;
  }
  HIPCHK(hipSetDevice(root->device));
  for (size_t k = 0; k < r0.tab.size(); ++k) {
    pin_host(root, planes[k].out, r0.bytes[k]);
    if (!r0.tab[k].r.fill) HIPCHK(hipMemcpyAsync(stage + at[k], planes[k].out, r0.bytes[k], hipMemcpyHostToDevice, root->stream));
  }
  for (int d = 0; d < g.n; ++d) {
    mckpp_hip_ctx *x = g.ctx[d];
    vrec_planes &r = rs[(size_t)d];
    HIPCHK(hipSetDevice(x->device));
    for (size_t k = 0; k < r.tab.size(); ++k) r.tab[k].r.out = stage + at[k];
    // a further shard's rows behind the root's launch, which is behind the planes that went up
    if (vrec_launch(x, r, d == 0, d > 0 ? (hipEvent_t)root->ev_delivered : nullptr)) return -1;
    if (d > 0) {
      HIPCHK(hipSetDevice(root->device));
      HIPCHK(hipStreamWaitEvent(root->stream, x->ev_delivered, 0));
    }
  }
  HIPCHK(hipSetDevice(root->device));
  for (size_t k = 0; k < r0.tab.size(); ++k)
    HIPCHK(hipMemcpyAsync(planes[k].out, stage + at[k], r0.bytes[k], hipMemcpyDeviceToHost, root->stream));
  HIPCHK(hipStreamSynchronize(root->stream));
  return 0;
}

// mckpp_hip_vrecords_vaxis_dev / _host: records_dev's rule - a shard writes its own rows of every plane, the root the
// land values at the positions the group has no row for
int vrecords_vaxis(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes, bool dev_form,
                   void *consumer_stream)
{
  std::vector<vrec_planes> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (vrec_check(g.ctx[d], who, nplanes, planes, dev_form, rs[(size_t)d], dev_form ? &dev : nullptr)) return -1;
  const vrec_planes &r0 = rs[0];
  if (r0.tab.empty()) return 0;   // (no plane)
  for (size_t k = 0; k < r0.tab.size(); ++k)
    if (r0.tab[k].r.fill && group_norow(g, who, r0.sched[k])) return -1;
  if (!dev_form) return vrec_host_deliver(g, who, rs, planes);
  if (caller_event(g, dev, consumer_stream)) return -1;
  for (int d = 0; d < g.n; ++d) {
    mckpp_hip_ctx *x = g.ctx[d];
    HIPCHK(hipSetDevice(x->device));
    if (vrec_launch(x, rs[(size_t)d], d == 0, *g.ev)) return -1;   // behind what the consumer had queued on the arrays
    HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), x->ev_delivered, 0));
  }
  return 0;
}

int hv_records_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_hv_record_plane_c *planes, hv_recs &r, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_VRECORDS_PLANES_MAX) || uploaded_check(h, who)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = hv_recs{};
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_hv_record_plane_c &q = planes[k];
    mckpp_vrec_plane e{};   // into the staging by point number; what is no row is never written and never read
    const auto *w = vrec_resolve(h, who, k, q, e);
    if (!w) return -1;
    // the plane as hgrid_out_resolve reads one: its levels are the caller axis'
    const struct { int32_t grid, norm, nlev, dtype, fill_land; double land_value; void *out; } v{
        q.grid, q.norm, e.r.nlev, q.dtype, q.fill_land, q.land_value, q.out};
    const size_t elem = plane_elem(who, k, q.dtype);
    if (!elem || hgrid_out_resolve(h, who, k, v, elem, k == 0 ? dev : nullptr, r.o)) return -1;
    e.r.map = w->listed ? w->d_rowpt.get() : h->d_ipt.get();
    e.r.npoints = h->npts;
    r.first.push_back(e);
    r.sched.push_back(q.sched);
  }
  return 0;
}

// mckpp_hip_vrecords_hv_dev: remap_records_dev's order with another first stage
int vrecords_hv_dev(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_hv_record_plane_c *planes, void *consumer_stream)
{
  return grid_records_dev<mckpp_vrec_plane>(g, who, consumer_stream, [&](mckpp_hip_ctx *h, hv_recs &r, int *dev) {
    return hv_records_check(h, who, nplanes, planes, r, dev);
  });
}
}  // namespace
}  // extern "C++"

int mckpp_hip_hv_fetch_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return hv_fetch_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_hv_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return hv_put_dev(lone(h), who, nplanes, planes, producer_stream); });
}

int mckpp_hip_vrecords_vaxis_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vrecords_vaxis(lone(h), who, nplanes, planes, true, consumer_stream); });
}

int mckpp_hip_vrecords_vaxis_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vrecords_vaxis(lone(h), who, nplanes, planes, false, nullptr); });
}

int mckpp_hip_vrecords_hv_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_hv_record_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return vrecords_hv_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_remap_records_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_remap_record_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return remap_records_dev(lone(h), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_remap_put_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_remap_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return remap_put_dev(lone(h), who, nplanes, planes, producer_stream); });
}

// ---------------------------------------------------------------------------
// Records reduced over levels and points (include/mckpp_hip_reduce.h, which states the arithmetic).  A plane is resolved
// by the code that resolves a plane of mckpp_hip_records_dev; as there, a check that queues nothing and a part that
// queues.  Four launches on the context's stream - fill, terms, halve, finish (mckpp_kernels.hip) - and no host wait in
// the device form.
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
// the planes of a reduction resolved into the kernel's table, but for the blocks of the queueing context: [plane] its
// schedule, where its slabs begin in the block of terms, where its results do in the host form's block, their number
struct red_planes {
  std::vector<mckpp_red_plane> tab;
  std::vector<int> sched;
  std::vector<size_t> terms_off, out_off, nout;
  std::vector<void *> host_out;
  size_t terms = 0, outs = 0;
  int maxout = 0, maxslab = 0;
  int64_t xtiles = 0;
  bool halve = false, domain = false;
};

// fields whose axis is the interfaces 0 .. nz (the others with an axis are on the levels 1 .. nzp1)
bool on_interfaces(int f)
{
  switch (f) {
    case MCKPP_OUT_WU: case MCKPP_OUT_WV: case MCKPP_OUT_WT: case MCKPP_OUT_WS: case MCKPP_OUT_WB: case MCKPP_OUT_WTNT:
    case MCKPP_OUT_DIFM: case MCKPP_OUT_DIFT: case MCKPP_OUT_DIFS: return true;
    default: return false;
  }
}

int reduce_weights_check(const char *who, const char *name, const double *w, int64_t n)
{
  for (int64_t i = 0; w && i < n; ++i)
    if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
      return fail("%s: %s[%lld] = %g: every weight must be finite and >= 0", who, name, (long long)i, w[i]);
  return 0;
}

int reduce_weights_set(mckpp_hip_ctx *h, const char *who, const double *point_w, const double *level_w, const double *iface_w)
{
  if (h->npts <= 0) return fail("%s: upload the state first (point_w is sized to the grid's points)", who);
  if (reduce_weights_check(who, "point_w", point_w, h->npts) || reduce_weights_check(who, "level_w", level_w, h->nzp1) ||
      reduce_weights_check(who, "iface_w", iface_w, h->nzp1))
    return -1;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));   // a reduction in flight may read the weights in place
  auto &s = h->red;
  auto set = [](dev_buf<double> &d, const double *w, size_t n) -> hipError_t {
    if (!w) { d.reset(); return hipSuccess; }
    const hipError_t e = d.size() == n ? hipSuccess : d.alloc(n);
    return e == hipSuccess ? hipMemcpy(d, w, n * sizeof(double), hipMemcpyHostToDevice) : e;
  };
  HIPCHK(set(s.d_wp, point_w, (size_t)h->npts));
  HIPCHK(set(s.d_wl, level_w, (size_t)h->nzp1));
  HIPCHK(set(s.d_wi, iface_w, (size_t)h->nzp1));
  s.wl.assign(level_w, level_w ? level_w + h->nzp1 : level_w);
  s.wi.assign(iface_w, iface_w ? iface_w + h->nzp1 : iface_w);
  return 0;
}

const char *const red_op_names = "0 none, 1 sum, 2 average, 3 min, 4 max";

// dev: `out` is device memory, checked as mckpp_hip_records_dev checks it; otherwise host memory, refused if null
int reduce_check(mckpp_hip_ctx *h, const char *who, int32_t nplanes, const mckpp_reduce_plane_c *planes, bool dev_form,
                 red_planes &r, int *dev)
{
  if (planes_count_check(who, nplanes, planes, MCKPP_DEV_PLANES_MAX)) return -1;
  HIPCHK(hipSetDevice(h->device));
  r = red_planes{};
  const auto &s = h->red;
  for (int k = 0; k < nplanes; ++k) {
    const mckpp_reduce_plane_c &q = planes[k];
    char at[96], arg[32];
    snprintf(at, sizeof at, "%s: planes[%d]", who, k);
    snprintf(arg, sizeof arg, "planes[%d].out", k);
    size_t i = 0;
    mckpp_red_plane e{};
    const auto *sched = record_plane(h, who, k, q, e, &i);
    if (!sched) return -1;
    const auto &w = *sched;
    if (q.axis_op < 0 || q.axis_op > 4) return fail("%s: axis_op %d (%s)", at, q.axis_op, red_op_names);
    if (q.domain_op < 0 || q.domain_op > 4) return fail("%s: domain_op %d (%s)", at, q.domain_op, red_op_names);
    if (q.axis_op == 0 && q.domain_op == 0)
      return fail("%s: axis_op and domain_op are both 0 (none): a plane that is not reduced is mckpp_hip_records_dev's", at);
    if (q.weighted & ~3) return fail("%s: weighted 0x%x (bit 0: level weights, bit 1: point weights)", at, q.weighted);
    const double *wl = nullptr, *wp = nullptr;
    double wsum = (double)q.nlev;
    if (q.weighted & MCKPP_RED_W_LEVELS) {
      if (q.axis_op != MCKPP_RED_SUM && q.axis_op != MCKPP_RED_AVERAGE)
        return fail("%s: weighted bit 0 (level weights) with axis_op %d, a reduction that takes no weights (%s)", at, q.axis_op,
                    red_op_names);
      out_desc d;
      if (out_field(h, q.field, d)) return -1;
      if (d.nlev == 1) return fail("%s: weighted bit 0 (level weights), but field %d is two-dimensional", at, q.field);
      const bool iface = on_interfaces(q.field);
      const auto &hw = iface ? s.wi : s.wl;
      if (hw.empty())
        return fail("%s: weighted bit 0 (level weights), but no %s is set (mckpp_hip_reduce_weights; field %d is on the %s axis)", at,
                    iface ? "iface_w" : "level_w", q.field, iface ? "interface" : "level");
      const int first = w.lev_off[i] + q.lev0;
      wl = (iface ? s.d_wi.get() : s.d_wl.get()) + first;
      wsum = hw[(size_t)first];
      for (int l = 1; l < q.nlev; ++l) wsum = wsum + hw[(size_t)(first + l)];
    }
    if (q.weighted & MCKPP_RED_W_POINTS) {
      if (q.domain_op != MCKPP_RED_SUM && q.domain_op != MCKPP_RED_AVERAGE)
        return fail("%s: weighted bit 1 (point weights) with domain_op %d, a reduction that takes no weights (%s)", at, q.domain_op,
                    red_op_names);
      if (!s.d_wp) return fail("%s: weighted bit 1 (point weights), but no point_w is set (mckpp_hip_reduce_weights)", at);
      if ((int64_t)s.d_wp.size() != h->npts)
        return fail("%s: weighted bit 1 (point weights): point_w was set for %zu points, the grid has %lld", at, s.d_wp.size(),
                    (long long)h->npts);
      wp = s.d_wp;
    }
    const size_t nout = q.domain_op == 0 ? (size_t)w.npoints : q.axis_op == 0 ? (size_t)q.nlev : 1;
    if (!dev_form && !q.out) return fail("%s: %s is null", who, arg);
    if (dev_form && dev_ptr_check(h, who, arg, q.out, nout * sizeof(double), k == 0 ? dev : nullptr)) return -1;
    e.out = static_cast<double *>(q.out);
    e.map = win_map(h, w);
    e.point = w.listed ? w.d_rowpt.get() : h->d_ipt.get();
    e.wl = wl; e.wp = wp;
    e.land_value = q.land_value; e.wsum = wsum;
    e.n2 = 1;
    while (e.n2 < w.npoints) e.n2 *= 2;
    e.axis_op = q.axis_op; e.domain_op = q.domain_op;
    e.nslab = q.domain_op == 0 ? 0 : (q.axis_op == 0 ? q.nlev : 1) + (q.domain_op == MCKPP_RED_AVERAGE ? 1 : 0);
    r.tab.push_back(e);
    r.sched.push_back(q.sched);
    r.terms_off.push_back(r.terms);
    r.out_off.push_back(r.outs);
    r.nout.push_back(nout);
    r.host_out.push_back(q.out);
    r.terms += (size_t)e.nslab * (size_t)e.n2;
    r.outs += nout;
    r.maxslab = std::max(r.maxslab, e.nslab);
    if (q.domain_op != 0) r.maxout = std::max(r.maxout, (int)nout);
    r.xtiles = std::max<int64_t>(r.xtiles, (e.nrow + 63) / 64);
    r.domain = r.domain || q.domain_op != 0;
    r.halve = r.halve || (q.domain_op != 0 && e.n2 > h->red.m);
  }
  return 0;
}

// the blocks of `owner` (this context, or shard 0 of its multi handle) with room for the call; a block that grows may
// still be read by a reduction in flight, and everything that touches one is ordered on the owner's stream
int reduce_reserve(mckpp_hip_ctx *owner, const red_planes &r, bool dev_form)
{
  auto &s = owner->red;
  const size_t outs = dev_form ? 0 : r.outs;
  if (r.terms <= s.d_terms.size() && outs <= s.d_out.size()) return 0;
  HIPCHK(hipSetDevice(owner->device));
  HIPCHK(hipStreamSynchronize(owner->stream));
  HIPCHK(s.d_terms.reserve(r.terms));
  HIPCHK(s.d_out.reserve(outs));
  HIPCHK(s.h_out.reserve(outs));
  return 0;
}

// the table's blocks and lists: fill - this context writes what no row does (the root, from the lists group_norow has
// brought up to date); rows[k]: the rows all shards hold of plane k
int reduce_bind(mckpp_hip_ctx *h, mckpp_hip_ctx *owner, red_planes &r, bool dev_form, bool fill, const std::vector<int64_t> &rows)
{
  for (size_t k = 0; k < r.tab.size(); ++k) {
    mckpp_red_plane &e = r.tab[k];
    const auto &w = h->wsched[r.sched[k]];
    e.terms = owner->red.d_terms.get() + r.terms_off[k];
    if (!dev_form) e.out = owner->red.d_out.get() + r.out_off[k];
    e.fill = fill;
    e.norows = rows[k] == 0;
    if (fill && e.domain_op == 0) {
      if (w.listed) { e.norow = w.d_norow; e.nnorow = w.nnorow; }
      else { e.norow = h->d_land; e.nnorow = h->nland; }
    }
  }
  return 0;
}

int reduce_launch(mckpp_hip_ctx *h, const red_planes &r, int phase)
{
  HIPCHK(mckpp_launch_reduce(h->red_tab, (int)r.tab.size(), phase, r.maxout, r.maxslab, r.xtiles, h->red.m, h->stream));
  return 0;
}

// the host form's end on the owner's stream: one copy of all results through the pinned block, a wait, and out they go
int reduce_host_deliver(mckpp_hip_ctx *owner, const red_planes &r)
{
  auto &s = owner->red;
  HIPCHK(hipMemcpyAsync(s.h_out, s.d_out, r.outs * sizeof(double), hipMemcpyDeviceToHost, owner->stream));
  HIPCHK(hipStreamSynchronize(owner->stream));
  for (size_t k = 0; k < r.tab.size(); ++k) memcpy(r.host_out[k], s.h_out.get() + r.out_off[k], r.nout[k] * sizeof(double));
  return 0;
}

// mckpp_hip_records_reduce_dev / _host.  Per-shard sums combined afterwards would not be the single context's bits, so the
// shards deliver terms and the root reduces: the root fills its slabs (and the land values of the axis-only planes),
// every shard then writes the terms - or, axis only, the results - of its own rows, and behind all of them the root runs
// the tree and delivers.
int records_reduce(const ctx_group &g, const char *who, int32_t nplanes, const mckpp_reduce_plane_c *planes, bool dev_form,
                   void *consumer_stream)
{
  mckpp_hip_ctx *root = g.root();
  std::vector<red_planes> rs((size_t)g.n);
  int dev = -1;
  for (int d = 0; d < g.n; ++d)
    if (reduce_check(g.ctx[d], who, nplanes, planes, dev_form, rs[(size_t)d], &dev)) return -1;
  red_planes &r0 = rs[0];
  if (r0.tab.empty()) return 0;
  std::vector<int64_t> rows(r0.tab.size(), 0);
  for (size_t k = 0; k < r0.tab.size(); ++k) {
    for (int d = 0; d < g.n; ++d) rows[k] += rs[(size_t)d].tab[k].nrow;
    // axis only: the root writes the land value where the group has no row
    if (r0.tab[k].domain_op == 0 && group_norow(g, who, r0.sched[k])) return -1;
  }
  if (reduce_reserve(root, r0, dev_form)) return -1;
  for (int d = 1; d < g.n; ++d) {   // the other shards write into the root's blocks
    HIPCHK(hipSetDevice(g.ctx[d]->device));
    if (r0.terms > 0 && dev_ptr_check(g.ctx[d], who, "shard 0's block of terms", root->red.d_terms, r0.terms * sizeof(double)))
      return -1;
    if (!dev_form && dev_ptr_check(g.ctx[d], who, "shard 0's block of results", root->red.d_out, r0.outs * sizeof(double)))
      return -1;
  }
  for (int d = 0; d < g.n; ++d)
    if (reduce_bind(g.ctx[d], root, rs[(size_t)d], dev_form, d == 0, rows)) return -1;
  if (dev_form && caller_event(g, dev, consumer_stream)) return -1;
  HIPCHK(hipSetDevice(root->device));
  HIPCHK(root->red_tab.put(r0.tab, root->stream));
  if (dev_form) HIPCHK(hipStreamWaitEvent(root->stream, *g.ev, 0));   // what the consumer had queued on the arrays
  if (reduce_launch(root, r0, MCKPP_RED_PHASE_FILL)) return -1;
  if (g.n > 1) {   // the other shards' terms behind the root's fill
    HIPCHK(root->red.ev_fill.record(root->stream));
    for (int d = 1; d < g.n; ++d) {
      mckpp_hip_ctx *x = g.ctx[d];
      HIPCHK(hipSetDevice(x->device));
      HIPCHK(x->red_tab.put(rs[(size_t)d].tab, x->stream));
      HIPCHK(hipStreamWaitEvent(x->stream, root->red.ev_fill, 0));
      if (reduce_launch(x, rs[(size_t)d], MCKPP_RED_PHASE_TERMS)) return -1;
      HIPCHK(x->red.ev_terms.record(x->stream));
    }
    HIPCHK(hipSetDevice(root->device));
  }
  if (reduce_launch(root, r0, MCKPP_RED_PHASE_TERMS)) return -1;
  for (int d = 1; d < g.n; ++d) HIPCHK(hipStreamWaitEvent(root->stream, g.ctx[d]->red.ev_terms, 0));
  if (r0.halve && reduce_launch(root, r0, MCKPP_RED_PHASE_HALVE)) return -1;
  if (r0.domain && reduce_launch(root, r0, MCKPP_RED_PHASE_FINISH)) return -1;
  if (!dev_form) return reduce_host_deliver(root, r0);
  HIPCHK(root->ev_delivered.record(root->stream));
  HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), root->ev_delivered, 0));
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_hip_reduce_weights(mckpp_hip_handle h, const double *point_w, const double *level_w, const double *iface_w)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return reduce_weights_set(h, who, point_w, level_w, iface_w); });
}

int mckpp_hip_records_reduce_dev(mckpp_hip_handle h, int32_t nplanes, const mckpp_reduce_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return records_reduce(lone(h), who, nplanes, planes, true, consumer_stream); });
}

int mckpp_hip_records_reduce_host(mckpp_hip_handle h, int32_t nplanes, const mckpp_reduce_plane_c *planes)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return records_reduce(lone(h), who, nplanes, planes, false, nullptr); });
}

// the tree of include/mckpp_hip_reduce.h, c, as it is written there
double mckpp_host_reduce_tree(const double *t, int64_t n)
{
  double out = 0.0;
  (void)entry(__func__, [&]() -> int {
    if (!t || n <= 0) return 0;
    size_t n2 = 1;
    while (n2 < (size_t)n) n2 *= 2;
    std::vector<double> v(n2, 0.0);
    std::copy(t, t + n, v.begin());
    for (size_t m = n2 / 2; m >= 1; m /= 2)
      for (size_t i = 0; i < m; ++i) v[i] = v[i] + v[i + m];
    out = v[0];
    return 0;
  });
  return out;
}

// ---------------------------------------------------------------------------
// The export of a schedule's records (mckpp_hip_window_export).  window_record_fetch re-lays a plane on the context's
// stream and waits for it, so it cannot run under a later launch - and nothing but DMA can: k_column_ps fills every
// CU.  So all re-laying happens between the launches, on the context's stream: behind the launches of a call, one
// k_record_pack per record the call completed packs the record into its export slot, in the layout the host wants,
// and an event marks the slot.  A fetch is then one copy on the transfer stream behind that event; it never touches
// the context's stream.  The ring guard keeps later launches off the slots of unreleased records, as for snapshots.
// ---------------------------------------------------------------------------
using win_sched_t = mckpp_hip_ctx::win_sched;

static size_t exp_elem(int dtype) { return dtype == MCKPP_EXP_F32 ? sizeof(float) : sizeof(double); }

// the planes of a record of `w` over npts points: the fields in the schedule's order, the kept operations of each in
// bit order, every offset a multiple of 256 bytes
static int exp_layout(mckpp_hip_ctx *h, const win_sched_t &w, int64_t npts, int dtype, std::vector<win_sched_t::exp_plane> &planes,
                      size_t &record_bytes, int &maxlev)
{
  planes.clear();
  size_t off = 0;
  maxlev = 0;
  for (size_t i = 0; i < w.fields.size(); ++i) {
    for (int op = 0; op < 4; ++op) {
      if (!((w.ops[i] >> op) & 1u)) continue;
      planes.push_back({w.fields[i], op, w.nlev[i], (int64_t)off});
      off += (size_t)npts * (size_t)w.nlev[i] * exp_elem(dtype);
      off = (off + 255) & ~(size_t)255;
      maxlev = std::max(maxlev, w.nlev[i]);
    }
  }
  record_bytes = off;
  return 0;
}

// record `rec` into its export slot, and the slot's event, behind whatever the context's stream holds
static int exp_pack(mckpp_hip_ctx *h, win_sched_t &w, int64_t rec)
{
  auto &x = w.ex;
  const size_t slot = (size_t)(rec % w.nrec);
  if (x.slots && w.nrow > 0)
    HIPCHK(mckpp_launch_record_pack(x.d_tab, (int)x.planes.size(), x.maxlev, (int)slot, (double)w.period,
                                    x.compact ? nullptr : win_map(h, w), w.nrow, x.npts, x.slots + slot * x.record_bytes,
                                    x.dtype == MCKPP_EXP_F32, h->stream));
  HIPCHK(hipEventRecord(x.ev[slot], h->stream));
  return 0;
}

// after the launches of a call that began at step nt0 (win_advance has run): every record the call completed - one
// begun in an earlier call included - is packed
static int exp_advance(mckpp_hip_ctx *h, int nt0)
{
  if (h->ncol == 0) return 0;
  for (auto &w : h->wsched) {
    if (w.fields.empty() || w.ex.dtype == MCKPP_EXP_OFF) continue;
    const int64_t before = nt0 >= w.origin ? (nt0 - w.origin) / w.period - 1 : -1;   // complete before the call
    const int64_t lc = win_last_complete(w);
    for (int64_t rec = std::max(before + 1, w.first_kept); rec <= lc; ++rec)
      if (exp_pack(h, w, rec)) return -1;
  }
  return 0;
}

// a new export's first work on the stream: the land points, once - no step ever writes them (a shard's compact slots
// have none) -, every slot's event, and at once the records that are complete and not released
static int exp_start(mckpp_hip_ctx *h, win_sched_t &w, size_t total)
{
  const auto &x = w.ex;
  if (!x.compact && total > 0)
    HIPCHK(mckpp_launch_export_fill(x.slots, total / exp_elem(x.dtype), x.land, x.dtype == MCKPP_EXP_F32, h->stream));
  for (auto &ev : x.ev) HIPCHK(hipEventRecord(ev, h->stream));
  if (w.first_nt >= 0)
    for (int64_t rec = w.first_kept; rec <= win_last_complete(w); ++rec)
      if (exp_pack(h, w, rec)) return -1;
  return 0;
}

static int exp_set(mckpp_hip_ctx *h, const char *who, int sched, int dtype, double land_value, bool compact)
{
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  if (dtype != MCKPP_EXP_OFF && dtype != MCKPP_EXP_F64 && dtype != MCKPP_EXP_F32)
    return fail("%s: dtype %d (MCKPP_EXP_OFF 0, MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", who, dtype);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));   // no pack in flight may still write the slots
  exp_drop(w);
  if (dtype == MCKPP_EXP_OFF) return 0;
  win_sched_t::win_export x;
  x.dtype = dtype; x.compact = compact; x.land = land_value;
  x.npts = compact ? w.nrow : w.npoints;
  if (exp_layout(h, w, x.npts, dtype, x.planes, x.record_bytes, x.maxlev)) return -1;
  std::vector<mckpp_pack_plane> tab;
  for (const auto &p : x.planes) {
    size_t i = 0;
    while (w.fields[i] != p.field) ++i;
    const long long n = (long long)w.nrow * w.ld_out[i];
    mckpp_pack_plane e{};
    e.src = w.acc[i] + (long long)__builtin_popcount(w.ops[i] & ((1u << p.op) - 1u)) * n;
    e.slot_stride = (long long)__builtin_popcount(w.ops[i]) * n;
    e.dst_off = p.offset;
    e.ld = w.ld_out[i]; e.off = 0; e.nlev = p.nlev; e.op = p.op;
    tab.push_back(e);
  }
  const size_t total = (size_t)w.nrec * x.record_bytes;
  x.ev.resize((size_t)w.nrec);
  hipError_t e = hipSuccess;
  if (!h->snap_stream) e = h->snap_stream.create();
  if (e == hipSuccess && total > 0) e = x.slots.alloc(total);
  if (e == hipSuccess) e = x.d_tab.alloc(tab.size());
  for (int i = 0; i < w.nrec && e == hipSuccess; ++i) e = x.ev[(size_t)i].create();
  if (e == hipSuccess) e = hipMemcpy(x.d_tab, tab.data(), tab.size() * sizeof(mckpp_pack_plane), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: cannot allocate %zu bytes of device memory for the %d export slots of schedule %d (%s); the schedule "
                "stays set, without an export", who, total, w.nrec, sched, hipGetErrorString(e));
  }
  w.ex = std::move(x);
  if (exp_start(h, w, total)) {   // a failed call leaves the schedule without an export
    (void)hipStreamSynchronize(h->stream);
    exp_drop(w);
    return -1;
  }
  return 0;
}

int mckpp_hip_window_export(mckpp_hip_handle h, int sched, int dtype, double land_value)
{
  return entry(__func__, h, [&, who = __func__]() -> int { return exp_set(h, who, sched, dtype, land_value, false); });
}

// the layout of a record of the schedule's export over the points of its point axis (a shard's: of all shards')
static int exp_layout_out(mckpp_hip_ctx *h, const char *who, int sched, int32_t *nplanes, int32_t *field, int32_t *op,
                          int32_t *nlev, int64_t *offset_bytes, int64_t *record_bytes)
{
  if (sched < 0 || sched >= MCKPP_WIN_SCHEDULES) return fail("%s: schedule %d (0..%d)", who, sched, MCKPP_WIN_SCHEDULES - 1);
  const auto &w = h->wsched[sched];
  if (w.fields.empty()) return fail("%s: schedule %d is not set", who, sched);
  if (w.ex.dtype == MCKPP_EXP_OFF) return fail("%s: schedule %d has no export (mckpp_hip_window_export)", who, sched);
  std::vector<win_sched_t::exp_plane> planes;
  size_t rb = 0;
  int maxlev = 0;
  if (exp_layout(h, w, w.npoints, w.ex.dtype, planes, rb, maxlev)) return -1;
  if (nplanes) *nplanes = (int32_t)planes.size();
  for (size_t k = 0; k < planes.size(); ++k) {
    if (field) field[k] = planes[k].field;
    if (op) op[k] = planes[k].op;
    if (nlev) nlev[k] = planes[k].nlev;
    if (offset_bytes) offset_bytes[k] = planes[k].offset;
  }
  if (record_bytes) *record_bytes = (int64_t)rb;
  return 0;
}

int mckpp_hip_window_export_layout(mckpp_hip_handle h, int sched, int32_t *nplanes, int32_t *field, int32_t *op, int32_t *nlev,
                                   int64_t *offset_bytes, int64_t *record_bytes)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  return exp_layout_out(h, who, sched, nplanes, field, op, nlev, offset_bytes, record_bytes);
  });
}

// may record `rec` (plane: its plane of field and op, whose index among the export's planes comes back) be fetched
// through the export?  win_record's checks and messages, then the export's own
static int exp_check(mckpp_hip_ctx *h, const char *who, int sched, int64_t rec, bool plane, int field, int op, size_t *k)
{
  if (win_record_check(h, who, sched, rec, plane, field, op, nullptr)) return -1;
  const auto &x = h->wsched[sched].ex;
  if (x.dtype == MCKPP_EXP_OFF) return fail("%s: schedule %d has no export (mckpp_hip_window_export)", who, sched);
  size_t i = 0;
  if (plane) while (x.planes[i].field != field || x.planes[i].op != op) ++i;   // (kept: win_record_check)
  if (k) *k = i;
  return 0;
}

// `bytes` from `off` of the record's slot on their way into `out`, on the transfer stream behind the slot's event
static int exp_copy_start(mckpp_hip_ctx *h, const win_sched_t &w, int64_t rec, size_t off, size_t bytes, void *out)
{
  if (bytes == 0 || !w.ex.slots) return 0;
  const size_t slot = (size_t)(rec % w.nrec);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamWaitEvent(h->snap_stream, w.ex.ev[slot], 0));
  HIPCHK(hipMemcpyAsync(out, w.ex.slots + slot * w.ex.record_bytes + off, bytes, hipMemcpyDeviceToHost, h->snap_stream));
  return 0;
}

static int exp_copy_finish(mckpp_hip_ctx *h)
{
  if (!h->snap_stream) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->snap_stream));
  return 0;
}

static int exp_fetch(mckpp_hip_ctx *h, const char *who, int sched, int64_t rec, bool plane, int field, int op, void *out,
                     int64_t out_bytes)
{
  size_t k = 0;
  if (exp_check(h, who, sched, rec, plane, field, op, &k)) return -1;
  const auto &w = h->wsched[sched];
  const auto &x = w.ex;
  size_t off = 0, bytes = x.record_bytes;
  if (plane) { off = (size_t)x.planes[k].offset; bytes = (size_t)x.npts * (size_t)x.planes[k].nlev * exp_elem(x.dtype); }
  else if (out_bytes < (int64_t)x.record_bytes)
    return fail("%s: out_bytes %lld, but a record of schedule %d takes %zu bytes", who, (long long)out_bytes, sched, x.record_bytes);
  pin_host(h, out, bytes);
  const int rc = exp_copy_start(h, w, rec, off, bytes, out);
  if (exp_copy_finish(h)) return -1;   // (also behind a copy that could not be started: nothing stays in flight)
  return rc;
}

int mckpp_hip_window_export_fetch(mckpp_hip_handle h, int sched, int64_t rec, int field, int op, void *out)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!out) return fail("%s: null argument", who);
  return exp_fetch(h, who, sched, rec, true, field, op, out, 0);
  });
}

int mckpp_hip_window_export_fetch_record(mckpp_hip_handle h, int sched, int64_t rec, void *out, int64_t out_bytes)
{
  return entry(__func__, h, [&, who = __func__]() -> int {
  if (!out) return fail("%s: null argument", who);
  return exp_fetch(h, who, sched, rec, false, 0, 0, out, out_bytes);
  });
}

int mckpp_hip_status(mckpp_hip_handle h, int32_t *per_col, int64_t *n_flagged, int32_t *npasses)
{
  return entry(__func__, h, [&]() -> int {
  if (per_col) for (int64_t i = 0; i < h->npts; ++i) per_col[i] = 0;
  if (npasses) for (int64_t i = 0; i < h->npts; ++i) npasses[i] = 0;
  int64_t nf = 0;
  if (h->ncol > 0) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    // (the whole records, one contiguous copy; a 2-D copy of the two ints per record is no faster at 1e5 columns)
    std::vector<int> ci((size_t)h->ncol * MCKPP_CI);
    HIPCHK(hipMemcpy(ci.data(), h->d_ci, ci.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < h->ncol; ++c) {
      const int st = ci[(size_t)c * MCKPP_CI + CI_STATUS];
      if (st) ++nf;
      if (per_col) per_col[h->ipt[c]] = st;
      if (npasses) npasses[h->ipt[c]] = ci[(size_t)c * MCKPP_CI + CI_NPASS];
    }
  }
  if (n_flagged) *n_flagged = nf;
  return 0;
  });
}

int mckpp_hip_eos_batch(mckpp_hip_handle h, int64_t n, const double *s, const double *t, const double *p,
                        double *alpha, double *beta, double *sig0, double *cp)
{
  return entry(__func__, h, [&]() -> int {
  if (n <= 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  dev_buf<double> d;
  const size_t nb = (size_t)n * sizeof(double);
  HIPCHK(d.alloc(7 * (size_t)n));
  HIPCHK(hipMemcpy(d, s, nb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + n, t, nb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + 2 * n, p, nb, hipMemcpyHostToDevice));
  hipError_t e = mckpp_launch_eos_batch(n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n, d + 6 * n, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(alpha, d + 3 * n, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(beta, d + 4 * n, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(sig0, d + 5 * n, nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cp, d + 6 * n, nb, hipMemcpyDeviceToHost);
  HIPCHK(e);
  return 0;
  });
}

int mckpp_hip_div_batch(mckpp_hip_handle h, int64_t n, const double *num, const double *den, double *q4)
{
  return entry(__func__, h, [&]() -> int {
  if (n <= 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  dev_buf<double> d;
  const size_t nb = (size_t)n * sizeof(double);
  HIPCHK(d.alloc(6 * (size_t)n));
  hipError_t e = hipMemcpy(d, num, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, den, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = mckpp_launch_div_batch(n, d, d + n, d + 2 * n, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(q4, d + 2 * n, 4 * nb, hipMemcpyDeviceToHost);
  HIPCHK(e);
  return 0;
  });
}

int mckpp_hip_exp_batch(mckpp_hip_handle h, int64_t n, const double *x, double *y)
{
  return entry(__func__, h, [&]() -> int {
  if (n <= 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  dev_buf<double> d;
  const size_t nb = (size_t)n * sizeof(double);
  HIPCHK(d.alloc(2 * (size_t)n));
  hipError_t e = hipMemcpy(d, x, nb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = mckpp_launch_exp_batch(n, d, d + n, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(y, d + n, nb, hipMemcpyDeviceToHost);
  HIPCHK(e);
  return 0;
  });
}

// ---------------------------------------------------------------------------
// Several GPUs behind one handle: the run_physics columns are dealt round-robin to the
// devices (pass counts vary along a latitude band, so a contiguous split would unbalance the shards),
// every device holds the constants, a step launches on every device's stream before anything waits,
// and nothing crosses devices inside a step.  The only exchange is the output gather to one root
// device over the GPU interconnect (xGMI peer copies), relayout there, one transfer to the host.
// ---------------------------------------------------------------------------
// root-side resources of the gather, owned by the root device of the last gather (multi_release_root drops them as a
// whole): one stream per shard, the events that order a shard's copy behind its owner's stream and the final transfer
// behind all shards, the 3-D image, the staging area the shards' rows arrive in, every shard's column map
struct mckpp_multi_root {
  int root = -1;
  std::vector<hip_stream> gstream;          // [ndev], on the root device
  std::vector<hip_event> ev_done;           // [ndev], on the root device
  hip_event ev_init, ev_gcopy;              // on the root device: 3-D image ready for the shards / delivered to the host
  dev_buf<double> d_out, d_stage;           // grow-only (multi_prepare_root)
  dev_buf<int> d_gipt;
  bool gipt_valid = false;                  // d_gipt holds the maps of the current upload
  dev_buf<int> d_zmap;                      // grow-only: the shards' row maps of the zoomed record being gathered
};

struct mckpp_hip_multi : mckpp_multi_root {
  std::vector<mckpp_hip_ctx *> ctx;
  int64_t npts = 0;
  std::vector<std::vector<int32_t>> mask;   // run_physics of each shard
  std::vector<hip_event> ev_owner;          // [ndev], each on its shard's device
  // pinned staging the shards' export planes arrive in before the host merges them (mckpp_hip_multi_window_export_fetch)
  pinned_buf<char> h_exp;
  // the event on the caller's stream that orders every shard's part of a device-array call, on device ev_caller_dev
  hip_event ev_caller;
  int ev_caller_dev = -1;
};

// run_physics mask of shard `dev` of `ndev`: the j-th ocean point (in ipt order) goes to shard j mod ndev
int64_t mckpp_host_shard_mask(int64_t npts, const int32_t *run_physics, int32_t ndev, int32_t dev, int32_t *mask_out)
{
  if (npts < 0 || ndev < 1 || dev < 0 || dev >= ndev || !mask_out) return -1;
  int64_t j = 0, mine = 0;
  for (int64_t i = 0; i < npts; ++i) {
    const bool ocean = !run_physics || run_physics[i];
    mask_out[i] = (ocean && (j % ndev) == dev) ? 1 : 0;
    if (ocean) { mine += mask_out[i]; ++j; }
  }
  return mine;
}

// the root-side buffers, streams and events go with the root device they were created on
static void multi_release_root(mckpp_hip_multi *m)
{
  if (m->root < 0) return;
  hipSetDevice(m->ctx[m->root]->device);
  for (auto &st : m->gstream) if (st) hipStreamSynchronize(st);   // nothing of a gather may still use the buffers
  static_cast<mckpp_multi_root &>(*m) = mckpp_multi_root{};
}

int mckpp_hip_multi_init(const mckpp_const_c *c, int32_t ndev, const int32_t *devices, mckpp_hip_multi_handle *out)
{
  return entry(__func__, [&]() -> int {
  if (!c || !out || ndev < 1) return fail("mckpp_hip_multi_init: bad argument (ndev=%d)", ndev);
  // any return or throw below finalizes the shards made so far, once (mckpp_hip_multi_finalize takes any stage of this)
  half_built<mckpp_hip_multi, mckpp_hip_multi_finalize> m(new mckpp_hip_multi());
  m->ctx.reserve((size_t)ndev);   // (so that no context can be made and then not be kept)
  for (int d = 0; d < ndev; ++d) {
    mckpp_hip_handle h = nullptr;
    if (mckpp_hip_init(c, devices ? devices[d] : d, &h) != 0) return -1;   // message of mckpp_hip_init
    m->ctx.push_back(h);
  }
  m->mask.resize(ndev);
  m->ev_owner.resize(ndev);
  for (int d = 0; d < ndev; ++d)
    if (hipSetDevice(m->ctx[d]->device) != hipSuccess || m->ev_owner[d].create() != hipSuccess)
      return fail("mckpp_hip_multi_init: cannot create the events of shard %d", d);
  *out = m.release();
  return 0;
  });
}

int mckpp_hip_multi_finalize(mckpp_hip_multi_handle m)
{
  if (!m) return 0;
  multi_release_root(m);
  for (size_t d = 0; d < m->ev_owner.size(); ++d)
    if (m->ev_owner[d]) { hipSetDevice(m->ctx[d]->device); m->ev_owner[d].reset(); }
  for (auto *x : m->ctx) mckpp_hip_finalize(x);
  delete m;
  return 0;
}

int32_t mckpp_hip_multi_ndev(mckpp_hip_multi_handle m) { return m ? (int32_t)m->ctx.size() : -1; }
mckpp_hip_handle mckpp_hip_multi_ctx(mckpp_hip_multi_handle m, int32_t i)
{
  const bool ok = m && i >= 0 && i < (int)m->ctx.size();
  if (!ok) entry(__func__, [&]() -> int { return fail("mckpp_hip_multi_ctx: shard %d", i); });
  return ok ? m->ctx[i] : nullptr;
}

int mckpp_hip_multi_upload(mckpp_hip_multi_handle m, const mckpp_state_ptrs_c *s)
{
  return entry(__func__, m, [&]() -> int {
  if (!s) return fail("mckpp_hip_multi_upload: null argument");
  if (s->npts <= 0) return fail("mckpp_hip_multi_upload: npts=%lld", (long long)s->npts);
  const int ndev = (int)m->ctx.size();
  m->npts = s->npts;
  for (int d = 0; d < ndev; ++d) {
    m->mask[d].assign((size_t)s->npts, 0);
    mckpp_host_shard_mask(s->npts, s->run_physics, ndev, d, m->mask[d].data());
    mckpp_state_ptrs_c sd = *s;
    sd.run_physics = m->mask[d].data();
    if (mckpp_hip_upload(m->ctx[d], &sd) != 0) return -1;
  }
  m->gipt_valid = false;   // the root's copy of the column maps is of the previous upload
  for (auto *x : m->ctx) x->land_kind = 0;   // ... and so is shard 0's list of the points that no shard holds
  for (auto *x : m->ctx)
    for (auto &g : x->hgd) g.out.kind = 0;   // ... and the out tables of the caller's grids, built for the union of the shards' columns
  return 0;
  });
}

// the entry points that are the same call on every shard: the first failure ends them, with the shard's text
extern "C++" template <class F>
int multi_each(const char *who, mckpp_hip_multi *m, F &&call) noexcept
{
  return entry(who, m, [&]() -> int {
  for (auto *x : m->ctx) if (call(x) != 0) return -1;
  return 0;
  });
}

int mckpp_hip_multi_set_forcing(mckpp_hip_multi_handle m, const double *sflux) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_forcing(x, sflux); }); }
int mckpp_hip_multi_set_diagnostics(mckpp_hip_multi_handle m, int on) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_diagnostics(x, on); }); }
int mckpp_hip_multi_set_solver_mode(mckpp_hip_multi_handle m, int mode) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_solver_mode(x, mode); }); }
int mckpp_hip_multi_init_ocean(mckpp_hip_multi_handle m, int ntime) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_init_ocean(x, ntime); }); }
// asynchronous on every device: all shards are launched before the caller can wait on any of them
int mckpp_hip_multi_step(mckpp_hip_multi_handle m, int ntime, int nsteps) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_step(x, ntime, nsteps); }); }
int mckpp_hip_multi_synchronize(mckpp_hip_multi_handle m) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_synchronize(x); }); }
int mckpp_hip_multi_update_ancillaries(mckpp_hip_multi_handle m, const mckpp_state_ptrs_c *s) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_update_ancillaries(x, s); }); }
int mckpp_hip_multi_bottomtemp(mckpp_hip_multi_handle m, const double *bottom_temp) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_bottomtemp(x, bottom_temp); }); }
int mckpp_hip_multi_set_bottomtemp(mckpp_hip_multi_handle m, const double *bottom_temp) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_bottomtemp(x, bottom_temp); }); }
int mckpp_hip_multi_set_ancillary_series(mckpp_hip_multi_handle m, int kind, int rec0, int nrec, const double *records)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_ancillary_series(x, kind, rec0, nrec, records); });
}
int mckpp_hip_multi_ancillary_schedule(mckpp_hip_multi_handle m, int kind, int nt_origin, int cadence, int epoch0, int nepochs,
                                       const mckpp_anc_epoch_c *epochs)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_ancillary_schedule(x, kind, nt_origin, cadence, epoch0, nepochs, epochs); });
}
int mckpp_hip_multi_fluxes(mckpp_hip_multi_handle m, int ntime, const double *taux, const double *tauy, const double *swf,
                           const double *lwf, const double *lhf, const double *shf, const double *rain, const double *snow,
                           int l_rest, double flsn, double el)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_fluxes(x, ntime, taux, tauy, swf, lwf, lhf, shf, rain, snow, l_rest, flsn, el); });
}
int64_t mckpp_hip_multi_ncolumns(mckpp_hip_multi_handle m)
{
  if (!m) return -1;
  int64_t n = 0;
  for (auto *x : m->ctx) n += x->ncol;
  return n;
}

int mckpp_hip_multi_status(mckpp_hip_multi_handle m, int32_t *per_col, int64_t *n_flagged, int32_t *npasses)
{
  return entry(__func__, m, [&]() -> int {
  int64_t nf = 0;
  std::vector<int32_t> st, np_;
  if (per_col) { st.assign((size_t)m->npts, 0); for (int64_t i = 0; i < m->npts; ++i) per_col[i] = 0; }
  if (npasses) { np_.assign((size_t)m->npts, 0); for (int64_t i = 0; i < m->npts; ++i) npasses[i] = 0; }
  for (auto *x : m->ctx) {
    int64_t f = 0;
    if (mckpp_hip_status(x, per_col ? st.data() : nullptr, &f, npasses ? np_.data() : nullptr) != 0) return -1;
    nf += f;
    for (int64_t c = 0; c < x->ncol; ++c) {
      const int i = x->ipt[(size_t)c];
      if (per_col) per_col[i] = st[(size_t)i];
      if (npasses) npasses[i] = np_[(size_t)i];
    }
  }
  if (n_flagged) *n_flagged = nf;
  return 0;
  });
}

// ---- The gather.  One row field of every shard -> the caller's (npts, nlev) array in the Fortran
// layout: the shards' rows travel device to device to shard `root` (peer copies over the GPU interconnect, each on
// its own stream of the root device behind an event on its owner's stream - so all of them are in flight at once,
// and a gather queued behind a step overlaps the other shards' tail), are re-laid there into the 3-D order by one
// kernel per shard (disjoint points), and cross PCIe once.  Land points keep what `out` held.  `src[d]` are the
// shards' device rows (ld doubles each), src_off the first element taken from a row.
static int multi_prepare_root(mckpp_hip_multi *m, int root, size_t nout, size_t nstage)
{
  const int ndev = (int)m->ctx.size();
  mckpp_hip_ctx *r = m->ctx[root];
  if (m->root != root) {
    multi_release_root(m);
    HIPCHK(hipSetDevice(r->device));
    mckpp_multi_root n;   // built here, moved in when all of it is there
    n.root = root;
    n.gstream.resize(ndev);
    n.ev_done.resize(ndev);
    for (int d = 0; d < ndev; ++d) {
      HIPCHK(n.gstream[d].create());
      HIPCHK(n.ev_done[d].create());
      if (d != root && m->ctx[d]->device != r->device) {
        hipError_t e = hipDeviceEnablePeerAccess(m->ctx[d]->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();   // staged copies still work
      }
    }
    HIPCHK(n.ev_init.create());
    HIPCHK(n.ev_gcopy.create());
    static_cast<mckpp_multi_root &>(*m) = std::move(n);
  }
  HIPCHK(hipSetDevice(r->device));
  size_t ngipt = 0;
  for (auto *x : m->ctx) ngipt += (size_t)x->ncol;
  const bool grow = nout > m->d_out.size() || nstage > m->d_stage.size() || ngipt > m->d_gipt.size();
  if (grow) {   // nothing of an earlier gather may still be using the buffers
    for (auto &st : m->gstream) HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(r->stream));
    HIPCHK(hipStreamSynchronize(r->copy_stream));
  }
  HIPCHK(m->d_out.reserve(nout));
  HIPCHK(m->d_stage.reserve(nstage));
  if (ngipt > m->d_gipt.size()) { m->gipt_valid = false; HIPCHK(m->d_gipt.reserve(ngipt)); }
  if (!m->gipt_valid) {   // the shards' column maps, once per upload
    size_t go = 0;
    for (auto *x : m->ctx) {
      if (x->ncol) HIPCHK(hipMemcpy(m->d_gipt + go, x->ipt.data(), (size_t)x->ncol * sizeof(int), hipMemcpyHostToDevice));
      go += (size_t)x->ncol;
    }
    m->gipt_valid = true;
  }
  return 0;
}

// The shards' rows gathered into out(npts, nlev).  `z` null: a shard's rows are its resident columns, at the points of
// its column map.  Otherwise the rows of a record with a point list (mckpp_hip_window_schedule_zoom): shard d has
// z->nrow[d] of them, row r at position z->map[d][r] of the list's z->npoints points.
struct multi_rows { int64_t npoints; std::vector<int64_t> nrow; std::vector<const std::vector<int> *> map; };

static int multi_gather_rows(mckpp_hip_multi *m, int root, const std::vector<const double *> &src, int ld, int src_off,
                             int nlev, double *out, const double *whole = nullptr, size_t whole_elems = 0,
                             const multi_rows *z = nullptr)
{
  const int ndev = (int)m->ctx.size();
  mckpp_hip_ctx *r = m->ctx[root];
  const int64_t npts = z ? z->npoints : m->npts;
  auto rows_of = [&](int d) { return z ? z->nrow[(size_t)d] : m->ctx[d]->ncol; };
  const size_t nout = (size_t)npts * nlev;
  size_t nstage = 0, ncols = 0;
  for (int d = 0; d < ndev; ++d) {
    ncols += (size_t)rows_of(d);
    if (d != root) nstage += (size_t)rows_of(d) * ld;   // the root's own rows are read where they are
  }
  if (z && ncols == 0) return 0;   // (no listed point is a resident column: `out` stays as it is)
  if (multi_prepare_root(m, root, nout, nstage ? nstage : 1)) return -1;
  const int *map = m->d_gipt;
  if (z) {   // (the gathers before this one have delivered: multi_gather_finish)
    HIPCHK(m->d_zmap.reserve(ncols));
    size_t go = 0;
    for (int d = 0; d < ndev; ++d) {
      if (rows_of(d)) HIPCHK(hipMemcpy(m->d_zmap + go, z->map[(size_t)d]->data(), (size_t)rows_of(d) * sizeof(int), hipMemcpyHostToDevice));
      go += (size_t)rows_of(d);
    }
    map = m->d_zmap;
  }
  if (whole) pin_host(r, whole, whole_elems * sizeof(double));
  else pin_host(r, out, nout * sizeof(double));
  // the 3-D image: behind the transfer of the previous gather; land points keep the caller's values
  HIPCHK(hipStreamWaitEvent(r->stream, m->ev_gcopy, 0));
  if (ncols < (size_t)npts) HIPCHK(hipMemcpyAsync(m->d_out, out, nout * sizeof(double), hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipEventRecord(m->ev_init, r->stream));
  size_t so = 0, go = 0;
  for (int d = 0; d < ndev; ++d) {
    mckpp_hip_ctx *x = m->ctx[d];
    const int64_t nrow = rows_of(d);
    if (nrow == 0) continue;
    const size_t n = (size_t)nrow * ld;
    hipStream_t gs = m->gstream[d];
    HIPCHK(hipSetDevice(x->device));
    HIPCHK(hipEventRecord(m->ev_owner[d], x->stream));   // whatever the owner's stream still has queued
    HIPCHK(hipSetDevice(r->device));
    HIPCHK(hipStreamWaitEvent(gs, m->ev_owner[d], 0));
    HIPCHK(hipStreamWaitEvent(gs, m->ev_init, 0));
    const double *rows = src[d];
    if (d != root) {
      if (x->device == r->device) HIPCHK(hipMemcpyAsync(m->d_stage + so, src[d], n * sizeof(double), hipMemcpyDeviceToDevice, gs));
      else HIPCHK(hipMemcpyPeerAsync(m->d_stage + so, r->device, src[d], x->device, n * sizeof(double), gs));
      rows = m->d_stage + so;
      so += n;
    }
    HIPCHK(mckpp_launch_scatter_rows(rows, ld, src_off, map + go, nrow, m->d_out, npts, nlev, 0, gs));
    HIPCHK(hipEventRecord(m->ev_done[d], gs));
    HIPCHK(hipStreamWaitEvent(r->copy_stream, m->ev_done[d], 0));
    go += (size_t)nrow;
  }
  HIPCHK(hipStreamWaitEvent(r->copy_stream, m->ev_init, 0));
  HIPCHK(hipMemcpyAsync(out, m->d_out, nout * sizeof(double), hipMemcpyDeviceToHost, r->copy_stream));
  HIPCHK(hipEventRecord(m->ev_gcopy, r->copy_stream));
  return 0;
}

// the gathers queued so far have delivered
static int multi_gather_finish(mckpp_hip_multi *m)
{
  if (m->root < 0) return 0;
  mckpp_hip_ctx *r = m->ctx[m->root];
  HIPCHK(hipSetDevice(r->device));
  HIPCHK(hipStreamSynchronize(r->copy_stream));
  return 0;
}

// `field` 0 U, 1 V, 2 T, 3 S -> out(npts,nzp1), 4 hmix -> out(npts)
int mckpp_hip_multi_gather(mckpp_hip_multi_handle m, int32_t field, int32_t root, double *out)
{
  return entry(__func__, m, [&]() -> int {
  if (!out) return fail("mckpp_hip_multi_gather: null argument");
  const int ndev = (int)m->ctx.size();
  if (root < 0 || root >= ndev) return fail("mckpp_hip_multi_gather: root %d of %d", root, ndev);
  if (field < 0 || field > 4) return fail("mckpp_hip_multi_gather: field %d", field);
  if (m->npts <= 0) return fail("mckpp_hip_multi_gather: nothing uploaded");
  std::vector<const double *> src(ndev);
  for (int d = 0; d < ndev; ++d) {
    mckpp_hip_ctx *x = m->ctx[d];
    src[d] = field == 0 ? x->d_prof[P_U] : field == 1 ? x->d_prof[P_V] : field == 2 ? x->d_prof[P_T]
           : field == 3 ? x->d_prof[P_S] : x->d_cs;
  }
  mckpp_hip_ctx *r = m->ctx[root];
  if (multi_gather_rows(m, root, src, field < 4 ? r->ld : MCKPP_CS, field < 4 ? 0 : CS_HMIX, field < 4 ? r->nzp1 : 1, out))
    return -1;
  return multi_gather_finish(m);
  });
}

// mckpp_hip_download for all shards: the per-column records of every shard come to the host on their own (each
// crosses PCIe once), every row field goes through the gather - one transfer per field, whatever the number
// of devices.
int mckpp_hip_multi_download(mckpp_hip_multi_handle m, mckpp_state_ptrs_c *s, uint32_t mask)
{
  return entry(__func__, m, [&]() -> int {
  if (!s) return fail("mckpp_hip_multi_download: null argument");
  if (s->npts != m->npts) return fail("mckpp_hip_multi_download: npts=%lld but %lld were uploaded", (long long)s->npts, (long long)m->npts);
  const int ndev = (int)m->ctx.size();
  std::vector<std::vector<row_xfer>> plans(ndev);
  for (int d = 0; d < ndev; ++d) row_plan(m->ctx[d], s, T_DOWN, mask, plans[d]);
  std::vector<const double *> src(ndev);
  for (size_t e = 0; e < plans[0].size(); ++e) {
    for (int d = 0; d < ndev; ++d) src[d] = plans[d][e].dev;
    const row_xfer &x = plans[0][e];
    if (multi_gather_rows(m, 0, src, m->ctx[0]->ld, x.off, x.nlev, x.host, x.whole, x.whole_elems)) return -1;
  }
  for (auto *x : m->ctx) {
    if (x->ncol == 0) continue;
    HIPCHK(hipSetDevice(x->device));
    if (download_records(x, s, mask)) return -1;
  }
  return multi_gather_finish(m);
  });
}

// ---- the forced time loop, the output windows and the restart set for all shards
int mckpp_hip_multi_set_flux_series(mckpp_hip_multi_handle m, int rec0, int nrec, const double *fields)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_set_flux_series(x, rec0, nrec, fields); });
}
// the flux ring over all shards: every shard compacts its own columns of the one caller array into its own ring
int mckpp_hip_multi_flux_ring(mckpp_hip_multi_handle m, int nslots)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_flux_ring(x, nslots); });
}
int mckpp_hip_multi_flux_ring_put(mckpp_hip_multi_handle m, int rec, const double *fields)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_flux_ring_put(x, rec, fields); });
}
// the range common to all shards (they are put to together: it is every shard's own)
int mckpp_hip_multi_flux_ring_records(mckpp_hip_multi_handle m, int *first, int *last)
{
  return entry(__func__, m, [&]() -> int {
  int a = -1, b = -1;
  bool any = false, empty = false;
  for (auto *x : m->ctx) {
    int fa, fb;
    if (mckpp_hip_flux_ring_records(x, &fa, &fb) != 0) return -1;
    if (fb < 0) empty = true;
    a = any ? std::max(a, fa) : fa;
    b = any ? std::min(b, fb) : fb;
    any = true;
  }
  if (empty || a > b) a = b = -1;
  if (first) *first = a;
  if (last) *last = b;
  return 0;
  });
}
// asynchronous on every device, like mckpp_hip_multi_step
int mckpp_hip_multi_run_forced(mckpp_hip_multi_handle m, int nt_first, int nsteps, int ndtocn, int l_rest, double flsn, double el)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_run_forced(x, nt_first, nsteps, ndtocn, l_rest, flsn, el); });
}
int mckpp_hip_multi_window_select(mckpp_hip_multi_handle m, const int32_t *fields, int32_t nfields) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_select(x, fields, nfields); }); }
int mckpp_hip_multi_window_reset(mckpp_hip_multi_handle m) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_reset(x); }); }
int mckpp_hip_multi_window_accumulate(mckpp_hip_multi_handle m) { return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_accumulate(x); }); }

// every shard reduces its own columns; the reduced rows are gathered like any other field
int mckpp_hip_multi_window_fetch(mckpp_hip_multi_handle m, int field, int op, double *out)
{
  return entry(__func__, m, [&]() -> int {
  if (!out) return fail("mckpp_hip_multi_window_fetch: null argument");
  if (m->npts <= 0) return fail("mckpp_hip_multi_window_fetch: nothing uploaded");
  const int ndev = (int)m->ctx.size();
  std::vector<const double *> src(ndev, nullptr);
  int ld_out = 0, nlev = 0;
  for (int d = 0; d < ndev; ++d)
    if (window_prepare(m->ctx[d], field, op, &src[d], &ld_out, &nlev)) return -1;
  if (multi_gather_rows(m, 0, src, ld_out, 0, nlev, out)) return -1;
  return multi_gather_finish(m);
  });
}

// output windows inside the step launches: every shard keeps its columns' records (and the same bookkeeping: the
// shards run the same steps); a record is gathered into 3-D order like window_fetch's fields
int mckpp_hip_multi_window_schedule(mckpp_hip_multi_handle m, int sched, int nt_origin, int period, int nrec,
                                    const int32_t *fields, const uint32_t *ops, int32_t nfields)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_schedule(x, sched, nt_origin, period, nrec, fields, ops, nfields); });
}
// a zoomed schedule: every shard checks the whole zoom and keeps rows for the listed points it owns
int mckpp_hip_multi_window_schedule_zoom(mckpp_hip_multi_handle m, int sched, int nt_origin, int period, int nrec,
                                         const int32_t *fields, const uint32_t *ops, int32_t nfields, const mckpp_win_zoom_c *zoom)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_schedule_zoom(x, sched, nt_origin, period, nrec, fields, ops, nfields, zoom); });
}
// the zoom of shard 0 (every shard's), ring_bytes summed over the shards
int mckpp_hip_multi_window_zoom(mckpp_hip_multi_handle m, int sched, int64_t *npoints, int32_t *lev0, int32_t *nlev, int64_t *ring_bytes)
{
  return entry(__func__, m, [&]() -> int {
  int64_t sum = 0;
  for (auto *x : m->ctx) {
    int64_t b = 0;
    if (mckpp_hip_window_zoom(x, sched, npoints, lev0, nlev, &b)) return -1;
    sum += b;
  }
  if (ring_bytes) *ring_bytes = sum;
  return 0;
  });
}
int mckpp_hip_multi_window_record_fetch(mckpp_hip_multi_handle m, int sched, int64_t rec, int field, int op, double *out)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  if (!out) return fail("%s: null argument", who);
  if (m->npts <= 0) return fail("%s: nothing uploaded", who);
  const int ndev = (int)m->ctx.size();
  std::vector<const double *> src(ndev, nullptr);
  int ld_out = 0, nlev = 0;
  for (int d = 0; d < ndev; ++d)
    if (win_record(m->ctx[d], who, sched, rec, field, op, &src[d], &ld_out, &nlev)) return -1;
  multi_rows z;
  if (m->ctx[0]->wsched[sched].listed) {
    z.npoints = m->ctx[0]->wsched[sched].npoints;
    for (auto *x : m->ctx) { z.nrow.push_back(x->wsched[sched].nrow); z.map.push_back(&x->wsched[sched].rowpos); }
  }
  if (multi_gather_rows(m, 0, src, ld_out, 0, nlev, out, nullptr, 0, z.map.empty() ? nullptr : &z)) return -1;
  return multi_gather_finish(m);
  });
}
int mckpp_hip_multi_window_record_release(mckpp_hip_multi_handle m, int sched, int64_t upto_rec)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_window_record_release(x, sched, upto_rec); });
}
int mckpp_hip_multi_window_records(mckpp_hip_multi_handle m, int sched, int64_t *first_kept, int64_t *last_complete)
{
  return entry(__func__, m, [&]() -> int { return mckpp_hip_window_records(m->ctx[0], sched, first_kept, last_complete); });
}

// ---- the export (mckpp_hip_window_export) over all shards
extern "C++" {
namespace {
template <class T>
void export_merge_t(int64_t npts, int nlev, T land, int nsh, const int64_t *ncol, const int32_t *const *points,
                    const void *const *planes, T *out, const unsigned char *covered)
{
  for_columns(npts, [&](int64_t i0, int64_t i1) {
    for (int l = 0; l < nlev; ++l)
      for (int64_t i = i0; i < i1; ++i)
        if (!covered[i]) out[(int64_t)l * npts + i] = land;
  });
  for (int d = 0; d < nsh; ++d) {
    const int64_t n = ncol[d];
    const T *p = static_cast<const T *>(planes[d]);
    const int32_t *pt = points[d];
    for_columns(n, [&](int64_t c0, int64_t c1) {
      for (int l = 0; l < nlev; ++l)
        for (int64_t c = c0; c < c1; ++c) out[(int64_t)l * npts + pt[c]] = p[(int64_t)l * n + c];
    });
  }
}

void export_merge(int64_t npts, int nlev, int dtype, double land, int nsh, const int64_t *ncol, const int32_t *const *points,
                  const void *const *planes, void *out, const unsigned char *covered)
{
  if (dtype == MCKPP_EXP_F32) export_merge_t<float>(npts, nlev, (float)land, nsh, ncol, points, planes, static_cast<float *>(out), covered);
  else export_merge_t<double>(npts, nlev, land, nsh, ncol, points, planes, static_cast<double *>(out), covered);
}

// which points belong to a shard; -1 for a point outside the grid
int export_covered(int64_t npts, int nsh, const int64_t *ncol, const int32_t *const *points, std::vector<unsigned char> &covered)
{
  covered.assign((size_t)npts, 0);
  for (int d = 0; d < nsh; ++d)
    for (int64_t c = 0; c < ncol[d]; ++c) {
      const int64_t i = points[d][c];
      if (i < 0 || i >= npts) return -1;
      covered[(size_t)i] = 1;
    }
  return 0;
}
}  // namespace
}  // extern "C++"

int mckpp_host_export_merge(int64_t npts, int32_t nlev, int32_t dtype, double land_value, int32_t nshards, const int64_t *ncol,
                            const int32_t *const *points, const void *const *planes, void *out)
{
  return entry(__func__, [&, who = __func__]() -> int {
  if (npts < 0 || nlev < 1 || nshards < 0 || (nshards > 0 && (!ncol || !points || !planes)) || (npts > 0 && !out))
    return fail("%s: bad argument (npts=%lld nlev=%d nshards=%d)", who, (long long)npts, nlev, nshards);
  if (dtype != MCKPP_EXP_F64 && dtype != MCKPP_EXP_F32) return fail("%s: dtype %d (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", who, dtype);
  for (int d = 0; d < nshards; ++d)
    if (ncol[d] < 0 || (ncol[d] > 0 && (!points[d] || !planes[d]))) return fail("%s: shard %d: bad argument (ncol=%lld)", who, d, (long long)ncol[d]);
  std::vector<unsigned char> covered;
  if (export_covered(npts, nshards, ncol, points, covered)) return fail("%s: a point outside 0..%lld", who, (long long)npts - 1);
  export_merge(npts, nlev, dtype, land_value, nshards, ncol, points, planes, out, covered.data());
  return 0;
  });
}

int mckpp_hip_multi_window_export(mckpp_hip_multi_handle m, int sched, int dtype, double land_value)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  const bool compact = m->ctx.size() > 1;
  for (auto *x : m->ctx)
    if (exp_set(x, who, sched, dtype, land_value, compact) != 0) {   // all shards or none
      const std::string why = g_err;
      for (auto *y : m->ctx)
        if (sched >= 0 && sched < MCKPP_WIN_SCHEDULES && !y->wsched[sched].fields.empty()) exp_set(y, who, sched, MCKPP_EXP_OFF, 0.0, compact);
      return fail("%s", why.c_str());
    }
  return 0;
  });
}

int mckpp_hip_multi_window_export_layout(mckpp_hip_multi_handle m, int sched, int32_t *nplanes, int32_t *field, int32_t *op,
                                         int32_t *nlev, int64_t *offset_bytes, int64_t *record_bytes)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  return exp_layout_out(m->ctx[0], who, sched, nplanes, field, op, nlev, offset_bytes, record_bytes);
  });
}

// every shard's copy into the pinned staging is started before any is waited for; the host then merges
static int multi_exp_fetch(mckpp_hip_multi *m, const char *who, int sched, int64_t rec, bool plane, int field, int op, void *out,
                           int64_t out_bytes)
{
  if (!out) return fail("%s: null argument", who);
  const int ndev = (int)m->ctx.size();
  if (ndev == 1) return exp_fetch(m->ctx[0], who, sched, rec, plane, field, op, out, out_bytes);
  if (m->npts <= 0) return fail("%s: nothing uploaded", who);
  size_t k = 0;
  for (auto *x : m->ctx)
    if (exp_check(x, who, sched, rec, plane, field, op, &k)) return -1;
  const auto &w0 = m->ctx[0]->wsched[sched];
  const int dtype = w0.ex.dtype;
  std::vector<win_sched_t::exp_plane> gp;   // the layout over all points
  size_t grb = 0;
  int maxlev = 0;
  const int64_t npoints = w0.npoints;   // (the same list on every shard)
  if (exp_layout(m->ctx[0], w0, npoints, dtype, gp, grb, maxlev)) return -1;
  if (!plane && out_bytes < (int64_t)grb)
    return fail("%s: out_bytes %lld, but a record of schedule %d takes %zu bytes", who, (long long)out_bytes, sched, grb);
  std::vector<size_t> at((size_t)ndev, 0), nb((size_t)ndev, 0);
  size_t total = 0;
  for (int d = 0; d < ndev; ++d) {
    const auto &x = m->ctx[d]->wsched[sched].ex;
    nb[(size_t)d] = plane ? (size_t)x.npts * (size_t)x.planes[k].nlev * exp_elem(dtype) : x.record_bytes;
    at[(size_t)d] = total;
    total += (nb[(size_t)d] + 255) & ~(size_t)255;
  }
  HIPCHK(m->h_exp.reserve(total, hipHostMallocPortable));
  int rc = 0;
  for (int d = 0; d < ndev && rc == 0; ++d) {
    const auto &w = m->ctx[d]->wsched[sched];
    rc = exp_copy_start(m->ctx[d], w, rec, plane ? (size_t)w.ex.planes[k].offset : 0, nb[(size_t)d], m->h_exp + at[(size_t)d]);
  }
  for (auto *x : m->ctx) if (exp_copy_finish(x)) return -1;
  if (rc) return -1;
  std::vector<int64_t> ncol((size_t)ndev);
  std::vector<const int32_t *> points((size_t)ndev);
  std::vector<const void *> planes((size_t)ndev);
  for (int d = 0; d < ndev; ++d) {   // a shard's rows and where they go on the point axis
    const auto &w = m->ctx[d]->wsched[sched];
    ncol[(size_t)d] = w.nrow; points[(size_t)d] = win_host_map(m->ctx[d], w).data();
  }
  std::vector<unsigned char> covered;
  if (export_covered(npoints, ndev, ncol.data(), points.data(), covered)) return fail("%s: a shard's point outside the grid", who);
  for (size_t q = plane ? k : 0; q < (plane ? k + 1 : gp.size()); ++q) {
    for (int d = 0; d < ndev; ++d)
      planes[(size_t)d] = m->h_exp + at[(size_t)d] + (plane ? 0 : (size_t)m->ctx[d]->wsched[sched].ex.planes[q].offset);
    export_merge(npoints, gp[q].nlev, dtype, w0.ex.land, ndev, ncol.data(), points.data(), planes.data(),
                 static_cast<char *>(out) + (plane ? 0 : (size_t)gp[q].offset), covered.data());
  }
  return 0;
}

int mckpp_hip_multi_window_export_fetch(mckpp_hip_multi_handle m, int sched, int64_t rec, int field, int op, void *out)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return multi_exp_fetch(m, who, sched, rec, true, field, op, out, 0); });
}
int mckpp_hip_multi_window_export_fetch_record(mckpp_hip_multi_handle m, int sched, int64_t rec, void *out, int64_t out_bytes)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return multi_exp_fetch(m, who, sched, rec, false, 0, 0, out, out_bytes); });
}

// one file per shard: <path>.<d>of<ndev>
static std::string shard_path(const char *path, int d, int ndev)
{
  return std::string(path) + "." + std::to_string(d) + "of" + std::to_string(ndev);
}
int mckpp_hip_multi_save_restart(mckpp_hip_multi_handle m, const char *path)
{
  return entry(__func__, m, [&]() -> int {
  if (!path) return fail("mckpp_hip_multi_save_restart: null argument");
  const int ndev = (int)m->ctx.size();
  for (int d = 0; d < ndev; ++d)
    if (m->ctx[d]->ncol > 0 && mckpp_hip_save_restart(m->ctx[d], shard_path(path, d, ndev).c_str()) != 0) return -1;
  return 0;
  });
}
// the files must have been written by a handle with the same number of shards over the same land mask: every
// shard's column map is checked against the one the current upload gave it before anything is replaced
int mckpp_hip_multi_load_restart(mckpp_hip_multi_handle m, const char *path)
{
  return entry(__func__, m, [&]() -> int {
  if (!path) return fail("mckpp_hip_multi_load_restart: null argument");
  if (m->npts <= 0) return fail("mckpp_hip_multi_load_restart: upload the state first (the shards' column maps come from it)");
  const int ndev = (int)m->ctx.size();
  for (int d = 0; d < ndev; ++d) {   // pass 1: headers and column maps only
    mckpp_hip_ctx *x = m->ctx[d];
    if (x->ncol == 0) continue;
    const std::string sp = shard_path(path, d, ndev);
    FILE *f = fopen(sp.c_str(), "rb");
    if (!f) return fail("mckpp_hip_multi_load_restart: cannot open %s", sp.c_str());
    restart_header hd{};
    std::vector<int> ipt;
    bool ok = fread(&hd, sizeof hd, 1, f) == 1 && memcmp(hd.magic, kRestartMagic, 8) == 0 && hd.ncol == x->ncol && hd.npts == x->npts;
    if (ok) { ipt.resize((size_t)hd.ncol); ok = fread(ipt.data(), sizeof(int), ipt.size(), f) == ipt.size() && ipt == x->ipt; }
    fclose(f);
    if (!ok) return fail("mckpp_hip_multi_load_restart: %s does not belong to shard %d of %d of the uploaded columns", sp.c_str(), d, ndev);
  }
  for (int d = 0; d < ndev; ++d)
    if (m->ctx[d]->ncol > 0 && mckpp_hip_load_restart(m->ctx[d], shard_path(path, d, ndev).c_str()) != 0) return -1;
  return 0;
  });
}

// restart snapshots inside the step launches (mckpp_hip_restart_schedule) over all shards: every shard keeps the
// snapshots of its own columns (and the same bookkeeping: the shards run the same steps); a snapshot is one file per
// shard, named as multi_save_restart names them, and multi_load_restart reads them
int mckpp_hip_multi_restart_schedule(mckpp_hip_multi_handle m, int nt_origin, int period, int nslots)
{
  return entry(__func__, m, [&]() -> int {
  for (auto *x : m->ctx)
    if (mckpp_hip_restart_schedule(x, nt_origin, period, nslots) != 0) {   // all shards or none
      const std::string why = g_err;
      for (auto *y : m->ctx) mckpp_hip_restart_schedule(y, 1, 0, 0);
      return fail("%s", why.c_str());
    }
  return 0;
  });
}
int mckpp_hip_multi_restart_snapshots(mckpp_hip_multi_handle m, int64_t *first_kept, int64_t *last_complete)
{
  return entry(__func__, m, [&]() -> int { return mckpp_hip_restart_snapshots(m->ctx[0], first_kept, last_complete); });
}
int mckpp_hip_multi_restart_snapshot_save(mckpp_hip_multi_handle m, int64_t snap, const char *path)
{
  return entry(__func__, m, [&]() -> int {
  if (!path) return fail("mckpp_hip_multi_restart_snapshot_save: null argument");
  const int ndev = (int)m->ctx.size();
  for (int d = 0; d < ndev; ++d)
    if (m->ctx[d]->ncol > 0 && mckpp_hip_restart_snapshot_save(m->ctx[d], snap, shard_path(path, d, ndev).c_str()) != 0) return -1;
  return 0;
  });
}
int mckpp_hip_multi_restart_snapshot_release(mckpp_hip_multi_handle m, int64_t upto_snap)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_restart_snapshot_release(x, upto_snap); });
}

// the step log (mckpp_hip_step_log) over all shards: one log of `capacity` records per shard; the counts add up, the
// ORs are ORed, and fetch merges the shards' records (their points are the caller's already) and sorts them
int mckpp_hip_multi_step_log(mckpp_hip_multi_handle m, int64_t capacity, int min_passes)
{
  return entry(__func__, m, [&]() -> int {
  for (auto *x : m->ctx)
    if (mckpp_hip_step_log(x, capacity, min_passes) != 0) {   // all shards or none
      const std::string why = g_err;
      for (auto *y : m->ctx) mckpp_hip_step_log(y, 0, 0);
      return fail("%s", why.c_str());
    }
  return 0;
  });
}
int mckpp_hip_multi_step_log_count(mckpp_hip_multi_handle m, int64_t *n_events, int64_t *n_stored, int32_t *status_or)
{
  return entry(__func__, m, [&]() -> int {
  int64_t ne = 0, ns = 0;
  int32_t so = 0;
  for (auto *x : m->ctx) {
    int64_t a = 0, b = 0;
    int32_t c = 0;
    if (mckpp_hip_step_log_count(x, &a, &b, &c) != 0) return -1;
    ne += a; ns += b; so |= c;
  }
  if (n_events) *n_events = ne;
  if (n_stored) *n_stored = ns;
  if (status_or) *status_or = so;
  return 0;
  });
}
int mckpp_hip_multi_step_log_fetch(mckpp_hip_multi_handle m, int64_t n, int32_t *nt, int32_t *point, int32_t *status,
                                   int32_t *npasses)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  std::vector<log_event> all, ev;
  for (auto *x : m->ctx) {
    if (x->slog.cap == 0) return fail("%s: no step log is set", who);
    int64_t stored = 0;
    if (log_read_ctl(x, nullptr, &stored, nullptr) || log_fetch_raw(x, who, stored, ev)) return -1;
    all.insert(all.end(), ev.begin(), ev.end());
  }
  if (n < 0 || n > (int64_t)all.size())
    return fail("%s: n=%lld (%lld records are stored)", who, (long long)n, (long long)all.size());
  std::sort(all.begin(), all.end(), log_before);
  all.resize((size_t)n);
  return log_deliver(all, nt, point, status, npasses);
  });
}
int mckpp_hip_multi_step_log_clear(mckpp_hip_multi_handle m)
{
  return multi_each(__func__, m, [&](auto *x) { return mckpp_hip_step_log_clear(x); });
}

// ---- the device-array interface and what follows it (mckpp_hip_device.h, _device_records.h, _reduce.h, _put.h, _vaxis.h,
// _hgrid.h, _remap.h) over all shards: each call is its one body, given the shards as its group.  The event on the
// caller's stream is the handle's, on the device of the caller's arrays.
extern "C++" {
namespace {
ctx_group shards(mckpp_hip_multi *m) { return ctx_group{m->ctx.data(), (int)m->ctx.size(), 2, &m->ev_caller, &m->ev_caller_dev}; }
}  // namespace
}  // extern "C++"

int mckpp_hip_multi_fluxes_dev(mckpp_hip_multi_handle m, int ntime, const double *const fields[8], int l_rest, double flsn,
                               double el, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return fluxes_dev(shards(m), who, ntime, fields, l_rest, flsn, el, producer_stream); });
}

int mckpp_hip_multi_flux_ring_put_dev(mckpp_hip_multi_handle m, int rec, const double *const fields[8], void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return flux_ring_put_dev(shards(m), who, rec, fields, producer_stream); });
}

int mckpp_hip_multi_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_dev_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return fetch_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_records_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_dev_record_plane_c *planes,
                                void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return records_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_reduce_weights(mckpp_hip_multi_handle m, const double *point_w, const double *level_w, const double *iface_w)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  for (auto *x : m->ctx)   // (the first shard's checks are every shard's: nothing is replaced unless all can be)
    if (reduce_weights_set(x, who, point_w, level_w, iface_w)) return -1;
  return 0;
  });
}

int mckpp_hip_multi_records_reduce_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_reduce_plane_c *planes,
                                       void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return records_reduce(shards(m), who, nplanes, planes, true, consumer_stream); });
}

int mckpp_hip_multi_records_reduce_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_reduce_plane_c *planes)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return records_reduce(shards(m), who, nplanes, planes, false, nullptr); });
}

int mckpp_hip_multi_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return put_planes(shards(m), who, nplanes, planes, true, producer_stream); });
}

int mckpp_hip_multi_put_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_put_plane_c *planes)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return put_planes(shards(m), who, nplanes, planes, false, nullptr); });
}

// an axis on every shard
int mckpp_hip_multi_vaxis_define(mckpp_hip_multi_handle m, int axis, int32_t n, const double *z)
{
  return multi_each(__func__, m, [&, who = __func__](auto *x) { return vaxis_define(x, who, axis, n, z); });
}

int mckpp_hip_multi_vaxis_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vaxis_put(shards(m), who, nplanes, planes, true, producer_stream); });
}

int mckpp_hip_multi_vaxis_put_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_put_plane_c *planes)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vaxis_put(shards(m), who, nplanes, planes, false, nullptr); });
}

int mckpp_hip_multi_vaxis_init_profiles_dev(mckpp_hip_multi_handle m, const mckpp_vaxis_profiles_c *p, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vaxis_init_profiles(shards(m), who, p, true, producer_stream); });
}

int mckpp_hip_multi_vaxis_init_profiles_host(mckpp_hip_multi_handle m, const mckpp_vaxis_profiles_c *p)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vaxis_init_profiles(shards(m), who, p, false, nullptr); });
}

int mckpp_hip_multi_vaxis_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_dev_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vaxis_fetch_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

// a grid on every shard
int mckpp_hip_multi_hgrid_define(mckpp_hip_multi_handle m, int grid, int64_t n, const mckpp_hgrid_table_c *in, const mckpp_hgrid_table_c *out)
{
  return multi_each(__func__, m, [&, who = __func__](auto *x) { return hgrid_define(x, who, grid, n, in, out); });
}

// shard 0's out table is that of the union of the shards' columns; the in tables' padded sizes add up
int mckpp_hip_multi_hgrid_info(mckpp_hip_multi_handle m, int grid, int64_t info[6])
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  if (!info) return fail("%s: null argument", who);
  int64_t padded_in = 0;
  for (auto *x : m->ctx) {
    if (!hgrid_of(x, who, "grid", grid)) return -1;
    if (x == m->ctx[0] && !x->hg[grid].out.ptr.empty() && group_hgrid_out(shards(m), who, grid)) return -1;
    if (hgrid_info(x, who, grid, info, true)) return -1;
    padded_in += info[3];
  }
  if (hgrid_info(m->ctx[0], who, grid, info, true)) return -1;
  info[3] = padded_in;
  return 0;
  });
}

int mckpp_hip_multi_hgrid_fluxes_dev(mckpp_hip_multi_handle m, int grid, int ntime, const double *const fields[8], int l_rest,
                                     double flsn, double el, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int {
  return fluxes_dev(shards(m), who, ntime, fields, l_rest, flsn, el, producer_stream, &grid);
  });
}

int mckpp_hip_multi_hgrid_flux_ring_put_dev(mckpp_hip_multi_handle m, int grid, int rec, const double *const fields[8], void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return flux_ring_put_dev(shards(m), who, rec, fields, producer_stream, &grid); });
}

int mckpp_hip_multi_hgrid_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hgrid_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return hgrid_fetch_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_remap_records_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_remap_record_plane_c *planes,
                                      void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return remap_records_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_remap_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_remap_put_plane_c *planes,
                                  void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return remap_put_dev(shards(m), who, nplanes, planes, producer_stream); });
}

int mckpp_hip_multi_hv_fetch_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_plane_c *planes, void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return hv_fetch_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_hv_put_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_put_plane_c *planes, void *producer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return hv_put_dev(shards(m), who, nplanes, planes, producer_stream); });
}

int mckpp_hip_multi_vrecords_vaxis_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes,
                                       void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vrecords_vaxis(shards(m), who, nplanes, planes, true, consumer_stream); });
}

int mckpp_hip_multi_vrecords_vaxis_host(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_vaxis_record_plane_c *planes)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vrecords_vaxis(shards(m), who, nplanes, planes, false, nullptr); });
}

int mckpp_hip_multi_vrecords_hv_dev(mckpp_hip_multi_handle m, int32_t nplanes, const mckpp_hv_record_plane_c *planes,
                                    void *consumer_stream)
{
  return entry(__func__, m, [&, who = __func__]() -> int { return vrecords_hv_dev(shards(m), who, nplanes, planes, consumer_stream); });
}

int mckpp_hip_multi_dev_fence(mckpp_hip_multi_handle m, void *stream)
{
  return entry(__func__, m, [&]() -> int { return dev_fence(shards(m), stream); });
}

// the caller's arrays pinned on behalf of this handle go back to pageable memory (before the caller frees them)
int mckpp_hip_multi_release_host_arrays(mckpp_hip_multi_handle m)
{
  return entry(__func__, m, [&]() -> int {
  for (auto *x : m->ctx) { HIPCHK(hipSetDevice(x->device)); if (xfer_finish(x)) return -1; unpin_all(x); }
  return 0;
  });
}

}  // extern "C"
