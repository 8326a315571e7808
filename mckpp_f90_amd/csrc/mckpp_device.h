// mckpp_device.h - shared between the HIP kernels and the host runtime.
//
// Device-resident layout (see DESIGN.md "Data layout in HBM"):
//   level arrays   double[ncol][ld]     ld = 64*LPL, level-fastest, one row
//                                        per water column (512 B at nz<=61)
//     profiles (U,V,T,S,Us*,Xs*,U_init)  element j  <-> reference level k=j+1
//     diagnostics (rho,cp,dif*,wU,wX...) element k  <-> reference index k
//   column record  double cs[ncol][MCKPP_CS]   (scalars in/out, in place)
//                  int    ci[ncol][MCKPP_CI]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MCKPP_CS 24
#define MCKPP_CI 8
#define MCKPP_XS 8
enum { XS_RELAX_SST = 0, XS_SST0, XS_FCORR_TWOD, XS_RELAX_SAL, XS_RELAX_OCNT };

// cs[] slots
enum {
  CS_F = 0, CS_SSURF, CS_SREF, CS_SSREF, CS_OCDEPTH,
  CS_SFLUX1, CS_SFLUX2, CS_SFLUX3, CS_SFLUX4, CS_SFLUX5, CS_SFLUX6,
  CS_HMIXD0, CS_HMIXD1, CS_HMIX, CS_KMIX, CS_UREF, CS_VREF, CS_TREF,
  CS_RESET, CS_DAMPU, CS_DAMPV, CS_FREEZE, CS_FCORR, CS_SPARE1
};
// ci[] slots
enum { CI_OLD = 0, CI_NEW, CI_JERLOV, CI_INITFLAG, CI_STATUS, CI_NPASS, CI_LOCEAN, CI_IPT };

// STEP: ocnstep + check_profile; INIT: initial vmix + seeds (initialize_ocean.F90); PASS: one vmix + ocnint
// (configs[1]); VMIX: mckpp_physics_verticalmixing alone - diagnostics and hmix/kmix only, state untouched
enum { MCKPP_MODE_STEP = 0, MCKPP_MODE_INIT = 1, MCKPP_MODE_PASS = 2, MCKPP_MODE_VMIX = 3 };

// The kernel parameter block, once with plain pointers (host code, by-value kernel arguments) and once with
// pointers typed as global memory: a pointer that a kernel loads from the block in memory is otherwise a generic
// pointer - flat instructions, 64-bit VGPR address arithmetic, LDS waits tied to memory traffic - whereas
// through mckpp_kparams_dev (same layout) every access is a global_load / global_store.
template <class T> using mckpp_ptr_plain = T *;
template <class T> using mckpp_ptr_global = __attribute__((address_space(1))) T *;

// Output windows accumulated by the column kernel itself (mckpp_hip_window_schedule): one entry per (schedule, field).
// The field is read as k_out_sample reads it - element off + l of row c (row length ld), plus the column's Sref if
// add_sref - and folded into the record of the window the step belongs to: window w = (nt - origin) / period, ring slot
// w % nrec; operation j of the entry (the j-th set bit of ops: sum for the mean, min, max, last) at
// acc + (slot * nops + j) * plane + r * ld_out + l, r the column's row of the record.
// A zoomed schedule (mckpp_hip_window_schedule_zoom) keeps rows for its listed columns only: `row` is its table
// int[ncol], resident column -> row, or -1 for a column outside the list, whose items pass the entry by.  Null: row =
// column.  Its level range needs nothing here: the host adds lev0 to `off` and gives the zoomed count as nlev.
#define MCKPP_WIN_ENTRIES 64
template <template <class> class P>
struct mckpp_win_t {
  P<const double> src;
  P<double> acc;
  P<const int> row;       // null, or the zoom's table: column -> row of the record, -1: not kept
  long long plane;        // doubles of one operation's record: rows * ld_out
  int ld, off, nlev, add_sref, ld_out;
  int ops, nops;          // MCKPP_WIN_* mask and its number of bits
  int origin, period, nrec;
};

// One column-step's selection of one ancillary kind (mckpp_kparams_t::anc_sel): offsets in doubles from the kind's records
#define MCKPP_ANC_KINDS 7
enum { ANC_SST0 = 0, ANC_FCORR_TWOD, ANC_FCORR_WITHZ, ANC_SFCORR_WITHZ, ANC_OCNT_CLIM, ANC_SAL_CLIM, ANC_BOTTOM_TEMP };
struct mckpp_anc_sel { long long off_prev, off_next; double w_prev, w_next; };

// A record of the step log: {nt, resident column, status word, passes} of one column-step, one 16-byte store
typedef int mckpp_log_rec __attribute__((ext_vector_type(4)));

template <template <class> class P>
struct mckpp_kparams_t {
  int nz, nzp1, ncol, ld;
  int ntime, itermax, mode, diag;
  int L_SSref, LDD, clim_present;
  int l2pre;      // L2 works from per-layer terms formed once per column (deep reference-level sums; host-chosen)
  double hmixtolfrac, dto, grav, vonk, sice;
  double Vtc;     // bldepth_mod.F90:91, host-evaluated
  double cg;      // blmix_mod.F90:62, host-evaluated (libm pow)
  double dm_nz;   // dm(NZ)
  // constants, device pointers; Fortran-indexed, padded to ldc doubles
  P<const double> zm, hm, tri0, tri1;
  P<const double> swfrac_tab;  // [6][ldc]  swfrac(k), k=1..nzp1, per Jerlov type
  P<const double> swdk_tab;    // [6][ldc]  swdk_opt(k), k=0..nz
  int ldc;
  int LRI;        // rimix (kppmix_mod.F90:72-74); .FALSE.: the interior diffusivities stay zero, Rig is not formed
  int solver_mode;   // 0: tridiagonal sweeps in the reference's order (solvers.F90:112-161); 1: two-ended elimination (opt-in)
  int l3cap;      // > 0: L3 forms the bulk Richardson numbers at most down to this level before the scan asks for the
                  // rest (MCKPP_L3_CAP, tests: the second round of the scan on every pass)
  // How far down L3 forms them (k_column_ps: M0, scan_result; read on the manager wave only)
  int first_margin;   // >= 0: a column's first pass of a step goes down to the kmix its previous step left plus this many
                      // levels (MCKPP_FIRST_MARGIN); < 0: to every level (MCKPP_FIRST_GUESS=0)
  int scan_rule;      // bits 0-15: later passes go down to the level the scan of the pass before ended at plus this many
                      // (MCKPP_GUESS_MARGIN); bit 16: a scan that runs out of levels with every column across counts as
                      // stopped (not under MCKPP_FIRST_GUESS=0)
  P<const double> wtab;        // [(NJ+2)][(NI+2)] pairs {wmt, wst}
  // state
  P<double> U, V, T, S;
  P<double> Us[2], Vs[2], Ts[2], Ss[2];
  P<const double> U_init, V_init;
  P<double> cs;
  P<int> ci;
  P<int> qhead;   // column queue head for the persistent cooperative kernel (zeroed per launch)
  int nsteps_launch;   // model steps this launch takes every column through (1: the step-per-launch path)
  int nqueues;         // nsteps_launch > 1: queues = XCDs of the device (qhead[0..nqueues-1]); column c is in queue c mod nqueues
  int xcc_queue[16];   // hardware XCC id -> queue index
  // forced run in one launch (mckpp_hip_run_forced): the flux records and how a step finds its own
  P<const double> series;   // [nrec][8][ncol]: taux, tauy, swf, lwf, lhf, shf, rain, snow; null: the forcing is what cs holds
  int series_rec0, ndtocn, l_rest;
  int series_nring;   // > 0: `series` is a ring of that many slots [8][ncol] (mckpp_hip_flux_ring), record r in slot
                      // r % series_nring, series_rec0 unused; 0: the linear series from record series_rec0 on
  double flsn, el;
  P<int> qowner;  // [16] per queue: 0 free, else hardware XCC id + 1 of the XCD whose workgroups serve it (zeroed per launch)
  P<int> done;    // [ncol] steps of this launch a column has completed, then [ncol] steps of it that have been started
                  // (zeroed per launch; nsteps_launch > 1 only)
  P<unsigned long long> dbg;   // optional [40] phase-cycle accumulators, counts of L3's guesses (diagnostic builds of a run only)
  // optional physics: ext != 0 selects the kernel build that carries it
  int ext, L_RELAX_SST, L_RELAX_CALCONLY, L_FCORR, L_FCORR_WITHZ, L_SFCORR, L_SFCORR_WITHZ;
  int L_RELAX_SAL, L_RELAX_OCNT, L_NO_FREEZE, L_NO_ISOTHERM, L_DAMP_CURR, iso_bot, dt_uvdamp, maxmodeadv;
  double iso_thresh;
  P<const double> dm;      // dm(0:nz)
  P<const double> hsum;    // hsum(n) = hm(1)+...+hm(n), summed in that order (rhsmod's delta)
  P<const double> xs;      // [ncol][MCKPP_XS]: relax_sst, SST0, fcorr_twod, relax_sal, relax_ocnT
  P<const double> fcorr_withz, sfcorr_withz, ocnT_clim, sal_clim;   // profile rows
  P<double> tinc_fcorr, sinc_fcorr, ocnTcorr, scorr;                // diagnostic rows
  P<const int> adv_i;      // [ncol][1+maxmodeadv]: nmodeadv(2), modeadv(:,2)
  P<const double> adv_d;   // [ncol][maxmodeadv]:   advection(:,2)
  // diagnostics (all or none)
  P<double> rho, cp, buoy, talpha, sbeta, difm, difs, dift, ghat;
  P<double> wU1, wU2, wX1, wX2, wX3, wXNT1, Rig, dbloc, Shsq;
  // k_column_ps: the iterate's scratch rows, one block per (workgroup, slot) (mckpp_ps_scratch_doubles)
  P<double> scratch;
  size_t scratch_doubles;
  // Stragglers (k_column_ps, M0 / G_late): columns on their way to itermax are left alone in their workgroup.
  P<int> sync;        // [0] stragglers the device holds right now (zeroed per launch)
  int solo_after;     // a column past this many passes of a try is one (default 12; MCKPP_SOLO_AFTER)
  int view_kmax;      // most slots of a view (0: as many as the workgroup's waves other than the manager's hold items for; MCKPP_VIEW_KMAX)
  int solo_limit;     // workgroups leave their other slots empty for a straggler while the device holds at most this many
                      // (0: never - MCKPP_SOLO=0; default: workgroups / 32, at least 2; MCKPP_SOLO_LIMIT)
  // output windows of MCKPP_MODE_STEP launches (k_column_ps, finish round): nwin entries of the context's device table
  // (0: no schedule, nothing sampled)
  P<const mckpp_win_t<P>> win;
  int nwin;
  // restart snapshots of MCKPP_MODE_STEP launches (mckpp_hip_restart_schedule; k_column_ps, finish round).  A column
  // that has finished step snap_origin + (s+1)*snap_period - 1 copies its restart set into ring slot s % snap_nslots:
  // whole rows (ld doubles) of U, V, T, S, Us/Vs/Ts/Ss(0:1), cp, rho - MCKPP_SNAP_ROWS planes of snap_plane doubles in
  // the order of the restart file - at snap_rows + slot * snap_slot, and its records at snap_cs / snap_ci + slot * ncol
  // records.  snap_period 0: no schedule, nothing copied.
  P<double> snap_rows, snap_cs;
  P<int> snap_ci;
  long long snap_slot, snap_plane;
  int snap_origin, snap_period, snap_nslots;
  // step log of MCKPP_MODE_STEP launches (mckpp_hip_step_log; k_column_ps, finish round).  A column-step that ends with
  // a non-zero status word, or with at least log_min_passes passes (0: status only), is an event: it ORs its status into
  // log_ctl[1], takes the next index from log_ctl[0] and, below log_cap, writes its record there.  log_cap 0: no log.
  P<mckpp_log_rec> log_rec;
  P<int> log_ctl;
  int log_cap, log_min_passes;
  // resident bottom temperature of MCKPP_MODE_STEP launches (mckpp_hip_set_bottomtemp; k_column_ps, finish round): one
  // value per resident column.  Every column-step ends with mckpp_physics_overrides_bottomtemp (overrides.F90:12-24) on
  // its own column, from bot_temp[c].  Null: nothing is set, no override.
  P<const double> bot_temp;
  // ancillary record series of MCKPP_MODE_STEP launches (mckpp_hip_ancillary_schedule).  Bit `kind` of anc_mask: the kind
  // has a schedule, and a column-step reads it not from xs / the rows above / bot_temp but from anc_rec[kind] - records
  // [ncol] (2-D kinds) or [ncol][ld] - through the selection of its own step: entry (nt - anc_nt0) * MCKPP_ANC_KINDS +
  // kind of anc_sel, which the host writes per launch call.  off_next < 0: the record at off_prev as it is; otherwise
  // rec[off_next + i] * w_next + rec[off_prev + i] * w_prev (boundary_interpolate.F90:60, :115).  Nothing is ever
  // rewritten in place: columns of one launch are at different steps.  anc_mask 0: no schedule, the plain pointers.
  P<const mckpp_anc_sel> anc_sel;
  P<const double> anc_rec[MCKPP_ANC_KINDS];
  int anc_mask, anc_nt0;
  // 1 (only with diag != 0; always in the modes other than STEP): every step of the launch is a diagnostic step -
  // something inside the launch reads what the last vmix leaves behind (an output schedule with a diagnostic field, the
  // bottom-temperature override), or MCKPP_LEAN_DIAG=0.  0: with diag != 0 only the launch's last step and the restart
  // schedule's snapshot steps are (k_column_ps, M0); the others store no diagnostics - their column's next step would
  // overwrite them before the host could see them.
  int diag_every;
};
#define MCKPP_SNAP_ROWS 14
using mckpp_kparams = mckpp_kparams_t<mckpp_ptr_plain>;
using mckpp_kparams_dev = mckpp_kparams_t<mckpp_ptr_global>;
using mckpp_win = mckpp_win_t<mckpp_ptr_plain>;
static_assert(sizeof(mckpp_kparams) == sizeof(mckpp_kparams_dev), "same layout");
static_assert(sizeof(mckpp_win) == sizeof(mckpp_win_t<mckpp_ptr_global>), "same layout");

// what the last cooperative-kernel launch looked like (for the residency check of the tests)
struct mckpp_launch_info { int nblocks, threads, max_blocks_per_cu; size_t lds_bytes; };

// launchers
// The column step: packed, stateless-lane cooperative kernel (mckpp_kernels_ps.hip), persistent grid; level
// phases loop over (slot, level) items.  `dp` is a device copy of `p` (every field but ntime is read from it;
// ntime is passed by value)
hipError_t mckpp_launch_column_kernel_ps(const mckpp_kparams &p, const mckpp_kparams *dp, int num_cu,
                                         hipStream_t stream, mckpp_launch_info *info);
size_t mckpp_ps_scratch_doubles(int nzp1, int variant, int num_cu);   // what p.scratch must hold (variant: 0 default physics, 1 optional, 2 optional with double diffusion)
hipError_t mckpp_launch_xcc_probe(unsigned *mask, hipStream_t stream);   // OR of 1 << XCC id over a 4096-workgroup grid
hipError_t mckpp_launch_eos_batch(int64_t n, const double *s, const double *t, const double *p,
                                  double *alpha, double *beta, double *sig0, double *cp,
                                  hipStream_t stream);
hipError_t mckpp_launch_div_batch(int64_t n, const double *num, const double *den, double *q, hipStream_t stream);
hipError_t mckpp_launch_exp_batch(int64_t n, const double *x, double *y, hipStream_t stream);
hipError_t mckpp_launch_bottomtemp(const mckpp_kparams &p, const double *bt, hipStream_t stream);
hipError_t mckpp_launch_fluxes(const mckpp_kparams &p, int ntime, const double *f8, int l_rest, double flsn,
                               double el, hipStream_t stream);
// record slots a download wants as (npts) slabs: doubles of cs[], ints of ci[]
struct mckpp_pack_list { int nd, ni; int dslot[MCKPP_CS]; int islot[MCKPP_CI]; };
hipError_t mckpp_launch_unpack_sflux(const double *slabs, const int *ipt, double *cs, int64_t ncol, int64_t npts, hipStream_t stream);
hipError_t mckpp_launch_pack_records(const double *cs, const int *ci, const int *ipt, int64_t ncol, int64_t npts,
                                     const mckpp_pack_list &l, double *dout, int *iout, hipStream_t stream);
hipError_t mckpp_launch_out_sample(const double *src, int src_ld, int src_off, const double *cs, int add_sref,
                                   int64_t ncol, int nlev, int ld_out, double *sum, double *mn, double *mx, int first,
                                   double *inst, hipStream_t stream);
hipError_t mckpp_launch_window_mean(const double *sum, double *out, size_t n, double count, hipStream_t stream);
// One plane of an export record (mckpp_hip_window_export; k_record_pack): operation `op` (0 mean: sum / period,
// 1 min, 2 max, 3 last) of one field of a schedule.  Ring slot s of the plane is rows [ncol][ld] at src + s *
// slot_stride, elements off .. off + nlev - 1 of a row; it goes to dst_off bytes (a multiple of 256) into the export
// slot, as [nlev][npts] values.
struct mckpp_pack_plane {
  const double *src;
  long long slot_stride, dst_off;
  int ld, off, nlev, op;
};
// all `nplanes` planes of the record in ring slot `ring_slot` into the export slot at dst_slot; maxlev: the most
// levels of a plane; ipt null: point = column; f32: the slot holds floats
hipError_t mckpp_launch_record_pack(const mckpp_pack_plane *tab, int nplanes, int maxlev, int ring_slot, double period,
                                    const int *ipt, int64_t ncol, int64_t npts, void *dst_slot, int f32, hipStream_t stream);
hipError_t mckpp_launch_export_fill(void *p, size_t nelem, double v, int f32, hipStream_t stream);
// The device-array interface (include/mckpp_hip_device.h).  The eight forcing fields as the caller's (npts) device
// arrays: taux, tauy, swf, lwf, lhf, shf, rain, snow.
struct mckpp_dev_fields { const double *f[8]; };
// k_fluxes with the eight values read from `f` through the column map
hipError_t mckpp_launch_fluxes_dev(const mckpp_kparams &p, int ntime, const mckpp_dev_fields &f, const int *ipt, int l_rest,
                                   double flsn, double el, hipStream_t stream);
// `f` through the column map into one slot [8][ncol] of the flux ring
hipError_t mckpp_launch_flux_gather(const mckpp_dev_fields &f, const int *ipt, int64_t ncol, double *slot, hipStream_t stream);
// One plane of mckpp_hip_fetch_dev (k_fetch_planes): elements off .. off + nlev - 1 of the rows [ncol][ld] at src (plus
// the column's Sref: add_sref) go to out(npts, nlev) as doubles or (f32) floats; fill_land: the points of the launch's
// land list get land_value at every level of the plane.
struct mckpp_fetch_plane {
  const double *src;
  void *out;
  double land_value;
  int ld, off, nlev, add_sref, f32, fill_land;
};
#define MCKPP_FETCH_PLANES 64   // most planes of one call (the device table's size)
// all `nplanes` planes of the device table `tab`; maxlev: the most levels of a plane; land[nland]: the points that are
// no resident column (nland 0: no plane fills them)
hipError_t mckpp_launch_fetch_planes(const mckpp_fetch_plane *tab, int nplanes, int maxlev, const int *ipt, int64_t ncol,
                                     int64_t npts, const double *cs, const int *land, int64_t nland, hipStream_t stream);
// One plane of mckpp_hip_records_dev (k_record_planes): a plane of a schedule's record with its own geometry.  src:
// the rows [nrow][ld] of the operation's plane in the record's ring slot; elements off .. off + nlev - 1 of row r go
// to position map[r] of out(npoints, nlev), doubles or (f32) floats; mean: divided by `period` first (k_window_mean's
// division).  fill: the nnorow positions at norow - those of the point axis that are no row - get land_value at
// every level of the plane.
struct mckpp_rec_plane {
  const double *src;
  void *out;
  const int *map;
  const int *norow;
  double period, land_value;
  long long nrow, npoints, nnorow;
  int ld, off, nlev, mean, f32, fill;
};
// all `nplanes` planes of the device table `tab`; maxlev: the most levels of a plane; xtiles: the most 64-entry tiles
// of a plane, rows and - where it fills - non-row positions together
hipError_t mckpp_launch_record_planes(const mckpp_rec_plane *tab, int nplanes, int maxlev, int64_t xtiles, hipStream_t stream);
// One plane of mckpp_hip_records_reduce_dev / _host (include/mckpp_hip_reduce.h states the arithmetic; k_reduce_fill,
// k_reduce_terms, k_reduce_halve, k_reduce_finish): mckpp_rec_plane's rows and geometry, reduced.  axis_op / domain_op:
// MCKPP_RED_*.  wl: the level weights of elements off .. off + nlev - 1 (null: 1.0), wsum their sum W in ascending
// order ((double)nlev without weights), formed by the host; wp: the point weights by point number (null: 1.0), point:
// row -> point number.  A domain-reduced plane sends its terms through `terms`: nslab slabs of n2 doubles - n2 the
// smallest power of two >= the points of the plane's axis -, one per level (one in all behind an axis reduction), and behind them, for an
// average, the slab of the denominator's terms.  `terms` is shard 0's block and `out` the one array under a multi
// handle; fill: this context writes what no row does - the slabs' padding and non-row terms, and land_value at the
// nnorow positions of an axis-only plane.  norows: no shard has a row, every element is land_value.
enum { RED_NONE = 0, RED_SUM, RED_AVERAGE, RED_MIN, RED_MAX };   // MCKPP_RED_* of the header
struct mckpp_red_plane {
  const double *src;
  double *out, *terms;
  const int *map, *point, *norow;
  const double *wl, *wp;
  double period, land_value, wsum;
  long long nrow, nnorow, n2;
  int ld, off, nlev, mean, axis_op, domain_op, nslab, fill, norows;
};
// Most partials of a plane's tree that one workgroup finishes (k_reduce_finish's LDS); the launches take m, a power of
// two 64 .. MCKPP_RED_M: the tree of a slab of more than m terms is halved down to m in place first (k_reduce_halve).
#define MCKPP_RED_M 1024
// one kernel (`phase`) over all `nplanes` planes of the device table `tab`; maxlev: the most results of a domain-reduced
// plane, maxslab: the most slabs, xtiles: the most 64-row tiles of a plane
hipError_t mckpp_launch_reduce(const mckpp_red_plane *tab, int nplanes, int phase, int maxlev, int maxslab, int64_t xtiles,
                               int m, hipStream_t stream);
enum { MCKPP_RED_PHASE_FILL = 0, MCKPP_RED_PHASE_TERMS, MCKPP_RED_PHASE_HALVE, MCKPP_RED_PHASE_FINISH };
// One plane of mckpp_hip_put_dev / _put_host (k_put_planes), mckpp_fetch_plane turned round: in(npts, nlev), doubles or
// (f32) floats, is set into (add: added to) elements off .. off + nlev - 1 of the rows [ncol][ld] at row; sub_sref: a
// set writes the value minus the column's Sref; skip: a value == skip_value leaves its element alone; lv0 / lv1: the
// field's two saved time levels, written too (null: they stay).  ref_slot >= 0: the plane holds level 0, and the thread
// that writes a column's element there restates cs[ref_slot] from it - plus the column's Sref where ref_sref (Ssurf).
struct mckpp_put_plane {
  const void *in;
  double *row, *lv0, *lv1;
  double skip_value;
  int ld, off, nlev, f32, add, skip, sub_sref, ref_slot, ref_sref;
};
#define MCKPP_PUT_PLANES 64   // most planes of one call (the device table's size)
// all `nplanes` planes of the device table `tab`; maxlev: the most levels of a plane
hipError_t mckpp_launch_put_planes(const mckpp_put_plane *tab, int nplanes, int maxlev, const int *ipt, int64_t ncol,
                                   int64_t npts, double *cs, hipStream_t stream);
// The caller's vertical axes (include/mckpp_hip_vaxis.h states the interpolation).  One entry of an axis table, built
// by mckpp_host_vaxis_map: which source levels a target level reads - kin alone (branch 0 above the axis, 1 below it)
// or kin and kin + 1 (branch 2) - and the two numbers of the bracket that depend on the axes alone.
struct mckpp_vaxis_ent { int branch, kin; double t, dz; };
// One plane of mckpp_hip_vaxis_put_dev / _put_host and of the profiles of mckpp_hip_vaxis_init_profiles
// (k_vaxis_put_planes): put.in is in(npts, n_axis) and put.nlev the model's nzp1; level lev of a column takes vinterp of
// the column's input through tab[lev], and put_element does with it what `put` says - whose own skip is 0: `skip` is
// decided on the input side, where the values the branch reads are.  row2 (null: none): rows that take the value too
// (U_init); kelvin (null: none): the word that gets bit 0 where a value written is > 200 and < 400.
struct mckpp_vaxis_put_plane {
  mckpp_put_plane put;
  const mckpp_vaxis_ent *tab;
  double *row2;
  unsigned *kelvin;
  int skip;
};
// One plane of mckpp_hip_vaxis_fetch_dev (k_vaxis_fetch_planes): f.nlev is the caller axis' n, level j of out takes
// vinterp of the row's elements f.off .. f.off + nzp1 - 1 (plus Sref first: f.add_sref) through tab[j].
struct mckpp_vaxis_fetch_plane {
  mckpp_fetch_plane f;
  const mckpp_vaxis_ent *tab;
};
#define MCKPP_VAXIS_PLANES 64   // most planes of one call (the device tables' size)
hipError_t mckpp_launch_vaxis_put_planes(const mckpp_vaxis_put_plane *tab, int nplanes, int nzp1, const int *ipt, int64_t ncol,
                                         int64_t npts, double *cs, hipStream_t stream);
hipError_t mckpp_launch_vaxis_fetch_planes(const mckpp_vaxis_fetch_plane *tab, int nplanes, int maxlev, const int *ipt,
                                           int64_t ncol, int64_t npts, const double *cs, const int *land, int64_t nland,
                                           hipStream_t stream);
// the end of mckpp_hip_vaxis_init_profiles, behind the profiles' planes: the Kelvin rule where *kelvin is set, Sref,
// SSref, X2 = S - Sref, Tref and Ssurf, a wave per column
hipError_t mckpp_launch_vaxis_init_finish(double *T, double *S, int ld, int nzp1, int64_t ncol, double *cs,
                                          const unsigned *kelvin, double tk0, int l_ssref, hipStream_t stream);
// The caller's horizontal grids (include/mckpp_hip_hgrid.h states the arithmetic and the layout).  A weight table on the
// device, the sliced ELL mckpp_host_hgrid_slices builds: slice s - rows 64 s .. 64 s + 63, one wave's - has the width
// (off[s + 1] - off[s]) / 64, entry k of row r is element off[r / 64] + 64 k + r % 64 of idx and w, and len[r] entries
// of row r are loaded.
struct mckpp_hgrid_ell {
  const int64_t *off;
  const int *len;
  const int *idx;
  const double *w;
  int64_t nrows;
};
// k_fluxes_dev / k_flux_gather with each resident column's eight values summed from the caller grid's arrays `f`
// through the in table `t`, whose rows are the resident columns in column order
hipError_t mckpp_launch_hgrid_fluxes(const mckpp_kparams &p, int ntime, const mckpp_hgrid_ell &t, const mckpp_dev_fields &f,
                                     int l_rest, double flsn, double el, hipStream_t stream);
hipError_t mckpp_launch_hgrid_flux_gather(const mckpp_hgrid_ell &t, const mckpp_dev_fields &f, int64_t ncol, double *slot,
                                          hipStream_t stream);
// One plane of mckpp_hip_hgrid_fetch_dev's second stage (k_hgrid_out): level lev of out(t.nrows, nlev), doubles or (f32)
// floats, is the row sum through the out table `t` of stage(npts, nlev)'s level lev; norm: MCKPP_HGRID_NORM_*; fill: a
// caller point without a used entry gets land_value.
struct mckpp_hgrid_plane {
  const double *stage;
  void *out;
  double land_value;
  mckpp_hgrid_ell t;
  int64_t npts;
  int nlev, f32, norm, fill;
};
#define MCKPP_HGRID_PLANES 64   // most planes of one call (the device table's size)
// all `nplanes` planes of the device table `tab`; maxlev: the most levels of a plane, maxn: the most points of a grid
hipError_t mckpp_launch_hgrid_out(const mckpp_hgrid_plane *tab, int nplanes, int maxlev, int64_t maxn, hipStream_t stream);
// One plane of mckpp_hip_remap_put_dev (include/mckpp_hip_remap.h; k_remap_put_planes): put.in is in(n, put.nlev) on a
// caller grid of n points; level lev of resident column c takes the sum of row c of the in table `t` - whose rows are
// the resident columns in column order - over the plane's level lev, and put_element does with it what `put` says.
// put's own skip is 0: `skip` is decided on the input side, where the values the entries read are.  A column with an
// empty row is left alone.
struct mckpp_remap_put_plane {
  mckpp_put_plane put;
  mckpp_hgrid_ell t;
  int64_t n;
  int skip;
};
#define MCKPP_REMAP_PLANES 64   // most planes of one call (the device table's size)
hipError_t mckpp_launch_remap_put_planes(const mckpp_remap_put_plane *tab, int nplanes, int maxlev, int64_t ncol, double *cs,
                                         hipStream_t stream);
// One plane of mckpp_hip_hv_put_dev (include/mckpp_hip_hv.h; k_hv_put_planes): put.in is in(n, n_axis) on a caller grid
// of n points and a caller axis of n_axis levels, put.nlev the model's nzp1.  Level lev of resident column c takes
// vinterp through tab[lev], the axis's in table, of the sums of row c of the in table `t` over the one or two caller
// levels the entry names, and put_element does with it what `put` says.  put's own skip is 0: `skip` is decided on the
// input side, where the values the entries read at those caller levels are.  A column with an empty row is left alone.
struct mckpp_hv_put_plane {
  mckpp_put_plane put;
  mckpp_hgrid_ell t;
  const mckpp_vaxis_ent *tab;
  int64_t n;
  int n_axis, skip;
};
#define MCKPP_HV_PLANES 64   // most planes of one call (the device table's size)
hipError_t mckpp_launch_hv_put_planes(const mckpp_hv_put_plane *tab, int nplanes, int nzp1, int64_t ncol, double *cs,
                                      hipStream_t stream);
// One plane of mckpp_hip_vrecords_vaxis_dev / _host and of the first stage of mckpp_hip_vrecords_hv_dev
// (include/mckpp_hip_vrecords.h; k_vaxis_record_planes): mckpp_rec_plane's rows and geometry with r.nlev the caller
// axis' n: level j of out(npoints, n) takes vinterp through tab[j], the axis's out table, of the row's elements - of a
// mean each divided by r.period first.  tab's kin counts model levels; the row's element 0 is model level lev0 of the
// schedule, so the element read is r.off + kin - lev0 (the host has checked that every one is a kept level).
struct mckpp_vrec_plane {
  mckpp_rec_plane r;
  const mckpp_vaxis_ent *tab;
  int lev0;
};
#define MCKPP_VREC_PLANES 64   // most planes of one call (the device table's size)
// as mckpp_launch_record_planes
hipError_t mckpp_launch_vaxis_record_planes(const mckpp_vrec_plane *tab, int nplanes, int maxlev, int64_t xtiles, hipStream_t stream);
// layout kernels: Fortran (npts-fastest) <-> device rows
hipError_t mckpp_launch_gather_rows(const double *src3d, int64_t npts, int nlev, int lev_off,
                                    const int *ipt, int64_t ncol, double *dst, int ld, int dst_off,
                                    hipStream_t stream);
hipError_t mckpp_launch_scatter_rows(const double *src, int ld, int src_off, const int *ipt,
                                     int64_t ncol, double *dst3d, int64_t npts, int nlev, int lev_off,
                                     hipStream_t stream);
