/*
 * mckpp_hip.h - C-ABI of the MI355X (gfx950) column-physics library.
 *
 * This is the drop-in boundary for MC-KPP's per-column physics step.  The
 * reference (aosprey/mckpp-f90) has no FFI seam of its own: the seam is the
 * Fortran call surface
 *     CALL mckpp_physics_driver()          src/mckpp_physics_driver_mod.F90:15
 *       -> mckpp_physics_ocnstep(kpp_1d_fields, kpp_const_fields)
 *                                          src/mckpp_physics_ocnstep_mod.F90:43
 *       -> mckpp_physics_overrides_check_profile   src/mckpp_physics_overrides.F90:42
 *     CALL mckpp_initialize_ocean_model()  src/mckpp_initialize_ocean.F90:18
 * operating on the module globals kpp_3d_fields / kpp_const_fields
 * (src/mckpp_data_fields.F90:348-349).  The entry points below are what an
 * iso_c_binding module in that code base binds (see INTEGRATION.md and
 * mckpp_f90_amd/fortran/mckpp_hip_binding.F90): plain pointers into the
 * Fortran-owned ALLOCATABLE components, plain sizes, int return codes.
 *
 * Conventions
 *  - every array pointer addresses a Fortran array in its native layout
 *    (column index `ipt` fastest), fp64 / int32 / 4-byte LOGICAL;
 *  - the library never frees or keeps host pointers beyond the call;
 *  - column state is device-resident between mckpp_hip_upload and
 *    mckpp_hip_download;
 *  - all functions return 0 on success, <0 on error (text from
 *    mckpp_hip_last_error()).  Numerical conditions never abort: they are
 *    reported per column through the status bitmask.
 *  - no C++ exception leaves the library - it is an error like any other -
 *    and every error text begins with the function's name (a failed HIP call
 *    is named instead, with its source line).
 *  - not re-entrant; call from one host thread per handle.
 *
 * Every array pointer here is a host pointer.  The companion header
 * mckpp_hip_device.h is the device-array interface: forcing from, and output
 * fields into, arrays in device memory, ordered on the caller's stream.
 */
#ifndef MCKPP_HIP_H
#define MCKPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCKPP_NI 890 /* wmt/wst first extent  = NI+2 (src/mckpp_physics_lookup_mod.F90:20) */
#define MCKPP_NJ 48  /* wmt/wst second extent = NJ+2 (:21) */

/* per-column status bits (replace the reference's stderr warnings / STOP) */
#define MCKPP_ST_ZERO_PIVOT   1  /* src/mckpp_physics_solvers.F90:140-151 (reference STOPs) */
#define MCKPP_ST_LONG_ITER    2  /* src/mckpp_physics_ocnstep_mod.F90:184-191 */
#define MCKPP_ST_RETRIED      4  /* :200-227 instability trap fired at least once */
#define MCKPP_ST_FAILED       8  /* :229-236 ten retries exhausted */
#define MCKPP_ST_DODGY_OLDNEW 16 /* :93-102 */

/* kpp_const_type, hot-path subset (src/mckpp_data_fields.F90:187-346) plus
 * the mckpp_parameters integers the path reads (src/mckpp_parameters.F90). */
typedef struct mckpp_const_c {
  int32_t nz;        /* layers; nzp1 = nz+1 grid points               */
  int32_t nztmax;    /* >= nzp1 (sizes difm/difs/dift/wU/wX/wXNT/ghat) */
  int32_t nsflxs;    /* first flux extent of sflux (9)                */
  int32_t njdt;      /* sflux(npts,nsflxs,5,0:njdt)                   */
  int32_t itermax;   /* 200                                           */
  int32_t LKPP, LRI, LDD, L_SSref;
  int32_t L_RELAX_SST, L_RELAX_CALCONLY, L_FCORR, L_FCORR_WITHZ;
  int32_t L_SFCORR, L_SFCORR_WITHZ, L_RELAX_SAL, L_RELAX_OCNT;
  int32_t L_NO_FREEZE, L_NO_ISOTHERM, L_DAMP_CURR;
  int32_t clim_present; /* ocnT_file/='none' .and. sal_file/='none'   */
  int32_t iso_bot, dt_uvdamp;
  int32_t maxmodeadv; /* second extent of modeadv/advection (6)       */
  int32_t L_ADVECT;   /* prescribed advection on (src/mckpp_initialize_advection_mod.F90:65: nmodeadv=0 otherwise) */
  double hmixtolfrac, dto, grav, vonk, sice, iso_thresh;
  const double *zm;  /* zm(nzp1)                                      */
  const double *hm;  /* hm(nzp1)                                      */
  const double *dm;  /* dm(0:nz)                                      */
  const double *tri; /* tri(0:nztmax,0:1,ngrid): only (:,:,1) is read  */
  const double *wmt; /* wmt(0:891,0:49)                               */
  const double *wst; /* wst(0:891,0:49)                               */
} mckpp_const_c;

/* Pointers into kpp_3d_type components (src/mckpp_data_fields.F90:8-101,
 * extents :353-447).  A NULL pointer means "field not exchanged". */
typedef struct mckpp_state_ptrs_c {
  int64_t npts;
  /* prognostic and saved profiles */
  double *U;       /* U(npts,nzp1,nvel)            */
  double *X;       /* X(npts,nzp1,nsclr)           */
  double *Us;      /* Us(npts,nzp1,nvel,0:1)       */
  double *Xs;      /* Xs(npts,nzp1,nsclr,0:1)      */
  double *U_init;  /* U_init(npts,nzp1,nvel)       */
  double *hmixd;   /* hmixd(npts,0:1)              */
  /* per-column scalars (npts) */
  double *f, *ocdepth, *Sref, *SSref, *Ssurf;
  double *hmix, *kmix, *Tref, *uref, *vref;
  double *reset_flag, *dampu_flag, *dampv_flag, *freeze_flag;
  double *sflux;   /* sflux(npts,nsflxs,5,0:njdt); (:,1:6,5,0) is read */
  int32_t *old, *new_, *jerlov;
  int32_t *l_ocean, *l_initflag, *run_physics; /* 4-byte LOGICAL       */
  /* diagnostics of the last vmix/ocnint pass of the step */
  double *rho, *cp;           /* (npts,0:nzp1tmax)                     */
  double *buoy;               /* (npts,nzp1tmax)                       */
  double *difm, *difs, *dift; /* (npts,0:nztmax)                       */
  double *wU;                 /* (npts,0:nztmax,nvp1)                  */
  double *wX;                 /* (npts,0:nztmax,nsp1)                  */
  double *wXNT;               /* (npts,0:nztmax,nsclr)                 */
  double *ghat;               /* (npts,nztmax)                         */
  double *Rig, *Shsq;         /* (npts,nzp1)                           */
  double *dbloc;              /* (npts,nz)                             */
  double *swfrac;             /* (npts,nzp1)                           */
  double *swdk_opt;           /* (npts,0:nz)                           */
  /* optional forcing corrections / relaxation (src/mckpp_physics_ocnint_mod.F90:97-215,
   * src/mckpp_physics_overrides.F90:42-125); only read when the matching switch is on */
  double *relax_sst, *SST0, *fcorr_twod, *relax_sal, *relax_ocnT; /* (npts)        */
  double *fcorr;              /* (npts) out: diagnosed surface flux correction    */
  double *fcorr_withz, *sfcorr_withz, *ocnT_clim, *sal_clim;      /* (npts,nzp1)  */
  double *tinc_fcorr, *sinc_fcorr, *ocnTcorr, *scorr;             /* (npts,nzp1) out */
  int32_t *nmodeadv;          /* (npts,2)            - column 2 (salinity) is used */
  int32_t *modeadv;           /* (npts,maxmodeadv,2)                               */
  double *advection;          /* (npts,maxmodeadv,2)                               */
} mckpp_state_ptrs_c;

/* field_mask bits for mckpp_hip_download */
#define MCKPP_F_PROFILES 1u /* U, X                                         */
#define MCKPP_F_SAVED    2u /* Us, Xs, hmixd, old, new                      */
#define MCKPP_F_SCALARS  4u /* hmix,kmix,Tref,uref,vref,Ssurf,*_flag        */
#define MCKPP_F_DIAG     8u /* rho..swdk_opt (needs diagnostics enabled)    */
#define MCKPP_F_RESTART  (MCKPP_F_PROFILES | MCKPP_F_SAVED | MCKPP_F_SCALARS)
#define MCKPP_F_ALL      0xFu

typedef struct mckpp_hip_ctx *mckpp_hip_handle;

const char *mckpp_hip_last_error(void);

/* Twelve hex digits identifying the kernel sources this library was built from
 * (measurement bookkeeping: profiles/ records it next to counter values). */
const char *mckpp_hip_build_id(void);
/* The compiler (hipcc --version line) the kernels were built and gate-checked with: the register budget and the
 * hand-scheduled LDS reads of the column kernel are checked on the code THAT compiler generated (tools/check_build.py,
 * run by the library's Makefile); a build made with CHECK=0 carries "-unchecked" in its build id. */
const char *mckpp_hip_build_compiler(void);

/* Number of visible gfx950 devices (<0 on error). */
int mckpp_hip_device_count(void);

/* Create a context on HIP device `device`; copies grid, tri and the lookup
 * tables to the device.  Replaces nothing in the reference: it is the
 * device-side mirror of kpp_const_fields after mckpp_initialize_namelist /
 * mckpp_physics_lookup / the tri() set-up of initialize_ocean.F90:34-43. */
int mckpp_hip_init(const mckpp_const_c *c, int device, mckpp_hip_handle *out);
int mckpp_hip_finalize(mckpp_hip_handle h);

/* Host helpers with no device work (so a caller written in C can build
 * kpp_const_fields): mckpp_physics_lookup (src/mckpp_physics_lookup_mod.F90:11)
 * and the tri() factors (src/mckpp_initialize_ocean.F90:34-43). */
void mckpp_host_lookup(double vonk, double *wmt, double *wst);
void mckpp_host_tri(int32_t nz, int32_t nztmax, double dto, const double *zm,
                    const double *hm, double *tri);

/* 3D -> device: compacts run_physics columns, re-lays column-fastest Fortran
 * arrays into level-fastest padded rows.  Replaces the gather half of
 * mckpp_fields_3dto1d (src/mckpp_types_transfer.F90:15-193), once instead of
 * every step. */
int mckpp_hip_upload(mckpp_hip_handle h, const mckpp_state_ptrs_c *s);

/* New surface forcing: sflux(:,1:6,5,0) as written by mckpp_fluxes
 * (src/mckpp_fluxes_mod.F90:62-69).  `sflux` is the full Fortran array. */
int mckpp_hip_set_forcing(mckpp_hip_handle h, const double *sflux);

/* mckpp_fluxes (src/mckpp_fluxes_mod.F90:35-89) on the device: assembles
 * sflux(:,1:6,5,0) from the eight surface forcing fields (each npts, 3D
 * ordering: taux,tauy,swf,lwf,lhf,shf,rain,snow; kpp_3d_type components of
 * the same names, src/mckpp_data_fields.F90:76-83) for every l_ocean column
 * and refreshes wXNT(:,1) like its mckpp_fluxes_ntflux call (:93-118).
 * l_rest, flsn, el: kpp_const_fields%L_REST, %FLSN, %EL. */
int mckpp_hip_fluxes(mckpp_hip_handle h, int ntime, const double *taux, const double *tauy,
                     const double *swf, const double *lwf, const double *lhf, const double *shf,
                     const double *rain, const double *snow, int l_rest, double flsn, double el);

/* Forced runs without per-step host traffic.  mckpp_hip_set_flux_series keeps `nrec`
 * successive records of the eight surface forcing fields on the device (layout
 * fields[rec][8][npts], field order and meaning as mckpp_hip_fluxes: what
 * kpp_3d_fields%taux..snow hold after the reference's flux reader at each
 * update); record 0 of the array is flux update number `rec0` of the run.
 * mckpp_hip_run_forced then is the reference's time loop without output
 * (src/mckpp_ocean_model_3D.F90:38-58): for nt = nt_first .. nt_first+nsteps-1
 *   IF (MOD(nt-1, ndtocn) == 0) mckpp_fluxes with record (nt-1)/ndtocn
 *   mckpp_physics_driver
 * all on the context's stream; it fails before launching anything if a needed
 * record is not resident.  l_rest, flsn, el as for mckpp_hip_fluxes. */
int mckpp_hip_set_flux_series(mckpp_hip_handle h, int rec0, int nrec, const double *fields);
int mckpp_hip_run_forced(mckpp_hip_handle h, int nt_first, int nsteps, int ndtocn, int l_rest,
                         double flsn, double el);

/* The flux-record ring: the forcing of a long or coupled run streamed in while earlier launches run, instead of a
 * series that a call replaces as a whole.  What arrives is what the reference's loop reads between steps
 * (src/mckpp_ocean_model_3D.F90:44-48) - the eight fields mckpp_fluxes assembles sflux from
 * (src/mckpp_fluxes_mod.F90:35-89) - one record at a time.  Record r lives in slot r % nslots of device memory, a slot
 * being [8][resident columns]; a put overwrites the oldest record.
 *   flux_ring: a ring of nslots empty slots (nslots 0: cancels it, after waiting for the context's stream and the
 *     ring's transfer stream).  Needs an uploaded state.  A ring in place is dropped first, and so is a series of
 *     mckpp_hip_set_flux_series; while a ring is set, set_flux_series is refused.  upload with another column map and
 *     load_restart cancel the ring; output, restart, step-log and ancillary schedules are left alone.
 *   flux_ring_put: `fields`[8][npts] is record `rec` of the run, layout and field order of one record of
 *     set_flux_series.  Records arrive in order: the first put names any rec >= 0, every later one the last plus 1.
 *     The record is compacted to the resident columns into pinned staging and copied into its slot on a transfer stream
 *     of the ring's own - under the launches already queued on the context's stream - behind, on the device, the
 *     launches of the last run_forced call that needed the record the slot held.  Returns without waiting for the
 *     device; `fields` may be rewritten at once.  (The one host wait: the staging has two turns, so a put waits for the
 *     copy of two puts back if that is still in flight.)
 *   flux_ring_records: the resident range, the last min(nslots, records put) records; -1, -1: the ring is empty.
 *   mckpp_hip_run_forced with a ring set checks its flux updates against that range - a record not yet put, or
 *     already overwritten, fails the call before anything is launched, naming steps, records and range - makes the
 *     context's stream wait for the copies of the records it needs, and launches as ever (one launch or a launch per
 *     step), every update step finding its record's slot itself.  A call needs at most nslots records: records must be
 *     resident when their launch starts.  There is no release call: the residency check is the only bookkeeping. */
int mckpp_hip_flux_ring(mckpp_hip_handle h, int nslots);
int mckpp_hip_flux_ring_put(mckpp_hip_handle h, int rec, const double *fields);
int mckpp_hip_flux_ring_records(mckpp_hip_handle h, int *first, int *last);

/* mckpp_physics_overrides_bottomtemp (src/mckpp_physics_overrides.F90:12-24),
 * which mckpp_physics_driver calls after the column loop when
 * kpp_const_fields%L_VARY_BOTTOM_TEMP (src/mckpp_physics_driver_mod.F90:67-71):
 *   tinc_fcorr(ipt,NZP1) = bottom_temp(ipt) - X(ipt,NZP1,1)
 *   ocnTcorr(ipt,NZP1)   = tinc_fcorr(ipt,NZP1)*rho(ipt,NZP1)*cp(ipt,NZP1)/dto
 *   X(ipt,NZP1,1)        = bottom_temp(ipt)
 * on every device-resident column.  `bottom_temp` is kpp_3d_fields%bottom_temp
 * (npts, 3D ordering).  Needs the diagnostics on (rho, cp of the last vmix).
 * Land points are not resident and stay untouched (the reference also rewrites
 * their X(:,NZP1,1), which nothing reads). */
int mckpp_hip_bottomtemp(mckpp_hip_handle h, const double *bottom_temp);

/* The same override from a resident field, inside the launches.  In the reference it is the driver's last act of a
 * step (src/mckpp_physics_driver_mod.F90:67-71, src/mckpp_physics_overrides.F90:12-24): step n+1 starts from the
 * overridden X(:,NZP1,1), and output and restart files, written after the driver, carry it.
 *   set_bottomtemp: `bottom_temp` (npts, 3D ordering) is compacted to the resident columns into a device array of its
 *     own and stays resident until replaced; NULL cancels it.  Allocates and zeroes the correction rows of a
 *     default-physics context, as mckpp_hip_bottomtemp does.  Output, restart and step-log schedules are left alone.
 *     upload and load_restart cancel the field (the column map may change).
 *   While a field is resident every MCKPP_MODE_STEP launch - step, run_forced and their multi_ forms, one launch or a
 *     launch per step - ends each column-step with the three assignments above on its own column, after check_profile
 *     (climatology reset, no-freeze clamp, isotherm reset) and before the launch's windows, snapshots and the
 *     column's next step.  rho and cp are those of the step's last vmix; Xs(:,:,:,new) keeps the step's own value.
 *     init_ocean, vmix_pass and vmix_only never apply it.  Such a launch needs the diagnostics on (rho and cp are
 *     diagnostics): with them off it fails before anything is launched.
 *   mckpp_hip_bottomtemp is refused while a field is resident: the override applied twice zeroes tinc_fcorr(:,NZP1)
 *     and ocnTcorr(:,NZP1).  Drop that call, or cancel the field.
 *   Cadence: the field set here is constant within a launch.  A run that updates bottom_temp every ndtupdbottom steps
 *     (L_UPD_BOTTOM_TEMP of mckpp_boundary_update) either cuts its launches there and calls set_bottomtemp with the new
 *     field between them, or keeps the records resident and schedules them (mckpp_hip_ancillary_schedule with
 *     MCKPP_ANC_BOTTOM_TEMP, below).  The two are mutually exclusive: the second one asked for is refused. */
int mckpp_hip_set_bottomtemp(mckpp_hip_handle h, const double *bottom_temp);

/* Ancillary record series: what mckpp_boundary_update (src/mckpp_boundary_update_mod.F90:24-124, called for every
 * nt /= 1 at src/mckpp_ocean_model_3D.F90:51-55) rewrites at the ndtupd* cadences, and with L_INTERP_OCNT /
 * L_INTERP_SAL every ndt_interp_* steps as a weighted sum of two records (src/mckpp_boundary_interpolate.F90:14-121),
 * inside the launches.  Columns of one launch are at different steps, so nothing is rewritten in place: the records
 * are resident and immutable, and every column-step selects its own record, or pair and weights, from the step it is in.
 *   set_ancillary_series keeps `nrec` records of one kind on the device: records[rec][npts] for the 2-D kinds (SST0,
 *     FCORR_TWOD, BOTTOM_TEMP), records[rec][nzp1][npts] for the others - each record the Fortran array (npts) or
 *     (npts, nzp1) the reference's reader leaves in kpp_3d_fields.  Record 0 of the array is record number `rec0` of
 *     the run.  Compacted to the resident columns; the 3-D kinds re-laid into rows as upload does.  Ordered on the
 *     context's stream behind the launches already queued; `records` may change when the call returns.  A call replaces
 *     the kind's resident records; nrec = 0 frees them (records may then be NULL).
 *   ancillary_schedule: step nt belongs to epoch (nt - nt_origin) / cadence, and epochs[i] describes epoch epoch0 + i:
 *     rec_next < 0: the field of the epoch is record rec_prev as it is, no arithmetic; otherwise it is
 *     record[rec_next]*w_next + record[rec_prev]*w_prev, two products and a sum in that order
 *     (boundary_interpolate.F90:60, :115), each separately rounded.  Interpolated epochs are accepted for OCNT_CLIM and
 *     SAL_CLIM only, as in the reference.  nepochs = 0 cancels the schedule.  Records are named by their number in
 *     the run; which file position the reference's reader would pick (mckpp_get_update_time) stays with the caller,
 *     as for the flux series.  mckpp_host_interp_weights gives the weights.
 *   While a kind has a schedule every MCKPP_MODE_STEP launch - step, run_forced, their multi_ forms, one launch or a
 *     launch per step - reads that kind, for each column-step, from the series through its epoch; the plain resident
 *     copy that update_ancillaries / set_bottomtemp write is left alone and not read by those launches.  The climatology
 *     that a step's check_profile resets to is that step's.  init_ocean, vmix_pass and vmix_only are unaffected.  A launch
 *     with a step before nt_origin, an epoch outside the table or a record that is not resident fails before anything is
 *     launched, naming kind, step, epoch and record.
 *   BOTTOM_TEMP with a schedule is the in-launch override of set_bottomtemp with the record chosen per column-step:
 *     the same rules (diagnostics on, mckpp_hip_bottomtemp refused), and refused while a set_bottomtemp field is resident.
 *   The other kinds are refused on a context without optional physics (none of L_RELAX_SST, L_FCORR, L_FCORR_WITHZ,
 *     L_SFCORR_WITHZ, L_RELAX_OCNT, L_RELAX_SAL, L_NO_ISOTHERM, clim_present, ...): nothing there reads them.
 *   upload and load_restart cancel all series and schedules (the column map may change).  Output windows, restart
 *     snapshots and the step log are left alone. */
enum { MCKPP_ANC_SST0 = 0, MCKPP_ANC_FCORR_TWOD, MCKPP_ANC_FCORR_WITHZ, MCKPP_ANC_SFCORR_WITHZ,
       MCKPP_ANC_OCNT_CLIM, MCKPP_ANC_SAL_CLIM, MCKPP_ANC_BOTTOM_TEMP, MCKPP_ANC_COUNT };
typedef struct { int32_t rec_prev, rec_next; double w_prev, w_next; } mckpp_anc_epoch_c;
int mckpp_hip_set_ancillary_series(mckpp_hip_handle h, int kind, int rec0, int nrec, const double *records);
int mckpp_hip_ancillary_schedule(mckpp_hip_handle h, int kind, int nt_origin, int cadence, int epoch0, int nepochs,
                                 const mckpp_anc_epoch_c *epochs);

/* The weights of mckpp_boundary_interpolate_temp / _sal (src/mckpp_boundary_interpolate.F90:25-35, :49-50; :80-90,
 * :104-105) at model time `time` (days) for records ndtupd steps of dto seconds apart (spd seconds per day), with the
 * reference's INTEGER true_time, prev_time and next_time (a REAL assigned to an INTEGER truncates toward zero) and its
 * prev_time < 0 branch, which adds `period`.  A restatement: no compiled reference pins it. */
void mckpp_host_interp_weights(double time, int32_t ndtupd, double dto, double spd, int32_t period, int32_t *prev_time,
                               int32_t *next_time, double *w_prev, double *w_next);

/* Enable/disable writing of the MCKPP_F_DIAG fields by step/init (default on; which steps of a
 * call of several steps write them: mckpp_hip_step). */
int mckpp_hip_set_diagnostics(mckpp_hip_handle h, int on);

/* Tridiagonal solver mode of the implicit step (an extension: the reference has one solver,
 * tridmat, src/mckpp_physics_solvers.F90:112-161).
 *   0 (default)  tridmat's order of operations - results bit-identical to the CPU restatement of the reference;
 *   1            the same systems eliminated from both ends at once (levels 1..nz/2 downward, nz..nz/2+1 upward,
 *                a 2x2 system in the middle): half the dependent chain, results within rounding of mode 0
 *                (profiles/r04/parity_tolerance.json; the oracle's solver_mode=1 restates
 *                it operation for operation).
 * The environment variable MCKPP_SOLVER_MODE sets the default of new handles.  <0 on an unknown mode. */
int mckpp_hip_set_solver_mode(mckpp_hip_handle h, int mode);
int mckpp_hip_get_solver_mode(mckpp_hip_handle h);

/* mckpp_initialize_ocean_model's per-column part
 * (src/mckpp_initialize_ocean.F90:48-107): initial vmix with l_initflag,
 * hmix/kmix, initial diagnostic fluxes, old/new/Us/Xs/hmixd seeds. */
int mckpp_hip_init_ocean(mckpp_hip_handle h, int ntime);

/* mckpp_physics_driver (src/mckpp_physics_driver_mod.F90:15-73): nsteps calls,
 * step i run with ntime+i.  Asynchronous on the context's stream.
 * After the call the MCKPP_F_DIAG fields are those of step ntime+nsteps-1.  Inside a
 * call of several steps (one launch; mckpp_hip_run_forced too) a step stores them only
 * where something can read them before the column's next step overwrites them: the
 * launch's last step, the restart schedule's snapshot steps, and every step while an
 * output schedule holds a diagnostic field or a bottom temperature is resident or
 * scheduled.  MCKPP_LEAN_DIAG=0 (read at every launch) makes every step store them. */
int mckpp_hip_step(mckpp_hip_handle h, int ntime, int nsteps);

/* One vmix + ocnint pass per column with Uo=U, Xo=X ("kppmix + tridiag
 * only"): mckpp_physics_verticalmixing (src/mckpp_physics_verticalmixing_mod.F90:14)
 * followed by mckpp_physics_ocnint (src/mckpp_physics_ocnint_mod.F90:19). */
int mckpp_hip_vmix_pass(mckpp_hip_handle h, int ntime);

/* mckpp_physics_verticalmixing alone (src/mckpp_physics_verticalmixing_mod.F90:14-161; the reference
 * also calls it from src/mckpp_initialize_ocean.F90:60) on every resident column with the column's own
 * l_initflag: hmix / kmix receive its hmixn / kmixn, uref / vref its scratch values (:115-125), and the
 * MCKPP_F_DIAG fields of a vmix (rho, cp, buoy, Rig, dbloc, Shsq, difm, difs, dift, ghat, wU(0), wX(0),
 * wXNT) are rewritten; profiles, saved time levels and hmixd stay as they are. */
int mckpp_hip_vmix_only(mckpp_hip_handle h, int ntime);

int mckpp_hip_synchronize(mckpp_hip_handle h);

/* device -> 3D: scatter half of mckpp_fields_1dto3d
 * (src/mckpp_types_transfer.F90:199-327) for the fields selected.  The row
 * fields are re-laid on the device into the Fortran order and cross PCIe once
 * each, the transfer of one field running under the layout kernel of the next;
 * the per-column records come as one array.  The arrays `s` points to (and
 * those of mckpp_hip_upload, _update_ancillaries, _window_fetch) are pinned on
 * first use (hipHostRegister) so the transfers run at the bus rate; they stay
 * pinned until the context is finalised - call mckpp_hip_release_host_arrays
 * before freeing them earlier.  MCKPP_HIP_NO_HOST_REGISTER=1 in the environment
 * switches the pinning off. */
int mckpp_hip_download(mckpp_hip_handle h, mckpp_state_ptrs_c *s, uint32_t field_mask);
int mckpp_hip_release_host_arrays(mckpp_hip_handle h);

/* Restart set (reference: XIOS restart context, src/mckpp_xios_io.F90:368-387
 * write list, :436-465 read path, cadence src/mckpp_xios_control.F90:61-83):
 * U,V,T,S,CP,rho,hmix,kmix,Sref,SSref,Ssurf,Tref,old,new,Us,Vs,Ts,Ss,hmixd (and
 * the column map) straight between HBM and a flat binary file.  load needs a
 * context created with the same vertical grid; it replaces any resident state
 * (only after the whole file has been read and checked: a bad file leaves the
 * resident state as it was). */
int mckpp_hip_save_restart(mckpp_hip_handle h, const char *path);
int mckpp_hip_load_restart(mckpp_hip_handle h, const char *path);

/* Restart snapshots taken inside the step launches, so that a run with restart output can still take many steps in
 * one launch.  The reference writes a restart whenever MOD(ntime, ndt_per_restart) == 0
 * (src/mckpp_xios_control.F90:61-83): restart_schedule(h, 1, ndt_per_restart, nslots).  Its other restart, "always
 * at the end of the run", is the ordinary mckpp_hip_save_restart after the last step.
 *   Snapshot s >= 0 is the state after step nt_origin + (s+1)*period - 1; it lives in ring slot s % nslots of device
 *   memory (a slot is as large as a restart file).  The column kernel copies each column's restart set there right
 *   after that column's step.
 *   restart_schedule: sets the schedule (period 0: cancels it).  The schedule in place is dropped first; if the slots
 *     cannot be allocated the call fails and no schedule is set.  upload and load_restart cancel the schedule.
 *   Every MCKPP_MODE_STEP launch - step, run_forced and their multi_ forms, one launch or a launch per step - takes
 *     the snapshots whose steps it runs (init_ocean, vmix_pass and vmix_only never do).  The steps under the schedule
 *     must follow on from one another, and a launch may not reach a snapshot whose slot holds one that is not yet
 *     released: such a launch fails before anything is launched.  A snapshot whose step ran before the schedule was
 *     set does not exist.
 *   restart_snapshots: first_kept, the first snapshot not released, and last_complete, the last one whose step has
 *     been launched (-1: none).
 *   restart_snapshot_save: writes snapshot `snap` to `path`, byte for byte the file mckpp_hip_save_restart would have
 *     written had the run stopped after the snapshot's step; mckpp_hip_load_restart reads it.  Waits for the launches
 *     of the call that completed the snapshot only, not for launches queued behind it: they keep running while the
 *     file is written.  Fails, naming the snapshot's step, for a snapshot that is incomplete, released or never existed.
 *   restart_snapshot_release: releases snapshots up to and including upto_snap (complete ones only).
 * A snapshot is the state as the step's kernel left it.  The L_VARY_BOTTOM_TEMP override from a resident field
 * (mckpp_hip_set_bottomtemp) is part of the step's kernel, so it is in the snapshot, as it is in the reference's restart
 * file; the override the host applies after a launch (mckpp_hip_bottomtemp) is not.  Scheduled output windows
 * likewise. */
int mckpp_hip_restart_schedule(mckpp_hip_handle h, int nt_origin, int period, int nslots);
int mckpp_hip_restart_snapshots(mckpp_hip_handle h, int64_t *first_kept, int64_t *last_complete);
int mckpp_hip_restart_snapshot_save(mckpp_hip_handle h, int64_t snap, const char *path);
int mckpp_hip_restart_snapshot_release(mckpp_hip_handle h, int64_t upto_snap);

/* The step log: what the status words and pass counts of the steps inside a launch were.  mckpp_hip_status reads the
 * words of the last step only - a column's word is zeroed when its next step starts - so after mckpp_hip_step(nt, n > 1)
 * or mckpp_hip_run_forced it says nothing of steps nt .. nt+n-2.  With a log set, every MCKPP_MODE_STEP launch - step,
 * run_forced and their multi_ forms, one launch or a launch per step - appends one record for each column-step that
 * ends with a non-zero status word or with at least min_passes passes (init_ocean, vmix_pass and vmix_only never
 * log).  The reference's STOP on a zero pivot (src/mckpp_physics_solvers.F90:140-148) and its located warnings
 * (src/mckpp_physics_ocnstep_mod.F90:184-191, 229-236) can so be reported for every step of a run of one launch.
 *   A column-step retried by the instability trap is one record, with the status accumulated over its tries and the
 *   passes of all of them, as mckpp_hip_status would have reported it after that step.
 *   step_log: sets the log: `capacity` records of 16 bytes in device memory; min_passes 0: flagged column-steps only.
 *     Capacity 0 cancels it; negative arguments are errors.  The log in place is dropped first; if the records cannot
 *     be allocated the call fails and no log is set.  upload and load_restart cancel the log (its records name
 *     resident columns).
 *   step_log_count: waits for the context's stream.  n_events: every event since the log was set or cleared;
 *     n_stored = min(n_events, capacity); status_or: the OR of the status words of all events, those that found no room
 *     included - a zero pivot is never lost to overflow.  Overflow never refuses or stops a launch; which `capacity`
 *     events are the stored ones is then unspecified.  (The device counts events in 32 bits.)
 *   step_log_fetch: the first n <= n_stored stored records, sorted by (nt, point): the step, the 0-based point in the
 *     caller's 3-D ordering - as mckpp_hip_status numbers its words - the status word and the passes.  Null arrays are
 *     skipped.  Does not clear the log.
 *   step_log_clear: keeps the log set; the event count and the OR are zero again (behind the launches already queued).
 * A launch without a log runs what it ran before the log existed, apart from one uniform branch. */
int mckpp_hip_step_log(mckpp_hip_handle h, int64_t capacity, int min_passes);
int mckpp_hip_step_log_count(mckpp_hip_handle h, int64_t *n_events, int64_t *n_stored, int32_t *status_or);
int mckpp_hip_step_log_fetch(mckpp_hip_handle h, int64_t n, int32_t *nt, int32_t *point, int32_t *status, int32_t *npasses);
int mckpp_hip_step_log_clear(mckpp_hip_handle h);

/* What the reference's time loop rewrites on the host between steps when the
 * optional physics is on (mckpp_boundary_update, src/mckpp_ocean_model_3D.F90:51-55;
 * the ndtupd* cadences of src/mckpp_boundary_update.F90): relax_sst, SST0,
 * fcorr_twod, relax_sal, relax_ocnT, fcorr_withz, sfcorr_withz, ocnT_clim,
 * sal_clim, nmodeadv/modeadv/advection.  Only those members of `s` are read;
 * the prognostic state stays as it is on the device.  Also what an
 * optional-physics context needs after mckpp_hip_load_restart (the restart set
 * does not carry these inputs; stepping is refused until they are resident).
 * No-op on a default-physics context. */
int mckpp_hip_update_ancillaries(mckpp_hip_handle h, const mckpp_state_ptrs_c *s);

/* Output fields and their temporal operations on the device: what mckpp_xios_output_control sends
 * every step (src/mckpp_xios_io.F90:74-210) and what XIOS then does with it ("instant", "average",
 * "minimum", "maximum", run/iodef.xml:88-157), so that only reduced fields leave the GPU.
 * MCKPP_OUT_* names follow the XIOS field ids; 3-D fields come back as out(npts,nzp1) on the vertical
 * axis the reference sends them on (levels 1..nzp1 for u, v, T, S, B, rho, cp, Rig, dbloc (0 at nzp1),
 * Shsq and the correction increments; interfaces 0..nz for wu..wTnt and for difm/dift/difs, whose
 * shifted copy at :136-148 is dif*(0:nz)), 2-D fields as out(npts).  S is X(:,:,2)+Sref as at :108-111;
 * MCKPP_OUT_S_ANOM is the bare X(:,:,2).  cplwght (a coupling weight, not on this path) is not offered.
 *   window_select: the fields accumulate reduces (default u, v, T, S_ANOM, hmix); resets the window
 *   window_reset / window_accumulate: start of an output window / once after each step
 *   window_fetch: op 0 mean, 1 min, 2 max over the window (selected fields); op 3 instant - the field as
 *     it stands on the device now, any field, no accumulate needed.  Land points keep what `out` held. */
enum {
  MCKPP_OUT_U = 0, MCKPP_OUT_V, MCKPP_OUT_T, MCKPP_OUT_S_ANOM, MCKPP_OUT_HMIX,
  MCKPP_OUT_S, MCKPP_OUT_B, MCKPP_OUT_WU, MCKPP_OUT_WV, MCKPP_OUT_WT, MCKPP_OUT_WS, MCKPP_OUT_WB, MCKPP_OUT_WTNT,
  MCKPP_OUT_DIFM, MCKPP_OUT_DIFT, MCKPP_OUT_DIFS, MCKPP_OUT_RHO, MCKPP_OUT_CP, MCKPP_OUT_SCORR, MCKPP_OUT_RIG,
  MCKPP_OUT_DBLOC, MCKPP_OUT_SHSQ, MCKPP_OUT_TINC_FCORR, MCKPP_OUT_FCORR_Z, MCKPP_OUT_SINC_FCORR,
  MCKPP_OUT_FCORR, MCKPP_OUT_TAUX_IN, MCKPP_OUT_TAUY_IN, MCKPP_OUT_SOLAR_IN, MCKPP_OUT_NSOLAR_IN, MCKPP_OUT_PMINUSE_IN,
  MCKPP_OUT_FREEZE_FLAG, MCKPP_OUT_COMP_FLAG, MCKPP_OUT_DAMPU_FLAG, MCKPP_OUT_DAMPV_FLAG,
  MCKPP_OUT_COUNT
};
int mckpp_hip_window_select(mckpp_hip_handle h, const int32_t *fields, int32_t nfields);
int mckpp_hip_window_reset(mckpp_hip_handle h);
int mckpp_hip_window_accumulate(mckpp_hip_handle h);
int mckpp_hip_window_fetch(mckpp_hip_handle h, int field, int op, double *out);

/* Output windows accumulated inside the step launches, so that a run with output can still take many steps in one
 * launch (mckpp_hip_run_forced, mckpp_hip_step with nsteps > 1).  A schedule is one XIOS <file> of iodef.xml: a
 * period in steps, MCKPP_OUT_* fields, and per field a mask of operations - MCKPP_WIN_MEAN, _MIN, _MAX, and _LAST,
 * the value after the window's last step (XIOS "instant" at the output step).  A context holds up to
 * MCKPP_WIN_SCHEDULES of them.  Window w >= 0 covers steps nt_origin + w*period .. nt_origin + (w+1)*period - 1.
 *   window_schedule: sets schedule `sched` (nfields 0: cancels it) with a ring of nrec records; window w lives in
 *     ring slot w % nrec.  Fails for an unknown field, an empty mask, a diagnostic field with the diagnostics off,
 *     a correction field without the correction rows, or device memory that cannot be allocated (the schedule is
 *     then not set).  upload and load_restart cancel every schedule.
 *   Every MCKPP_MODE_STEP launch - step, run_forced and their multi_ forms, one launch or a launch per step -
 *     accumulates every schedule in the column kernel, after each column's step (init_ocean, vmix_pass and
 *     vmix_only never do).  The steps under a schedule must follow on from one another, and a launch may not reach
 *     a window at or beyond first_kept + nrec: such a launch fails before anything is launched.
 *   window_record_fetch: record `rec`, op 0 mean, 1 min, 2 max, 3 last (the bit 1 << op of the field's mask), into
 *     out(npts[,nzp1]) as window_fetch lays it out; land points keep what `out` held.  Bit for bit what
 *     window_select, window_reset at the window's first step, window_accumulate after each of its steps and
 *     window_fetch (op 3: at its last step) give.  Fails, naming the record's steps, for a record that is not
 *     complete - one whose first steps ran before the schedule was set included - or has been released.
 *   window_record_release: releases records up to and including upto_rec (complete ones only), freeing their slots.
 *   window_records: first_kept, the first record not released, and last_complete, the last record whose steps have
 *     all run (-1: none); records first_kept .. last_complete can be fetched. */
#define MCKPP_WIN_MEAN 1u
#define MCKPP_WIN_MIN  2u
#define MCKPP_WIN_MAX  4u
#define MCKPP_WIN_LAST 8u
#define MCKPP_WIN_SCHEDULES 4
int mckpp_hip_window_schedule(mckpp_hip_handle h, int sched, int nt_origin, int period, int nrec,
                              const int32_t *fields, const uint32_t *ops, int32_t nfields);
int mckpp_hip_window_record_fetch(mckpp_hip_handle h, int sched, int64_t rec, int field, int op, double *out);
int mckpp_hip_window_record_release(mckpp_hip_handle h, int sched, int64_t upto_rec);
int mckpp_hip_window_records(mckpp_hip_handle h, int sched, int64_t *first_kept, int64_t *last_complete);

/* Packed export of a schedule's records, fetched while later launches run.  window_record_fetch re-lays a plane on
 * the context's stream, behind every launch already queued, and waits for that stream.  With an export set, every
 * step-launch call queues, behind its own column-kernel launches, one more launch per record the call completed:
 * it packs all planes of the record into an export slot in device memory, in the layout the host wants, and an
 * event marks the slot.  A fetch waits for that event alone and is one copy on a transfer stream of its own, into
 * the caller's array: launches queued later keep running (only DMA runs beside the column kernel, which fills
 * every CU).  The export ring has the schedule's nrec slots, record w in slot w % nrec, and no bookkeeping of its
 * own: window_records and window_record_release govern both rings.  It costs one more copy of every kept record in
 * device memory: npts * nlev * 8 (or 4) bytes per plane, 49 MB for a three-dimensional plane of 1e5 points x 61
 * levels as double.
 *   window_export: dtype MCKPP_EXP_F64, or MCKPP_EXP_F32 - every value narrowed to float after the mean's division,
 *     one conversion rounded to nearest even - or MCKPP_EXP_OFF, which drops the export.  Waits for the context's
 *     stream like window_schedule, allocates the slots, fills their land points with land_value once (no step ever
 *     writes them) and packs at once every record that is complete and not released.  Fails for an unset schedule,
 *     an unknown dtype, or memory that cannot be allocated (the schedule then stays set, without an export).
 *     window_schedule on the schedule, upload and load_restart cancel the export with the schedule.
 *   window_export_layout: the planes of a record - the schedule's fields in its order, within a field the kept
 *     operations in bit order (mean, min, max, last): per plane its field, op (0..3), levels and offset in bytes, a
 *     multiple of 256; record_bytes is the size of a record.  Plane (field, op) is [nlev][npts] values, points
 *     fastest: out(npts[,nzp1]) of window_record_fetch.  The arrays may be NULL (nplanes alone is the count).
 *   window_export_fetch: one plane of record `rec` into out (npts * nlev doubles or floats); bit for bit
 *     window_record_fetch into an array pre-filled with land_value (narrowed: that, converted).
 *   window_export_fetch_record: the whole record into out (out_bytes >= record_bytes); the bytes between planes are
 *     not specified.
 *   The fetches fail as window_record_fetch does, with the same messages, for a record that is incomplete or
 *     released; also for a schedule without an export, a plane it does not keep, or an out_bytes too small. */
#define MCKPP_EXP_OFF 0
#define MCKPP_EXP_F64 1
#define MCKPP_EXP_F32 2
int mckpp_hip_window_export(mckpp_hip_handle h, int sched, int dtype, double land_value);
int mckpp_hip_window_export_layout(mckpp_hip_handle h, int sched, int32_t *nplanes, int32_t *field, int32_t *op,
                                   int32_t *nlev, int64_t *offset_bytes, int64_t *record_bytes);
int mckpp_hip_window_export_fetch(mckpp_hip_handle h, int sched, int64_t rec, int field, int op, void *out);
int mckpp_hip_window_export_fetch_record(mckpp_hip_handle h, int sched, int64_t rec, void *out, int64_t out_bytes);

/* Per-column status words (npts entries in 3D ordering; land = 0), number of
 * columns with a non-zero word, and (optional) vmix+ocnint passes per column
 * of the last step. Any output pointer may be NULL. */
int mckpp_hip_status(mckpp_hip_handle h, int32_t *per_col, int64_t *n_flagged,
                     int32_t *npasses);

/* Timing of the most recent step/init/vmix_pass call on the context's stream, from HIP events recorded around its
 * kernel launches: total ms and the number of model steps (or passes) they covered.  mckpp_hip_step(nt, n > 1) with
 * constant forcing is ONE launch that takes every column through all n steps (a column's step waits for that
 * column's previous step only - no barrier across the device between steps, so a column that runs to itermax delays
 * nothing but itself; same results bit for bit; MCKPP_MULTISTEP=0 restores a launch per step):
 * mckpp_hip_last_launch_count tells how many kernel launches the call made. */
int mckpp_hip_last_kernel_ms(mckpp_hip_handle h, double *ms, int32_t *nlaunch);
int32_t mckpp_hip_last_launch_count(mckpp_hip_handle h);

/* Name of the column kernel this context launches for its grid and switches
 * ("k_column_ps", "k_column_ps<EXT>"); static storage, never NULL. */
const char *mckpp_hip_kernel_name(mckpp_hip_handle h);

/* Residency of this context's most recent column-kernel launch: workgroups per CU the launcher asked
 * for (its geometry is chosen per launch from the column depth and count), how many the runtime says fit
 * (registers, LDS), threads and dynamic LDS bytes per workgroup.  The launcher's choice assumes
 * max_blocks_per_cu >= blocks_per_cu. */
int mckpp_hip_kernel_residency(mckpp_hip_handle h, int32_t *blocks_per_cu, int32_t *max_blocks_per_cu,
                               int32_t *threads_per_block, int64_t *lds_bytes_per_block);

/* Number of device-resident (run_physics) columns. */
int64_t mckpp_hip_ncolumns(mckpp_hip_handle h);

/* Kernel-level batch entry points on caller-provided host arrays (tests). */
int mckpp_hip_eos_batch(mckpp_hip_handle h, int64_t n, const double *s,
                        const double *t, const double *p, double *alpha,
                        double *beta, double *sig0, double *cp);
int mckpp_hip_exp_batch(mckpp_hip_handle h, int64_t n, const double *x, double *y);
/* The kernels' exact-division helpers on n operand pairs: q4[0..n) = div_fast,
 * q4[n..2n) = div_fast_guarded, q4[2n..3n) = div_by_refined, q4[3n..4n) = the
 * compiler's IEEE n/d (csrc/mckpp_colmath.h); for the tests. */
int mckpp_hip_div_batch(mckpp_hip_handle h, int64_t n, const double *num, const double *den, double *q4);

/* ---------------------------------------------------------------------------
 * Several GPUs of one node behind one handle, for a host that is a single
 * process (the reference's program is one OpenMP process,
 * src/mckpp_physics_driver_mod.F90:27-65: one call covers all npts).  The
 * run_physics columns are dealt round-robin to the devices; each shard is an
 * ordinary context (mckpp_hip_multi_ctx) and every per-context entry point
 * above may be applied to it with the full-size Fortran arrays - a shard reads
 * and writes only its own columns.  The multi_* forms below do exactly that
 * for every shard; multi_step returns once all shards are launched.  There is
 * no collective inside a step.  mckpp_hip_multi_gather is the output gather:
 * shards -> root device over the GPU interconnect, relayout there, one
 * device-to-host transfer.
 * --------------------------------------------------------------------------- */
typedef struct mckpp_hip_multi *mckpp_hip_multi_handle;

/* run_physics mask of shard `dev` of `ndev` (host helper, no device work): the
 * j-th run_physics point in ipt order belongs to shard j mod ndev.  Returns the
 * number of columns of the shard, <0 on bad arguments. */
int64_t mckpp_host_shard_mask(int64_t npts, const int32_t *run_physics, int32_t ndev, int32_t dev, int32_t *mask_out);

/* devices == NULL: HIP devices 0 .. ndev-1. */
int mckpp_hip_multi_init(const mckpp_const_c *c, int32_t ndev, const int32_t *devices, mckpp_hip_multi_handle *out);
int mckpp_hip_multi_finalize(mckpp_hip_multi_handle m);
int32_t mckpp_hip_multi_ndev(mckpp_hip_multi_handle m);
mckpp_hip_handle mckpp_hip_multi_ctx(mckpp_hip_multi_handle m, int32_t shard);
int mckpp_hip_multi_upload(mckpp_hip_multi_handle m, const mckpp_state_ptrs_c *s);
int mckpp_hip_multi_set_forcing(mckpp_hip_multi_handle m, const double *sflux);
int mckpp_hip_multi_set_diagnostics(mckpp_hip_multi_handle m, int on);
int mckpp_hip_multi_set_solver_mode(mckpp_hip_multi_handle m, int mode);
int mckpp_hip_multi_update_ancillaries(mckpp_hip_multi_handle m, const mckpp_state_ptrs_c *s);
int mckpp_hip_multi_bottomtemp(mckpp_hip_multi_handle m, const double *bottom_temp);
int mckpp_hip_multi_set_bottomtemp(mckpp_hip_multi_handle m, const double *bottom_temp);
int mckpp_hip_multi_set_ancillary_series(mckpp_hip_multi_handle m, int kind, int rec0, int nrec, const double *records);
int mckpp_hip_multi_ancillary_schedule(mckpp_hip_multi_handle m, int kind, int nt_origin, int cadence, int epoch0,
                                       int nepochs, const mckpp_anc_epoch_c *epochs);
int mckpp_hip_multi_fluxes(mckpp_hip_multi_handle m, int ntime, const double *taux, const double *tauy,
                           const double *swf, const double *lwf, const double *lhf, const double *shf,
                           const double *rain, const double *snow, int l_rest, double flsn, double el);
int mckpp_hip_multi_init_ocean(mckpp_hip_multi_handle m, int ntime);
int mckpp_hip_multi_step(mckpp_hip_multi_handle m, int ntime, int nsteps);
int mckpp_hip_multi_synchronize(mckpp_hip_multi_handle m);
/* mckpp_hip_download over all shards (scatter half of src/mckpp_types_transfer.F90:199-327): every row
 * field goes through the gather (shards -> shard 0 -> host: one PCIe transfer per field whatever the number of
 * devices), the per-column records of each shard come to the host on their own. */
int mckpp_hip_multi_download(mckpp_hip_multi_handle m, mckpp_state_ptrs_c *s, uint32_t field_mask);
int mckpp_hip_multi_release_host_arrays(mckpp_hip_multi_handle m);
int mckpp_hip_multi_status(mckpp_hip_multi_handle m, int32_t *per_col, int64_t *n_flagged, int32_t *npasses);
int64_t mckpp_hip_multi_ncolumns(mckpp_hip_multi_handle m);
/* field: 0 U, 1 V, 2 T, 3 S -> out(npts,nzp1); 4 hmix -> out(npts); root: shard index that collects.  All
 * shards' peer copies are in flight at once (one stream per shard on the root device). */
int mckpp_hip_multi_gather(mckpp_hip_multi_handle m, int32_t field, int32_t root, double *out);
/* The reference's forced time loop (src/mckpp_ocean_model_3D.F90:38-58) over all shards: every shard keeps its
 * columns of the flux records (mckpp_hip_set_flux_series) and runs mckpp_hip_run_forced on its own stream;
 * returns once all shards are launched. */
int mckpp_hip_multi_set_flux_series(mckpp_hip_multi_handle m, int rec0, int nrec, const double *fields);
int mckpp_hip_multi_run_forced(mckpp_hip_multi_handle m, int nt_first, int nsteps, int ndtocn, int l_rest,
                               double flsn, double el);
/* The flux-record ring (mckpp_hip_flux_ring; src/mckpp_ocean_model_3D.F90:44-48, src/mckpp_fluxes_mod.F90:35-89) over
 * all shards: every shard keeps a ring of its own and compacts its own columns from the one caller array
 * `fields`[8][npts]; flux_ring_records is the range common to all shards. */
int mckpp_hip_multi_flux_ring(mckpp_hip_multi_handle m, int nslots);
int mckpp_hip_multi_flux_ring_put(mckpp_hip_multi_handle m, int rec, const double *fields);
int mckpp_hip_multi_flux_ring_records(mckpp_hip_multi_handle m, int *first, int *last);
/* Output windows (src/mckpp_xios_io.F90:74-210, run/iodef.xml:88-157) over all shards: each shard reduces
 * its own columns, window_fetch gathers the reduced rows like any other field. */
int mckpp_hip_multi_window_select(mckpp_hip_multi_handle m, const int32_t *fields, int32_t nfields);
int mckpp_hip_multi_window_reset(mckpp_hip_multi_handle m);
int mckpp_hip_multi_window_accumulate(mckpp_hip_multi_handle m);
int mckpp_hip_multi_window_fetch(mckpp_hip_multi_handle m, int field, int op, double *out);
/* Output windows inside the step launches (mckpp_hip_window_schedule) over all shards: every shard keeps the records
 * of its own columns; record_fetch gathers a record into 3-D order like window_fetch. */
int mckpp_hip_multi_window_schedule(mckpp_hip_multi_handle m, int sched, int nt_origin, int period, int nrec,
                                    const int32_t *fields, const uint32_t *ops, int32_t nfields);
int mckpp_hip_multi_window_record_fetch(mckpp_hip_multi_handle m, int sched, int64_t rec, int field, int op, double *out);
int mckpp_hip_multi_window_record_release(mckpp_hip_multi_handle m, int sched, int64_t upto_rec);
int mckpp_hip_multi_window_records(mckpp_hip_multi_handle m, int sched, int64_t *first_kept, int64_t *last_complete);
/* The export (mckpp_hip_window_export) over all shards: every shard packs its records compactly over its own resident
 * columns, points fastest in resident order; a fetch starts every shard's copy into pinned staging at once and the
 * host then merges them through the shards' point lists into `out`, setting land points to land_value
 * (mckpp_host_export_merge).  The layout is that of one context over all npts points.  A handle with one shard
 * copies straight into `out`. */
int mckpp_hip_multi_window_export(mckpp_hip_multi_handle m, int sched, int dtype, double land_value);
int mckpp_hip_multi_window_export_layout(mckpp_hip_multi_handle m, int sched, int32_t *nplanes, int32_t *field, int32_t *op,
                                         int32_t *nlev, int64_t *offset_bytes, int64_t *record_bytes);
int mckpp_hip_multi_window_export_fetch(mckpp_hip_multi_handle m, int sched, int64_t rec, int field, int op, void *out);
int mckpp_hip_multi_window_export_fetch_record(mckpp_hip_multi_handle m, int sched, int64_t rec, void *out, int64_t out_bytes);
/* The merge of the shards' planes (host only, no device work): out(npts, nlev), points fastest, of doubles
 * (MCKPP_EXP_F64) or floats (MCKPP_EXP_F32).  Shard d holds ncol[d] columns, column c at point points[d][c]; its plane
 * planes[d] is [nlev][ncol[d]] values of the same type.  A point of no shard gets land_value (converted to the
 * type) at every level.  Returns <0 on a bad argument (a point outside 0..npts-1 included; `out` is then untouched). */
int mckpp_host_export_merge(int64_t npts, int32_t nlev, int32_t dtype, double land_value, int32_t nshards,
                            const int64_t *ncol, const int32_t *const *points, const void *const *planes, void *out);
/* Restart set (src/mckpp_xios_io.F90:368-465) of all shards: one file per shard, <path>.<shard>of<ndev>.
 * load needs the state uploaded first (it gives the shards their column maps) and refuses files written for
 * another number of shards or another land mask, before anything resident is replaced. */
int mckpp_hip_multi_save_restart(mckpp_hip_multi_handle m, const char *path);
int mckpp_hip_multi_load_restart(mckpp_hip_multi_handle m, const char *path);
/* Restart snapshots inside the step launches (mckpp_hip_restart_schedule) over all shards: every shard keeps the
 * snapshots of its own columns; snapshot_save writes one file per shard, <path>.<shard>of<ndev>, which
 * mckpp_hip_multi_load_restart reads. */
int mckpp_hip_multi_restart_schedule(mckpp_hip_multi_handle m, int nt_origin, int period, int nslots);
int mckpp_hip_multi_restart_snapshots(mckpp_hip_multi_handle m, int64_t *first_kept, int64_t *last_complete);
int mckpp_hip_multi_restart_snapshot_save(mckpp_hip_multi_handle m, int64_t snap, const char *path);
int mckpp_hip_multi_restart_snapshot_release(mckpp_hip_multi_handle m, int64_t upto_snap);
/* The step log (mckpp_hip_step_log) over all shards: one log of `capacity` records per shard; count adds the shards'
 * counts and ORs their status words; fetch merges the shards' stored records and sorts them by (nt, point) - the points
 * are the caller's, the round-robin deal undone. */
int mckpp_hip_multi_step_log(mckpp_hip_multi_handle m, int64_t capacity, int min_passes);
int mckpp_hip_multi_step_log_count(mckpp_hip_multi_handle m, int64_t *n_events, int64_t *n_stored, int32_t *status_or);
int mckpp_hip_multi_step_log_fetch(mckpp_hip_multi_handle m, int64_t n, int32_t *nt, int32_t *point, int32_t *status,
                                   int32_t *npasses);
int mckpp_hip_multi_step_log_clear(mckpp_hip_multi_handle m);

#ifdef __cplusplus
}
#endif
#endif
