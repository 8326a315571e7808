!> iso_c_binding view of include/mckpp_hip.h and of its companions
!! mckpp_hip_device.h, mckpp_hip_zoom.h, mckpp_hip_device_records.h, mckpp_hip_put.h, mckpp_hip_reduce.h, mckpp_hip_vaxis.h, mckpp_hip_hgrid.h, mckpp_hip_remap.h and mckpp_hip_hv.h: the only place the Fortran host touches the HIP library.  Struct layouts mirror mckpp_const_c and
!! mckpp_state_ptrs_c member for member.
module mckpp_hip_binding
  use iso_c_binding
  implicit none

  ! per-column status bits (include/mckpp_hip.h, MCKPP_ST_*)
  integer(c_int32_t), parameter :: MCKPP_ST_ZERO_PIVOT = 1, MCKPP_ST_LONG_ITER = 2, MCKPP_ST_RETRIED = 4, MCKPP_ST_FAILED = 8, &
                                   MCKPP_ST_DODGY_OLDNEW = 16
  integer(c_int), parameter :: MCKPP_F_PROFILES = 1, MCKPP_F_SAVED = 2, MCKPP_F_SCALARS = 4, MCKPP_F_DIAG = 8
  integer(c_int), parameter :: MCKPP_F_RESTART = 7, MCKPP_F_ALL = 15
  ! MCKPP_OUT_* (XIOS field ids, src/mckpp_xios_io.F90:74-210) and the window operations
  integer(c_int), parameter :: MCKPP_OUT_U = 0, MCKPP_OUT_V = 1, MCKPP_OUT_T = 2, MCKPP_OUT_S_ANOM = 3, MCKPP_OUT_HMIX = 4, &
    MCKPP_OUT_S = 5, MCKPP_OUT_B = 6, MCKPP_OUT_WU = 7, MCKPP_OUT_WV = 8, MCKPP_OUT_WT = 9, MCKPP_OUT_WS = 10, &
    MCKPP_OUT_WB = 11, MCKPP_OUT_WTNT = 12, MCKPP_OUT_DIFM = 13, MCKPP_OUT_DIFT = 14, MCKPP_OUT_DIFS = 15, &
    MCKPP_OUT_RHO = 16, MCKPP_OUT_CP = 17, MCKPP_OUT_SCORR = 18, MCKPP_OUT_RIG = 19, MCKPP_OUT_DBLOC = 20, &
    MCKPP_OUT_SHSQ = 21, MCKPP_OUT_TINC_FCORR = 22, MCKPP_OUT_FCORR_Z = 23, MCKPP_OUT_SINC_FCORR = 24, &
    MCKPP_OUT_FCORR = 25, MCKPP_OUT_TAUX_IN = 26, MCKPP_OUT_TAUY_IN = 27, MCKPP_OUT_SOLAR_IN = 28, &
    MCKPP_OUT_NSOLAR_IN = 29, MCKPP_OUT_PMINUSE_IN = 30, MCKPP_OUT_FREEZE_FLAG = 31, MCKPP_OUT_COMP_FLAG = 32, &
    MCKPP_OUT_DAMPU_FLAG = 33, MCKPP_OUT_DAMPV_FLAG = 34
  integer(c_int), parameter :: MCKPP_OP_MEAN = 0, MCKPP_OP_MIN = 1, MCKPP_OP_MAX = 2, MCKPP_OP_INSTANT = 3
  ! operations of an output schedule (mckpp_hip_window_schedule): bit 2**op of a record fetch's op
  integer(c_int32_t), parameter :: MCKPP_WIN_MEAN = 1, MCKPP_WIN_MIN = 2, MCKPP_WIN_MAX = 4, MCKPP_WIN_LAST = 8
  integer(c_int), parameter :: MCKPP_OP_LAST = 3
  ! element types of an export of a schedule's records (mckpp_hip_window_export)
  integer(c_int), parameter :: MCKPP_EXP_OFF = 0, MCKPP_EXP_F64 = 1, MCKPP_EXP_F32 = 2
  ! kinds of the ancillary record series (MCKPP_ANC_*)
  integer(c_int), parameter :: MCKPP_ANC_SST0 = 0, MCKPP_ANC_FCORR_TWOD = 1, MCKPP_ANC_FCORR_WITHZ = 2, &
    MCKPP_ANC_SFCORR_WITHZ = 3, MCKPP_ANC_OCNT_CLIM = 4, MCKPP_ANC_SAL_CLIM = 5, MCKPP_ANC_BOTTOM_TEMP = 6, MCKPP_ANC_COUNT = 7

  !> one epoch of mckpp_hip_ancillary_schedule: record rec_prev as it is (rec_next < 0), or
  !! record(rec_next)*w_next + record(rec_prev)*w_prev
  type, bind(C) :: mckpp_anc_epoch_c
    integer(c_int32_t) :: rec_prev, rec_next
    real(c_double) :: w_prev, w_next
  end type mckpp_anc_epoch_c

  !> one plane of mckpp_hip_fetch_dev (include/mckpp_hip_device.h): levels lev0 .. lev0+nlev-1 (0-based) of output field
  !! `field` into the device array at `out`, as MCKPP_EXP_F64 or MCKPP_EXP_F32; fill_land /= 0: land points get land_value
  type, bind(C) :: mckpp_dev_plane_c
    integer(c_int32_t) :: field, lev0, nlev, dtype, fill_land
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_dev_plane_c

  !> one plane of mckpp_hip_records_dev (include/mckpp_hip_device_records.h): operation `op` (0 mean, 1 min, 2 max, 3 last)
  !! of output field `field` in record `rec` of schedule `sched`, levels lev0 .. lev0+nlev-1 (0-based) of those the schedule
  !! keeps, into the device array at `out`; fill_land /= 0: the positions that are no row of the record get land_value
  type, bind(C) :: mckpp_dev_record_plane_c
    integer(c_int32_t) :: sched, field, op, lev0, nlev, dtype, fill_land
    integer(c_int64_t) :: rec
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_dev_record_plane_c

  !> one plane of mckpp_hip_records_reduce_dev / _host (include/mckpp_hip_reduce.h): the plane mckpp_dev_record_plane_c
  !! names by sched, field, op, lev0, nlev and rec, reduced by axis_op over its levels and by domain_op over its points
  !! (MCKPP_RED_*; not both none), with the weights of mckpp_hip_reduce_weights where `weighted` has MCKPP_RED_W_LEVELS /
  !! MCKPP_RED_W_POINTS; out: doubles - npoints (domain_op none), nlev (axis_op none), or one
  type, bind(C) :: mckpp_reduce_plane_c
    integer(c_int32_t) :: sched, field, op, lev0, nlev, axis_op, domain_op, weighted
    integer(c_int64_t) :: rec
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_reduce_plane_c
  integer(c_int32_t), parameter :: MCKPP_RED_NONE = 0, MCKPP_RED_SUM = 1, MCKPP_RED_AVERAGE = 2, MCKPP_RED_MIN = 3, &
    MCKPP_RED_MAX = 4
  integer(c_int32_t), parameter :: MCKPP_RED_W_LEVELS = 1, MCKPP_RED_W_POINTS = 2

  !> one plane of mckpp_hip_put_dev / mckpp_hip_put_host (include/mckpp_hip_put.h): the array at `in`, (npts, nlev) of
  !! MCKPP_EXP_F64 or MCKPP_EXP_F32, is set into (op MCKPP_PUT_SET) or added to (MCKPP_PUT_ADD) levels lev0 .. lev0+nlev-1
  !! (0-based) of state field `field` (MCKPP_OUT_U, _V, _T, _S_ANOM, _S); flags: MCKPP_PUT_SKIP - elements equal to
  !! skip_value leave the state alone -, MCKPP_PUT_TIME_LEVELS - Us / Xs(:,:,0:1) take the same operation
  type, bind(C) :: mckpp_put_plane_c
    integer(c_int32_t) :: field, lev0, nlev, dtype, op, flags
    real(c_double) :: skip_value
    type(c_ptr) :: in
  end type mckpp_put_plane_c
  integer(c_int32_t), parameter :: MCKPP_PUT_SET = 0, MCKPP_PUT_ADD = 1
  integer(c_int32_t), parameter :: MCKPP_PUT_SKIP = 1, MCKPP_PUT_TIME_LEVELS = 2
  integer(c_int32_t), parameter :: MCKPP_PUT_PLANES_MAX = 64

  !> the caller's vertical axes (include/mckpp_hip_vaxis.h): MCKPP_VAXES axes per context, each 2 .. MCKPP_VAXIS_LEVELS_MAX
  !! heights, strictly decreasing like zm; the branch of an entry of mckpp_host_vaxis_map's table
  integer(c_int32_t), parameter :: MCKPP_VAXES = 8, MCKPP_VAXIS_LEVELS_MAX = 1024, MCKPP_VAXIS_PLANES_MAX = 64
  integer(c_int32_t), parameter :: MCKPP_VAXIS_ABOVE = 0, MCKPP_VAXIS_BELOW = 1, MCKPP_VAXIS_BRACKET = 2
  !> one plane of mckpp_hip_vaxis_put_dev / _put_host: the array at `in`, (npts, n of axis `axis`) of MCKPP_EXP_F64 or
  !! MCKPP_EXP_F32, interpolated onto every model level of state field `field`; op and flags are mckpp_put_plane_c's
  type, bind(C) :: mckpp_vaxis_put_plane_c
    integer(c_int32_t) :: field, axis, dtype, op, flags
    real(c_double) :: skip_value
    type(c_ptr) :: in
  end type mckpp_vaxis_put_plane_c
  !> the reference's initial profiles on their own axes (mckpp_hip_vaxis_init_profiles_dev / _host): u, v (npts, n of
  !! axis_vel), temp (npts, n of axis_temp), sal (npts, n of axis_sal), all of `dtype`; tk0: what the Kelvin rule subtracts
  type, bind(C) :: mckpp_vaxis_profiles_c
    integer(c_int32_t) :: axis_vel, axis_temp, axis_sal, dtype
    real(c_double) :: tk0
    type(c_ptr) :: u, v, temp, sal
  end type mckpp_vaxis_profiles_c
  !> one plane of mckpp_hip_vaxis_fetch_dev: `field` as it stands, interpolated onto axis `axis`, into out (npts, n)
  type, bind(C) :: mckpp_vaxis_dev_plane_c
    integer(c_int32_t) :: field, axis, dtype, fill_land
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_vaxis_dev_plane_c
  !> the caller's horizontal grids (include/mckpp_hip_hgrid.h): MCKPP_HGRIDS grids per context; the normalisation of a
  !! plane of mckpp_hip_hgrid_fetch_dev
  integer(c_int32_t), parameter :: MCKPP_HGRIDS = 4, MCKPP_HGRID_PLANES_MAX = 64
  integer(c_int32_t), parameter :: MCKPP_HGRID_NORM_NONE = 0, MCKPP_HGRID_NORM_USED = 1
  !> a weight table in CSR form, host memory: ptr (nrows + 1 of c_int64_t), idx (c_int32_t, 0-based), w (c_double)
  type, bind(C) :: mckpp_hgrid_table_c
    type(c_ptr) :: ptr, idx, w
  end type mckpp_hgrid_table_c
  !> one plane of mckpp_hip_hgrid_fetch_dev: levels lev0 .. lev0 + nlev - 1 of `field` as they stand, remapped onto
  !! caller grid `grid`, into out (n, nlev)
  type, bind(C) :: mckpp_hgrid_plane_c
    integer(c_int32_t) :: field, lev0, nlev, dtype, grid, norm, fill_land
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_hgrid_plane_c
  !> records out and state in on the caller's horizontal grids (include/mckpp_hip_remap.h).  One plane of
  !! mckpp_hip_remap_records_dev: mckpp_dev_record_plane_c's plane remapped onto caller grid `grid`, into out (n, nlev),
  !! with norm and fill_land as in mckpp_hgrid_plane_c; the used entries are those whose point is a row of the record
  integer(c_int32_t), parameter :: MCKPP_REMAP_PLANES_MAX = 64
  type, bind(C) :: mckpp_remap_record_plane_c
    integer(c_int32_t) :: sched, field, op, lev0, nlev, dtype, grid, norm, fill_land
    integer(c_int64_t) :: rec
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_remap_record_plane_c
  !> one plane of mckpp_hip_remap_put_dev: mckpp_put_plane_c's plane with the array at `in`, (n, nlev), on caller grid
  !! `grid`; every resident column takes the sum of its row of the grid's in table, an empty row leaves it alone
  type, bind(C) :: mckpp_remap_put_plane_c
    integer(c_int32_t) :: field, lev0, nlev, dtype, op, flags, grid
    real(c_double) :: skip_value
    type(c_ptr) :: in
  end type mckpp_remap_put_plane_c
  !> a caller grid and a caller axis in one call (include/mckpp_hip_hv.h).  One plane of mckpp_hip_hv_fetch_dev: `field`
  !! as it stands, interpolated onto axis `axis` at the model's points and then remapped onto caller grid `grid`, into
  !! out (n_grid, n_axis), with norm and fill_land as in mckpp_hgrid_plane_c
  integer(c_int32_t), parameter :: MCKPP_HV_PLANES_MAX = 64
  type, bind(C) :: mckpp_hv_plane_c
    integer(c_int32_t) :: field, axis, dtype, grid, norm, fill_land
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_hv_plane_c
  !> one plane of mckpp_hip_hv_put_dev: the array at `in`, (n_grid, n_axis), on caller grid `grid` and caller axis
  !! `axis`; every resident column takes the sums of its row of the grid's in table at the caller's levels and its
  !! whole profile is interpolated from them; op, flags and skip_value as in mckpp_vaxis_put_plane_c
  type, bind(C) :: mckpp_hv_put_plane_c
    integer(c_int32_t) :: field, axis, dtype, op, flags, grid
    real(c_double) :: skip_value
    type(c_ptr) :: in
  end type mckpp_hv_put_plane_c
  !> completed records on a caller axis (include/mckpp_hip_vrecords.h).  One plane of mckpp_hip_vrecords_vaxis_dev /
  !! _host: operation `op` of `field` in record `rec` of schedule `sched` - the record's value first, a mean divided by
  !! the period - interpolated onto axis `axis` at the record's points, into out (npoints, n_axis)
  integer(c_int32_t), parameter :: MCKPP_VRECORDS_PLANES_MAX = 64
  type, bind(C) :: mckpp_vaxis_record_plane_c
    integer(c_int32_t) :: sched, field, op, axis, dtype, fill_land
    integer(c_int64_t) :: rec
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_vaxis_record_plane_c
  !> one plane of mckpp_hip_vrecords_hv_dev: that plane remapped onto caller grid `grid`, into out (n_grid, n_axis), with
  !! norm and fill_land as in mckpp_hgrid_plane_c; the used entries are those whose point is a row of the record
  type, bind(C) :: mckpp_hv_record_plane_c
    integer(c_int32_t) :: sched, field, op, axis, dtype, grid, norm, fill_land
    integer(c_int64_t) :: rec
    real(c_double) :: land_value
    type(c_ptr) :: out
  end type mckpp_hv_record_plane_c

  !> the zoom of an output schedule (include/mckpp_hip_zoom.h): npoints distinct 0-based point numbers at `points`
  !! (c_null_ptr: every point) and levels lev0 .. lev0+nlev-1 (0-based; 0, 0: the whole axis) of each 3-D field's axis
  type, bind(C) :: mckpp_win_zoom_c
    type(c_ptr) :: points
    integer(c_int64_t) :: npoints
    integer(c_int32_t) :: lev0, nlev
  end type mckpp_win_zoom_c

  type, bind(C) :: mckpp_const_c
    integer(c_int32_t) :: nz, nztmax, nsflxs, njdt, itermax
    integer(c_int32_t) :: LKPP, LRI, LDD, L_SSref
    integer(c_int32_t) :: L_RELAX_SST, L_RELAX_CALCONLY, L_FCORR, L_FCORR_WITHZ
    integer(c_int32_t) :: L_SFCORR, L_SFCORR_WITHZ, L_RELAX_SAL, L_RELAX_OCNT
    integer(c_int32_t) :: L_NO_FREEZE, L_NO_ISOTHERM, L_DAMP_CURR
    integer(c_int32_t) :: clim_present
    integer(c_int32_t) :: iso_bot, dt_uvdamp
    integer(c_int32_t) :: maxmodeadv, L_ADVECT
    real(c_double) :: hmixtolfrac, dto, grav, vonk, sice, iso_thresh
    type(c_ptr) :: zm, hm, dm, tri, wmt, wst
  end type mckpp_const_c

  type, bind(C) :: mckpp_state_ptrs_c
    integer(c_int64_t) :: npts
    type(c_ptr) :: U, X, Us, Xs, U_init, hmixd
    type(c_ptr) :: f, ocdepth, Sref, SSref, Ssurf
    type(c_ptr) :: hmix, kmix, Tref, uref, vref
    type(c_ptr) :: reset_flag, dampu_flag, dampv_flag, freeze_flag
    type(c_ptr) :: sflux
    type(c_ptr) :: old, new_, jerlov
    type(c_ptr) :: l_ocean, l_initflag, run_physics
    type(c_ptr) :: rho, cp, buoy, difm, difs, dift, wU, wX, wXNT, ghat, Rig, Shsq, dbloc, swfrac, swdk_opt
    type(c_ptr) :: relax_sst, SST0, fcorr_twod, relax_sal, relax_ocnT, fcorr
    type(c_ptr) :: fcorr_withz, sfcorr_withz, ocnT_clim, sal_clim
    type(c_ptr) :: tinc_fcorr, sinc_fcorr, ocnTcorr, scorr
    type(c_ptr) :: nmodeadv, modeadv, advection
  end type mckpp_state_ptrs_c

  interface
    function mckpp_hip_last_error() bind(C, name="mckpp_hip_last_error") result(p)
      import :: c_ptr
      type(c_ptr) :: p
    end function
    function mckpp_hip_device_count() bind(C, name="mckpp_hip_device_count") result(n)
      import :: c_int
      integer(c_int) :: n
    end function
    function mckpp_hip_init(c, device, handle) bind(C, name="mckpp_hip_init") result(rc)
      import :: c_int, c_ptr, mckpp_const_c
      type(mckpp_const_c), intent(in) :: c
      integer(c_int), value :: device
      type(c_ptr), intent(out) :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_finalize(handle) bind(C, name="mckpp_hip_finalize") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    subroutine mckpp_host_lookup(vonk, wmt, wst) bind(C, name="mckpp_host_lookup")
      import :: c_double
      real(c_double), value :: vonk
      real(c_double), intent(out) :: wmt(*), wst(*)
    end subroutine
    subroutine mckpp_host_tri(nz, nztmax, dto, zm, hm, tri) bind(C, name="mckpp_host_tri")
      import :: c_double, c_int32_t
      integer(c_int32_t), value :: nz, nztmax
      real(c_double), value :: dto
      real(c_double), intent(in) :: zm(*), hm(*)
      real(c_double), intent(out) :: tri(*)
    end subroutine
    function mckpp_hip_upload(handle, s) bind(C, name="mckpp_hip_upload") result(rc)
      import :: c_int, c_ptr, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(in) :: s
      integer(c_int) :: rc
    end function
    function mckpp_hip_update_ancillaries(handle, s) bind(C, name="mckpp_hip_update_ancillaries") result(rc)
      import :: c_int, c_ptr, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(in) :: s
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_forcing(handle, sflux) bind(C, name="mckpp_hip_set_forcing") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in) :: sflux(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_fluxes(handle, ntime, taux, tauy, swf, lwf, lhf, shf, rain, snow, l_rest, flsn, el) &
        bind(C, name="mckpp_hip_fluxes") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime, l_rest
      real(c_double), intent(in) :: taux(*), tauy(*), swf(*), lwf(*), lhf(*), shf(*), rain(*), snow(*)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_flux_series(handle, rec0, nrec, fields) bind(C, name="mckpp_hip_set_flux_series") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: rec0, nrec
      real(c_double), intent(in) :: fields(*)
      integer(c_int) :: rc
    end function
    ! the flux-record ring (src/mckpp_ocean_model_3D.F90:44-48, src/mckpp_fluxes_mod.F90:35-89): fields(npts, 8) per record
    function mckpp_hip_flux_ring(handle, nslots) bind(C, name="mckpp_hip_flux_ring") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: nslots
      integer(c_int) :: rc
    end function
    function mckpp_hip_flux_ring_put(handle, rec, fields) bind(C, name="mckpp_hip_flux_ring_put") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: rec
      real(c_double), intent(in) :: fields(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_flux_ring_records(handle, first, last) bind(C, name="mckpp_hip_flux_ring_records") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), intent(out) :: first, last
      integer(c_int) :: rc
    end function
    function mckpp_hip_run_forced(handle, nt_first, nsteps, ndtocn, l_rest, flsn, el) &
        bind(C, name="mckpp_hip_run_forced") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: nt_first, nsteps, ndtocn, l_rest
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_bottomtemp(handle, bottom_temp) bind(C, name="mckpp_hip_bottomtemp") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in) :: bottom_temp(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_bottomtemp(handle, bottom_temp) bind(C, name="mckpp_hip_set_bottomtemp") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in), optional :: bottom_temp(*)   ! absent: NULL, cancels the resident field
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_ancillary_series(handle, kind, rec0, nrec, records) bind(C, name="mckpp_hip_set_ancillary_series") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: kind, rec0, nrec
      real(c_double), intent(in), optional :: records(*)   ! absent: NULL (nrec = 0 frees the kind's records)
      integer(c_int) :: rc
    end function
    function mckpp_hip_ancillary_schedule(handle, kind, nt_origin, cadence, epoch0, nepochs, epochs) &
        bind(C, name="mckpp_hip_ancillary_schedule") result(rc)
      import :: c_int, c_ptr, mckpp_anc_epoch_c
      type(c_ptr), value :: handle
      integer(c_int), value :: kind, nt_origin, cadence, epoch0, nepochs
      type(mckpp_anc_epoch_c), intent(in), optional :: epochs(*)   ! absent: NULL (nepochs = 0 cancels the schedule)
      integer(c_int) :: rc
    end function
    subroutine mckpp_host_interp_weights(time, ndtupd, dto, spd, period, prev_time, next_time, w_prev, w_next) &
        bind(C, name="mckpp_host_interp_weights")
      import :: c_double, c_int32_t
      real(c_double), value :: time, dto, spd
      integer(c_int32_t), value :: ndtupd, period
      integer(c_int32_t), intent(out) :: prev_time, next_time
      real(c_double), intent(out) :: w_prev, w_next
    end subroutine
    function mckpp_hip_save_restart(handle, path) bind(C, name="mckpp_hip_save_restart") result(rc)
      import :: c_int, c_ptr, c_char
      type(c_ptr), value :: handle
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_load_restart(handle, path) bind(C, name="mckpp_hip_load_restart") result(rc)
      import :: c_int, c_ptr, c_char
      type(c_ptr), value :: handle
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_diagnostics(handle, on) bind(C, name="mckpp_hip_set_diagnostics") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: on
      integer(c_int) :: rc
    end function
    function mckpp_hip_set_solver_mode(handle, mode) bind(C, name="mckpp_hip_set_solver_mode") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: mode
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_set_solver_mode(handle, mode) bind(C, name="mckpp_hip_multi_set_solver_mode") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: mode
      integer(c_int) :: rc
    end function
    function mckpp_hip_init_ocean(handle, ntime) bind(C, name="mckpp_hip_init_ocean") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime
      integer(c_int) :: rc
    end function
    function mckpp_hip_step(handle, ntime, nsteps) bind(C, name="mckpp_hip_step") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime, nsteps
      integer(c_int) :: rc
    end function
    ! ---- several GPUs behind one handle (include/mckpp_hip.h, mckpp_hip_multi_*) ----
    function mckpp_hip_multi_init(c, ndev, devices, handle) bind(C, name="mckpp_hip_multi_init") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_const_c
      type(mckpp_const_c), intent(in) :: c
      integer(c_int32_t), value :: ndev
      integer(c_int32_t), intent(in) :: devices(*)
      type(c_ptr), intent(out) :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_finalize(handle) bind(C, name="mckpp_hip_multi_finalize") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_ctx(handle, shard) bind(C, name="mckpp_hip_multi_ctx") result(h)
      import :: c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: shard
      type(c_ptr) :: h
    end function
    function mckpp_hip_multi_upload(handle, s) bind(C, name="mckpp_hip_multi_upload") result(rc)
      import :: c_int, c_ptr, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(in) :: s
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_update_ancillaries(handle, s) bind(C, name="mckpp_hip_multi_update_ancillaries") result(rc)
      import :: c_int, c_ptr, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(in) :: s
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_set_forcing(handle, sflux) bind(C, name="mckpp_hip_multi_set_forcing") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in) :: sflux(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_fluxes(handle, ntime, taux, tauy, swf, lwf, lhf, shf, rain, snow, l_rest, flsn, el) &
        bind(C, name="mckpp_hip_multi_fluxes") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime, l_rest
      real(c_double), intent(in) :: taux(*), tauy(*), swf(*), lwf(*), lhf(*), shf(*), rain(*), snow(*)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_bottomtemp(handle, bottom_temp) bind(C, name="mckpp_hip_multi_bottomtemp") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in) :: bottom_temp(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_set_bottomtemp(handle, bottom_temp) bind(C, name="mckpp_hip_multi_set_bottomtemp") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(in), optional :: bottom_temp(*)   ! absent: NULL, cancels the resident field
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_set_ancillary_series(handle, kind, rec0, nrec, records) bind(C, name="mckpp_hip_multi_set_ancillary_series") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: kind, rec0, nrec
      real(c_double), intent(in), optional :: records(*)   ! absent: NULL (nrec = 0 frees the kind's records)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_ancillary_schedule(handle, kind, nt_origin, cadence, epoch0, nepochs, epochs) &
        bind(C, name="mckpp_hip_multi_ancillary_schedule") result(rc)
      import :: c_int, c_ptr, mckpp_anc_epoch_c
      type(c_ptr), value :: handle
      integer(c_int), value :: kind, nt_origin, cadence, epoch0, nepochs
      type(mckpp_anc_epoch_c), intent(in), optional :: epochs(*)   ! absent: NULL (nepochs = 0 cancels the schedule)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_init_ocean(handle, ntime) bind(C, name="mckpp_hip_multi_init_ocean") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_step(handle, ntime, nsteps) bind(C, name="mckpp_hip_multi_step") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime, nsteps
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_synchronize(handle) bind(C, name="mckpp_hip_multi_synchronize") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_download(handle, s, mask) bind(C, name="mckpp_hip_multi_download") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(in) :: s
      integer(c_int32_t), value :: mask
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_gather(handle, field, root, out) bind(C, name="mckpp_hip_multi_gather") result(rc)
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: field, root
      real(c_double), intent(inout) :: out(*)
      integer(c_int) :: rc
    end function
    ! ---- the forced time loop, the output windows and the restart set for all shards ----
    function mckpp_hip_multi_set_flux_series(handle, rec0, nrec, fields) bind(C, name="mckpp_hip_multi_set_flux_series") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: rec0, nrec
      real(c_double), intent(in) :: fields(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_flux_ring(handle, nslots) bind(C, name="mckpp_hip_multi_flux_ring") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: nslots
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_flux_ring_put(handle, rec, fields) bind(C, name="mckpp_hip_multi_flux_ring_put") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: rec
      real(c_double), intent(in) :: fields(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_flux_ring_records(handle, first, last) bind(C, name="mckpp_hip_multi_flux_ring_records") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), intent(out) :: first, last
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_run_forced(handle, nt_first, nsteps, ndtocn, l_rest, flsn, el) &
        bind(C, name="mckpp_hip_multi_run_forced") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: nt_first, nsteps, ndtocn, l_rest
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_select(handle, fields, nfields) bind(C, name="mckpp_hip_multi_window_select") result(rc)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), intent(in) :: fields(*)
      integer(c_int32_t), value :: nfields
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_reset(handle) bind(C, name="mckpp_hip_multi_window_reset") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_accumulate(handle) bind(C, name="mckpp_hip_multi_window_accumulate") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_fetch(handle, field, op, out) bind(C, name="mckpp_hip_multi_window_fetch") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: field, op
      real(c_double), intent(inout) :: out(*)
      integer(c_int) :: rc
    end function
    ! output windows accumulated inside the step launches (mckpp_hip_window_schedule of include/mckpp_hip.h)
    function mckpp_hip_multi_window_schedule(handle, sched, nt_origin, period, nrec, fields, ops, nfields) &
        bind(C, name="mckpp_hip_multi_window_schedule") result(rc)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched, nt_origin, period, nrec
      integer(c_int32_t), intent(in) :: fields(*), ops(*)
      integer(c_int32_t), value :: nfields
      integer(c_int) :: rc
    end function
    ! ... over chosen points and levels (include/mckpp_hip_zoom.h); zoom c_null_ptr: the unzoomed schedule
    function mckpp_hip_multi_window_schedule_zoom(handle, sched, nt_origin, period, nrec, fields, ops, nfields, zoom) &
        bind(C, name="mckpp_hip_multi_window_schedule_zoom") result(rc)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched, nt_origin, period, nrec
      integer(c_int32_t), intent(in) :: fields(*), ops(*)
      integer(c_int32_t), value :: nfields
      type(c_ptr), value :: zoom   ! c_loc of a mckpp_win_zoom_c
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_zoom(handle, sched, npoints, lev0, nlev, ring_bytes) &
        bind(C, name="mckpp_hip_multi_window_zoom") result(rc)
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      integer(c_int64_t), intent(out) :: npoints, ring_bytes
      integer(c_int32_t), intent(out) :: lev0, nlev
      integer(c_int) :: rc
    end function
    function mckpp_host_zoom_box(nx, ny, ibegin, ni, jbegin, nj, points) bind(C, name="mckpp_host_zoom_box") result(rc)
      import :: c_int, c_int32_t, c_int64_t
      integer(c_int64_t), value :: nx, ny, ibegin, ni, jbegin, nj
      integer(c_int32_t), intent(out) :: points(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_record_fetch(handle, sched, rec, field, op, out) &
        bind(C, name="mckpp_hip_multi_window_record_fetch") result(rc)
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      integer(c_int64_t), value :: rec
      integer(c_int), value :: field, op
      real(c_double), intent(inout) :: out(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_record_release(handle, sched, upto_rec) &
        bind(C, name="mckpp_hip_multi_window_record_release") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      integer(c_int64_t), value :: upto_rec
      integer(c_int) :: rc
    end function
    ! the packed export of a schedule's records, fetched while later launches run (mckpp_hip_window_export of
    ! include/mckpp_hip.h); `out` is the address of the caller's array of doubles or floats
    function mckpp_hip_multi_window_export(handle, sched, dtype, land_value) &
        bind(C, name="mckpp_hip_multi_window_export") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: sched, dtype
      real(c_double), value :: land_value
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_export_layout(handle, sched, nplanes, field, op, nlev, offset_bytes, record_bytes) &
        bind(C, name="mckpp_hip_multi_window_export_layout") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      type(c_ptr), value :: nplanes, field, op, nlev, offset_bytes, record_bytes   ! each may be c_null_ptr
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_export_fetch(handle, sched, rec, field, op, out) &
        bind(C, name="mckpp_hip_multi_window_export_fetch") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      integer(c_int64_t), value :: rec
      integer(c_int), value :: field, op
      type(c_ptr), value :: out
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_window_export_fetch_record(handle, sched, rec, out, out_bytes) &
        bind(C, name="mckpp_hip_multi_window_export_fetch_record") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: sched
      integer(c_int64_t), value :: rec
      type(c_ptr), value :: out
      integer(c_int64_t), value :: out_bytes
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_save_restart(handle, path) bind(C, name="mckpp_hip_multi_save_restart") result(rc)
      import :: c_int, c_ptr, c_char
      type(c_ptr), value :: handle
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_load_restart(handle, path) bind(C, name="mckpp_hip_multi_load_restart") result(rc)
      import :: c_int, c_ptr, c_char
      type(c_ptr), value :: handle
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    ! restart snapshots taken inside the step launches (mckpp_hip_restart_schedule of include/mckpp_hip.h)
    function mckpp_hip_multi_restart_schedule(handle, nt_origin, period, nslots) &
        bind(C, name="mckpp_hip_multi_restart_schedule") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: nt_origin, period, nslots
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_restart_snapshots(handle, first_kept, last_complete) &
        bind(C, name="mckpp_hip_multi_restart_snapshots") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: first_kept, last_complete
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_restart_snapshot_save(handle, snap, path) &
        bind(C, name="mckpp_hip_multi_restart_snapshot_save") result(rc)
      import :: c_int, c_int64_t, c_ptr, c_char
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: snap
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_restart_snapshot_release(handle, upto_snap) &
        bind(C, name="mckpp_hip_multi_restart_snapshot_release") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: upto_snap
      integer(c_int) :: rc
    end function
    function mckpp_hip_restart_schedule(handle, nt_origin, period, nslots) bind(C, name="mckpp_hip_restart_schedule") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: nt_origin, period, nslots
      integer(c_int) :: rc
    end function
    function mckpp_hip_restart_snapshots(handle, first_kept, last_complete) bind(C, name="mckpp_hip_restart_snapshots") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: first_kept, last_complete
      integer(c_int) :: rc
    end function
    function mckpp_hip_restart_snapshot_save(handle, snap, path) bind(C, name="mckpp_hip_restart_snapshot_save") result(rc)
      import :: c_int, c_int64_t, c_ptr, c_char
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: snap
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_restart_snapshot_release(handle, upto_snap) bind(C, name="mckpp_hip_restart_snapshot_release") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: upto_snap
      integer(c_int) :: rc
    end function
    ! the step log of the step launches (mckpp_hip_step_log of include/mckpp_hip.h)
    function mckpp_hip_multi_step_log(handle, capacity, min_passes) bind(C, name="mckpp_hip_multi_step_log") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: capacity
      integer(c_int), value :: min_passes
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_step_log_count(handle, n_events, n_stored, status_or) &
        bind(C, name="mckpp_hip_multi_step_log_count") result(rc)
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: n_events, n_stored
      integer(c_int32_t), intent(out) :: status_or
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_step_log_fetch(handle, n, nt, point, status, npasses) &
        bind(C, name="mckpp_hip_multi_step_log_fetch") result(rc)
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: n
      integer(c_int32_t), intent(out) :: nt(*), point(*), status(*), npasses(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_step_log_clear(handle) bind(C, name="mckpp_hip_multi_step_log_clear") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_step_log(handle, capacity, min_passes) bind(C, name="mckpp_hip_step_log") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: capacity
      integer(c_int), value :: min_passes
      integer(c_int) :: rc
    end function
    function mckpp_hip_step_log_count(handle, n_events, n_stored, status_or) bind(C, name="mckpp_hip_step_log_count") result(rc)
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: n_events, n_stored
      integer(c_int32_t), intent(out) :: status_or
      integer(c_int) :: rc
    end function
    function mckpp_hip_step_log_fetch(handle, n, nt, point, status, npasses) bind(C, name="mckpp_hip_step_log_fetch") result(rc)
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), value :: n
      integer(c_int32_t), intent(out) :: nt(*), point(*), status(*), npasses(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_step_log_clear(handle) bind(C, name="mckpp_hip_step_log_clear") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_release_host_arrays(handle) bind(C, name="mckpp_hip_multi_release_host_arrays") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    ! ---- output fields with XIOS' temporal operations on the device (MCKPP_OUT_* of include/mckpp_hip.h) ----
    function mckpp_hip_window_select(handle, fields, nfields) bind(C, name="mckpp_hip_window_select") result(rc)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), intent(in) :: fields(*)
      integer(c_int32_t), value :: nfields
      integer(c_int) :: rc
    end function
    function mckpp_hip_window_reset(handle) bind(C, name="mckpp_hip_window_reset") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_window_accumulate(handle) bind(C, name="mckpp_hip_window_accumulate") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_window_fetch(handle, field, op, out) bind(C, name="mckpp_hip_window_fetch") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      integer(c_int), value :: field, op
      real(c_double), intent(inout) :: out(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vmix_only(handle, ntime) bind(C, name="mckpp_hip_vmix_only") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: ntime
      integer(c_int) :: rc
    end function
    function mckpp_hip_synchronize(handle) bind(C, name="mckpp_hip_synchronize") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: rc
    end function
    function mckpp_hip_download(handle, s, mask) bind(C, name="mckpp_hip_download") result(rc)
      import :: c_int, c_ptr, c_int32_t, mckpp_state_ptrs_c
      type(c_ptr), value :: handle
      type(mckpp_state_ptrs_c), intent(inout) :: s
      integer(c_int32_t), value :: mask
      integer(c_int) :: rc
    end function
    function mckpp_hip_status(handle, per_col, n_flagged, npasses) bind(C, name="mckpp_hip_status") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, per_col, n_flagged, npasses
      integer(c_int) :: rc
    end function
    !> status words and pass counts of the last step for all npts points of all devices (land: 0)
    function mckpp_hip_multi_status(m, per_col, n_flagged, npasses) bind(C, name="mckpp_hip_multi_status") result(rc)
      import :: c_int, c_ptr, c_int32_t, c_int64_t
      type(c_ptr), value :: m
      integer(c_int32_t), intent(out) :: per_col(*), npasses(*)
      integer(c_int64_t), intent(out) :: n_flagged
      integer(c_int) :: rc
    end function
    function mckpp_hip_last_kernel_ms(handle, ms, nlaunch) bind(C, name="mckpp_hip_last_kernel_ms") result(rc)
      import :: c_int, c_ptr, c_double, c_int32_t
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: ms
      integer(c_int32_t), intent(out) :: nlaunch
      integer(c_int) :: rc
    end function
    ! The device-array interface (include/mckpp_hip_device.h).  fields(8): the device addresses of taux, tauy, swf, lwf,
    ! lhf, shf, rain, snow (npts doubles each) - c_loc of the arrays inside an OpenMP `target data use_device_ptr` or an
    ! OpenACC `host_data use_device` region; streams: the caller's hipStream_t, c_null_ptr for the null stream.
    function mckpp_hip_fluxes_dev(handle, ntime, fields, l_rest, flsn, el, producer_stream) &
        bind(C, name="mckpp_hip_fluxes_dev") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle, producer_stream
      integer(c_int), value :: ntime, l_rest
      type(c_ptr), intent(in) :: fields(8)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_flux_ring_put_dev(handle, rec, fields, producer_stream) &
        bind(C, name="mckpp_hip_flux_ring_put_dev") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, producer_stream
      integer(c_int), value :: rec
      type(c_ptr), intent(in) :: fields(8)
      integer(c_int) :: rc
    end function
    function mckpp_hip_fetch_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_dev_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_dev_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_dev_fence(handle, stream) bind(C, name="mckpp_hip_dev_fence") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, stream
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_fluxes_dev(m, ntime, fields, l_rest, flsn, el, producer_stream) &
        bind(C, name="mckpp_hip_multi_fluxes_dev") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: m, producer_stream
      integer(c_int), value :: ntime, l_rest
      type(c_ptr), intent(in) :: fields(8)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_flux_ring_put_dev(m, rec, fields, producer_stream) &
        bind(C, name="mckpp_hip_multi_flux_ring_put_dev") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: m, producer_stream
      integer(c_int), value :: rec
      type(c_ptr), intent(in) :: fields(8)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_fetch_dev(m, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_multi_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_dev_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_dev_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_dev_fence(m, stream) bind(C, name="mckpp_hip_multi_dev_fence") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: m, stream
      integer(c_int) :: rc
    end function
    ! records of output schedules into device arrays (include/mckpp_hip_device_records.h): one launch for all planes on
    ! the context's stream, so mckpp_hip_window_record_release may follow at once
    function mckpp_hip_records_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_records_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_dev_record_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_dev_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_records_dev(m, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_multi_records_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_dev_record_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_dev_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! records reduced over levels and points (include/mckpp_hip_reduce.h, which states the arithmetic and its order);
    ! the weight arrays are host arrays, c_null_ptr: not set
    function mckpp_hip_reduce_weights(handle, point_w, level_w, iface_w) bind(C, name="mckpp_hip_reduce_weights") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, point_w, level_w, iface_w
      integer(c_int) :: rc
    end function
    function mckpp_hip_records_reduce_dev(handle, nplanes, planes, consumer_stream) &
        bind(C, name="mckpp_hip_records_reduce_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_reduce_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_reduce_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_records_reduce_host(handle, nplanes, planes) bind(C, name="mckpp_hip_records_reduce_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_reduce_plane_c
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nplanes
      type(mckpp_reduce_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_host_reduce_tree(t, n) bind(C, name="mckpp_host_reduce_tree") result(s)
      import :: c_double, c_int64_t
      real(c_double), intent(in) :: t(*)
      integer(c_int64_t), value :: n
      real(c_double) :: s
    end function
    function mckpp_hip_multi_reduce_weights(m, point_w, level_w, iface_w) bind(C, name="mckpp_hip_multi_reduce_weights") &
        result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: m, point_w, level_w, iface_w
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_records_reduce_dev(m, nplanes, planes, consumer_stream) &
        bind(C, name="mckpp_hip_multi_records_reduce_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_reduce_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_reduce_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_records_reduce_host(m, nplanes, planes) bind(C, name="mckpp_hip_multi_records_reduce_host") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_reduce_plane_c
      type(c_ptr), value :: m
      integer(c_int32_t), value :: nplanes
      type(mckpp_reduce_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! the prognostic state set or incremented in place (include/mckpp_hip_put.h): one launch for all planes on the
    ! context's stream, between launches; nothing the context has scheduled is cancelled.  A put through these raw
    ! interfaces leaves the host's kpp_3d_fields copy of U, X, Us, Xs stale, and the session layer does not see it
    function mckpp_hip_put_dev(handle, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_put_plane_c
      type(c_ptr), value :: handle, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_put_host(handle, nplanes, planes) bind(C, name="mckpp_hip_put_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_put_plane_c
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nplanes
      type(mckpp_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_put_dev(m, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_multi_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_put_plane_c
      type(c_ptr), value :: m, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_put_host(m, nplanes, planes) bind(C, name="mckpp_hip_multi_put_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_put_plane_c
      type(c_ptr), value :: m
      integer(c_int32_t), value :: nplanes
      type(mckpp_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! the caller's vertical axes (include/mckpp_hip_vaxis.h): axes defined per context, state in and the reference's
    ! initial profiles on the caller's levels, fields out on them.  As with the puts, the host's kpp_3d_fields copy of
    ! what these write is stale afterwards, and the session layer does not see it
    function mckpp_host_vaxis_map(ns, zs, nt, zt, branch, kin, t, dz) bind(C, name="mckpp_host_vaxis_map") result(rc)
      import :: c_int, c_int32_t, c_double
      integer(c_int32_t), value :: ns, nt
      real(c_double), intent(in) :: zs(*), zt(*)
      integer(c_int32_t), intent(out) :: branch(*), kin(*)
      real(c_double), intent(out) :: t(*), dz(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_define(handle, axis, n, z) bind(C, name="mckpp_hip_vaxis_define") result(rc)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: axis
      integer(c_int32_t), value :: n
      real(c_double), intent(in) :: z(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_put_dev(handle, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_vaxis_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_put_plane_c
      type(c_ptr), value :: handle, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_put_host(handle, nplanes, planes) bind(C, name="mckpp_hip_vaxis_put_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_put_plane_c
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_init_profiles_dev(handle, p, producer_stream) bind(C, name="mckpp_hip_vaxis_init_profiles_dev") result(rc)
      import :: c_int, c_ptr, mckpp_vaxis_profiles_c
      type(c_ptr), value :: handle, producer_stream
      type(mckpp_vaxis_profiles_c), intent(in) :: p
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_init_profiles_host(handle, p) bind(C, name="mckpp_hip_vaxis_init_profiles_host") result(rc)
      import :: c_int, c_ptr, mckpp_vaxis_profiles_c
      type(c_ptr), value :: handle
      type(mckpp_vaxis_profiles_c), intent(in) :: p
      integer(c_int) :: rc
    end function
    function mckpp_hip_vaxis_fetch_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_vaxis_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_dev_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_dev_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_define(m, axis, n, z) bind(C, name="mckpp_hip_multi_vaxis_define") result(rc)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: m
      integer(c_int), value :: axis
      integer(c_int32_t), value :: n
      real(c_double), intent(in) :: z(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_put_dev(m, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_multi_vaxis_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_put_plane_c
      type(c_ptr), value :: m, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_put_host(m, nplanes, planes) bind(C, name="mckpp_hip_multi_vaxis_put_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_put_plane_c
      type(c_ptr), value :: m
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_init_profiles_dev(m, p, producer_stream) bind(C, name="mckpp_hip_multi_vaxis_init_profiles_dev") result(rc)
      import :: c_int, c_ptr, mckpp_vaxis_profiles_c
      type(c_ptr), value :: m, producer_stream
      type(mckpp_vaxis_profiles_c), intent(in) :: p
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_init_profiles_host(m, p) bind(C, name="mckpp_hip_multi_vaxis_init_profiles_host") result(rc)
      import :: c_int, c_ptr, mckpp_vaxis_profiles_c
      type(c_ptr), value :: m
      type(mckpp_vaxis_profiles_c), intent(in) :: p
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vaxis_fetch_dev(m, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_multi_vaxis_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_dev_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_dev_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! the caller's horizontal grids (include/mckpp_hip_hgrid.h): grids and their weight tables per context, forcing in
    ! and fields out on a caller's grid; the three host functions need no GPU
    function mckpp_host_hgrid_check(name, nrows, nsrc, t, msg, msglen) bind(C, name="mckpp_host_hgrid_check") result(rc)
      import :: c_int, c_int64_t, c_char, mckpp_hgrid_table_c
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int64_t), value :: nrows, nsrc, msglen
      type(mckpp_hgrid_table_c), intent(in) :: t
      character(kind=c_char), intent(out) :: msg(*)
      integer(c_int) :: rc
    end function
    function mckpp_host_hgrid_apply(nrows, t, x, used, norm, fill, land_value, out) bind(C, name="mckpp_host_hgrid_apply") result(rc)
      import :: c_int, c_int64_t, c_double, c_ptr, mckpp_hgrid_table_c
      integer(c_int64_t), value :: nrows
      type(mckpp_hgrid_table_c), intent(in) :: t
      real(c_double), intent(in) :: x(*)
      type(c_ptr), value :: used   ! unsigned char per source index, or c_null_ptr: every entry is used
      integer(c_int), value :: norm, fill
      real(c_double), value :: land_value
      real(c_double), intent(inout) :: out(*)
      integer(c_int) :: rc
    end function
    function mckpp_host_hgrid_slices(nlist, rows, t, keep, slice_off, len, idx_out, w_out) &
        bind(C, name="mckpp_host_hgrid_slices") result(padded)
      import :: c_int32_t, c_int64_t, c_ptr, mckpp_hgrid_table_c
      integer(c_int64_t), value :: nlist
      type(c_ptr), value :: rows, keep, idx_out, w_out   ! c_null_ptr: all rows / nothing dropped / the sizing pass
      type(mckpp_hgrid_table_c), intent(in) :: t
      integer(c_int64_t), intent(out) :: slice_off(*)
      integer(c_int32_t), intent(out) :: len(*)
      integer(c_int64_t) :: padded
    end function
    function mckpp_hip_hgrid_define(handle, grid, n, tin, tout) bind(C, name="mckpp_hip_hgrid_define") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: grid
      integer(c_int64_t), value :: n
      type(c_ptr), value :: tin, tout   ! c_loc of a mckpp_hgrid_table_c, or c_null_ptr: that direction is missing
      integer(c_int) :: rc
    end function
    function mckpp_hip_hgrid_info(handle, grid, info) bind(C, name="mckpp_hip_hgrid_info") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int), value :: grid
      integer(c_int64_t), intent(out) :: info(6)
      integer(c_int) :: rc
    end function
    function mckpp_hip_hgrid_fluxes_dev(handle, grid, ntime, fields, l_rest, flsn, el, producer_stream) &
        bind(C, name="mckpp_hip_hgrid_fluxes_dev") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle, producer_stream
      integer(c_int), value :: grid, ntime, l_rest
      type(c_ptr), intent(in) :: fields(8)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_hgrid_flux_ring_put_dev(handle, grid, rec, fields, producer_stream) &
        bind(C, name="mckpp_hip_hgrid_flux_ring_put_dev") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, producer_stream
      integer(c_int), value :: grid, rec
      type(c_ptr), intent(in) :: fields(8)
      integer(c_int) :: rc
    end function
    function mckpp_hip_hgrid_fetch_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_hgrid_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hgrid_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hgrid_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hgrid_define(m, grid, n, tin, tout) bind(C, name="mckpp_hip_multi_hgrid_define") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: m
      integer(c_int), value :: grid
      integer(c_int64_t), value :: n
      type(c_ptr), value :: tin, tout   ! c_loc of a mckpp_hgrid_table_c, or c_null_ptr: that direction is missing
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hgrid_info(m, grid, info) bind(C, name="mckpp_hip_multi_hgrid_info") result(rc)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: m
      integer(c_int), value :: grid
      integer(c_int64_t), intent(out) :: info(6)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hgrid_fluxes_dev(m, grid, ntime, fields, l_rest, flsn, el, producer_stream) &
        bind(C, name="mckpp_hip_multi_hgrid_fluxes_dev") result(rc)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: m, producer_stream
      integer(c_int), value :: grid, ntime, l_rest
      type(c_ptr), intent(in) :: fields(8)
      real(c_double), value :: flsn, el
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hgrid_flux_ring_put_dev(m, grid, rec, fields, producer_stream) &
        bind(C, name="mckpp_hip_multi_hgrid_flux_ring_put_dev") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: m, producer_stream
      integer(c_int), value :: grid, rec
      type(c_ptr), intent(in) :: fields(8)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hgrid_fetch_dev(m, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_multi_hgrid_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hgrid_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hgrid_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! records out and state in on the caller's horizontal grids (include/mckpp_hip_remap.h): mckpp_hip_records_dev and
    ! mckpp_hip_put_dev through the weight tables of mckpp_hip_hgrid_define, with those calls' ordering
    function mckpp_hip_remap_records_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_remap_records_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_remap_record_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_remap_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_remap_put_dev(handle, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_remap_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_remap_put_plane_c
      type(c_ptr), value :: handle, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_remap_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_remap_records_dev(m, nplanes, planes, consumer_stream) &
        bind(C, name="mckpp_hip_multi_remap_records_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_remap_record_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_remap_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_remap_put_dev(m, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_multi_remap_put_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_remap_put_plane_c
      type(c_ptr), value :: m, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_remap_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! a caller grid and a caller axis in one call (include/mckpp_hip_hv.h): vertical first on the way out, horizontal
    ! first on the way in, with the ordering of mckpp_hip_hgrid_fetch_dev and of mckpp_hip_put_dev
    function mckpp_hip_hv_fetch_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_hv_fetch_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_hv_put_dev(handle, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_hv_put_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_put_plane_c
      type(c_ptr), value :: handle, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hv_fetch_dev(m, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_multi_hv_fetch_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_hv_put_dev(m, nplanes, planes, producer_stream) bind(C, name="mckpp_hip_multi_hv_put_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_put_plane_c
      type(c_ptr), value :: m, producer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_put_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    ! completed records on a caller axis (include/mckpp_hip_vrecords.h): the record's value, then the vertical
    ! interpolation, then - on a caller grid - the row sum, with the ordering of mckpp_hip_records_dev
    function mckpp_hip_vrecords_vaxis_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_vrecords_vaxis_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_record_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vrecords_vaxis_host(handle, nplanes, planes) bind(C, name="mckpp_hip_vrecords_vaxis_host") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_record_plane_c
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_vrecords_hv_dev(handle, nplanes, planes, consumer_stream) bind(C, name="mckpp_hip_vrecords_hv_dev") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_record_plane_c
      type(c_ptr), value :: handle, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vrecords_vaxis_dev(m, nplanes, planes, consumer_stream) &
        bind(C, name="mckpp_hip_multi_vrecords_vaxis_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_record_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vrecords_vaxis_host(m, nplanes, planes) bind(C, name="mckpp_hip_multi_vrecords_vaxis_host") &
        result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_vaxis_record_plane_c
      type(c_ptr), value :: m
      integer(c_int32_t), value :: nplanes
      type(mckpp_vaxis_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
    function mckpp_hip_multi_vrecords_hv_dev(m, nplanes, planes, consumer_stream) &
        bind(C, name="mckpp_hip_multi_vrecords_hv_dev") result(rc)
      import :: c_int, c_int32_t, c_ptr, mckpp_hv_record_plane_c
      type(c_ptr), value :: m, consumer_stream
      integer(c_int32_t), value :: nplanes
      type(mckpp_hv_record_plane_c), intent(in) :: planes(*)
      integer(c_int) :: rc
    end function
  end interface

contains

  !> Text of the last error as a Fortran string.
  function mckpp_hip_error_text() result(txt)
    character(len=:), allocatable :: txt
    character(kind=c_char), pointer :: p(:)
    type(c_ptr) :: cp
    integer :: n
    cp = mckpp_hip_last_error()
    txt = ''
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, p, [512])
    n = 0
    do while (n < 512)
      if (p(n+1) == c_null_char) exit
      n = n + 1
    end do
    allocate (character(len=n) :: txt)
    txt = transfer(p(1:n), txt)
  end function mckpp_hip_error_text

end module mckpp_hip_binding
