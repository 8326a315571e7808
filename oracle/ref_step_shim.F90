! TEST INFRASTRUCTURE - not part of the product path, own source.
!
! bind(C) entry points into the reference's own physics step, built by
! oracle/Makefile target `ref` together with the reference's sources (read where
! they lie) and oracle/netcdf_standin.F90 into
!   oracle/_ref/libmckpp_ref_step.so       (EXP = libm exp, as amdflang builds the reference)
!   oracle/_ref/libmckpp_ref_step_pexp.so  (EXP = the project's portable exp, through --wrap=exp)
! oracle/orc.py (ref_step) drives them; tests/ compare the oracle and, through
! recorded outputs under tests/golden/, the HIP kernel with them.
!
! The reference works on the module globals kpp_3d_fields / kpp_const_fields
! (src/mckpp_data_fields.F90) sized by the module variables of mckpp_parameters:
!   ref_step_setup   sets the parameters, (re)allocates and zeroes both types, fills
!                    the grid, constants and switches, and calls the reference's
!                    mckpp_physics_lookup for the wmt / wst tables;
!   ref_step_xfer    copies one 3D field in or out by name (Fortran layout, npts fastest);
!   ref_step_run     runs mckpp_physics_driver() for nsteps steps (ntime = ntime0 ...).
! and, for the reference's own init, flux assembly and time loop (oracle/orc.py: ref_init, ref_loop), after a
! ref_step_setup that was handed tri0 = tri1 = 0:
!   ref_loop_config    sets what those routines read beyond the step's (l_fluxdata, l_rest, flsn, el, ndtocn,
!                      startt, spd, dtsec, forcing_file, dlon, dlat, L_RESTART = .false.);
!   ref_loop_flux_file registers the flux records as the in-memory file behind oracle/netcdf_standin.F90, under
!                      the name forcing_file holds, on the longitudes and the latitude ref_loop_config set;
!   ref_loop_init      runs mckpp_initialize_time(), mckpp_initialize_fluxes(), mckpp_initialize_ocean_model()
!                      (src/mckpp_ocean_model_3D.F90:29, src/mckpp_initialize_fields_mod.F90:129-133);
!   ref_loop_tri       reads back tri(:,0,1), tri(:,1,1) as the reference's init computed them;
!   ref_loop_run       the body of the reference's time loop (src/mckpp_ocean_model_3D.F90:38-58 without the
!                      boundary update and the output) for steps nt_first .. nt_first + n - 1, written here in
!                      that order and calling the reference's routines only.
!
! Compiled with -fdefault-real-8, so REAL == c_double.

module ref_step_shim
  use iso_c_binding, only: c_int, c_double, c_char
  use mckpp_parameters
  use mckpp_data_fields, only: kpp_3d_fields, kpp_const_fields, kpp_3d_type, kpp_const_type, &
      mckpp_allocate_3d_fields, mckpp_allocate_const_fields
  implicit none
  private

contains

  ! sw(1:16) = LKPP LRI LDD L_SSref L_RELAX_SST L_RELAX_CALCONLY L_FCORR L_FCORR_WITHZ
  !            L_SFCORR L_SFCORR_WITHZ L_RELAX_SAL L_RELAX_OCNT L_NO_FREEZE L_NO_ISOTHERM
  !            L_DAMP_CURR L_VARY_BOTTOM_TEMP
  ! iv(1:4)  = itermax iso_bot dt_uvdamp clim_present (ocnT_file and sal_file named or 'none')
  ! rv(1:6)  = hmixtolfrac dto grav vonk sice iso_thresh
  ! zm(1:nz+1), hm(1:nz+1), dm(0:nz), tri0(0:nz) = tri(:,0,1), tri1(0:nz) = tri(:,1,1)
  subroutine ref_step_setup(nz_in, npts_in, sw, iv, rv, zm, hm, dm, tri0, tri1) bind(C, name="ref_step_setup")
    use mckpp_physics_lookup_mod, only: mckpp_physics_lookup
    integer(c_int), value :: nz_in, npts_in
    integer(c_int), intent(in) :: sw(16), iv(4)
    real(c_double), intent(in) :: rv(6), zm(nz_in + 1), hm(nz_in + 1), dm(0:nz_in), tri0(0:nz_in), tri1(0:nz_in)
    type(kpp_3d_type) :: empty3d
    type(kpp_const_type) :: emptyc

    ! mckpp_initialize_namelist_mod.F90:28-79, with one grid point per column
    nz = nz_in; nzm1 = nz - 1; nzp1 = nz + 1; ndim = 1
    nx = npts_in; ny = 1; npts = npts_in
    nvel = 2; nsclr = 2; nvp1 = nvel + 1; nsp1 = nsclr + 1; nsb = 0
    itermax = iv(1); hmixtolfrac = rv(1)
    ngrid = 1; nzl = 1; nzu = 2; nzdivmax = 8; nztmax = nz + 1; nzp1tmax = nztmax + 1; igridmax = 5
    nsflxs = 9; njdt = 1; nsflxsm1 = nsflxs - 1; nsflxsp2 = nsflxs + 2; ndharm = 5
    maxmodeadv = 6; mr = 100; mrp1 = mr + 1
    nx_globe = npts; ny_globe = 1; npts_globe = npts

    kpp_3d_fields = empty3d          ! deallocates whatever an earlier setup allocated
    kpp_const_fields = emptyc
    kpp_const_fields%L_COUPLE = .false.
    call mckpp_allocate_3d_fields()
    call mckpp_allocate_const_fields()
    allocate(kpp_const_fields%wmt(0:891, 0:49), kpp_const_fields%wst(0:891, 0:49))
    allocate(kpp_const_fields%tri(0:nztmax, 0:1, ngrid))
    call zero_3d()

    kpp_const_fields%zm = zm
    kpp_const_fields%hm = hm
    kpp_const_fields%dm = dm
    kpp_const_fields%tri = 0.
    kpp_const_fields%tri(0:nz, 0, 1) = tri0
    kpp_const_fields%tri(0:nz, 1, 1) = tri1
    kpp_const_fields%dto = rv(2)
    kpp_const_fields%grav = rv(3)
    kpp_const_fields%vonk = rv(4)
    kpp_const_fields%sice = rv(5)
    kpp_const_fields%iso_thresh = rv(6)
    kpp_const_fields%iso_bot = iv(2)
    kpp_const_fields%dt_uvdamp = iv(3)
    if (iv(4) /= 0) then
      kpp_const_fields%ocnT_file = 'ocnT_clim'
      kpp_const_fields%sal_file = 'sal_clim'
    else
      kpp_const_fields%ocnT_file = 'none'
      kpp_const_fields%sal_file = 'none'
    end if
    kpp_const_fields%LKPP = sw(1) /= 0
    kpp_const_fields%LRI = sw(2) /= 0
    kpp_const_fields%LDD = sw(3) /= 0
    kpp_const_fields%L_SSref = sw(4) /= 0
    kpp_const_fields%L_RELAX_SST = sw(5) /= 0
    kpp_const_fields%L_RELAX_CALCONLY = sw(6) /= 0
    kpp_const_fields%L_FCORR = sw(7) /= 0
    kpp_const_fields%L_FCORR_WITHZ = sw(8) /= 0
    kpp_const_fields%L_SFCORR = sw(9) /= 0
    kpp_const_fields%L_SFCORR_WITHZ = sw(10) /= 0
    kpp_const_fields%L_RELAX_SAL = sw(11) /= 0
    kpp_const_fields%L_RELAX_OCNT = sw(12) /= 0
    kpp_const_fields%L_NO_FREEZE = sw(13) /= 0
    kpp_const_fields%L_NO_ISOTHERM = sw(14) /= 0
    kpp_const_fields%L_DAMP_CURR = sw(15) /= 0
    kpp_const_fields%L_VARY_BOTTOM_TEMP = sw(16) /= 0
    kpp_const_fields%ifirst = 1
    kpp_const_fields%jfirst = 1
    call mckpp_physics_lookup(kpp_const_fields)
  end subroutine ref_step_setup

  subroutine zero_3d()
    associate(f => kpp_3d_fields)
      f%U = 0.; f%X = 0.; f%Rig = 0.; f%dbloc = 0.; f%Shsq = 0.; f%hmixd = 0.; f%Us = 0.; f%Xs = 0.
      f%rho = 0.; f%cp = 0.; f%buoy = 0.; f%rhoh2o = 0.; f%ocdepth = 0.; f%f = 0.; f%swfrac = 0.
      f%swdk_opt = 0.; f%difm = 0.; f%difs = 0.; f%dift = 0.; f%wU = 0.; f%wX = 0.; f%wXNT = 0.
      f%ghat = 0.; f%relax_sst = 0.; f%fcorr = 0.; f%cplwght = 0.; f%SST0 = 0.; f%fcorr_twod = 0.
      f%sfcorr_twod = 0.; f%tinc_fcorr = 0.; f%sinc_fcorr = 0.; f%fcorr_withz = 0.; f%sfcorr = 0.
      f%sfcorr_withz = 0.; f%advection = 0.; f%relax_sal = 0.; f%scorr = 0.; f%relax_ocnT = 0.
      f%ocnTcorr = 0.; f%sal_clim = 0.; f%ocnT_clim = 0.; f%hmix = 0.; f%kmix = 0.; f%Tref = 0.
      f%uref = 0.; f%vref = 0.; f%Ssurf = 0.; f%Sref = 0.; f%SSref = 0.; f%sflux = 0.; f%dlat = 0.
      f%dlon = 0.; f%freeze_flag = 0.; f%reset_flag = 0.; f%dampu_flag = 0.; f%dampv_flag = 0.
      f%U_init = 0.; f%bottom_temp = 0.; f%taux = 0.; f%tauy = 0.; f%swf = 0.; f%lwf = 0.; f%lhf = 0.
      f%shf = 0.; f%rain = 0.; f%snow = 0.; f%sst = 0.; f%iceconc = 0.; f%usf = 0.; f%vsf = 0.
      f%icedepth = 0.; f%snowdepth = 0.
      f%l_ocean = .true.; f%l_initflag = .false.; f%run_physics = .true.
      f%old = 0; f%new = 1; f%jerlov = 3; f%nmodeadv = 0; f%modeadv = 0
    end associate
  end subroutine zero_3d

  ! copy n values between buf and a contiguous field (put /= 0: buf -> field); -1 when sizes differ
  integer function xr(n, a, buf, nbuf, put)
    integer, intent(in) :: n, nbuf, put
    real(c_double), intent(inout) :: a(n), buf(nbuf)
    xr = -1
    if (n /= nbuf) return
    if (put /= 0) then
      a = buf
    else
      buf = a
    end if
    xr = 0
  end function xr

  integer function xi(n, a, buf, nbuf, put)
    integer, intent(in) :: n, nbuf, put
    integer, intent(inout) :: a(n)
    real(c_double), intent(inout) :: buf(nbuf)
    xi = -1
    if (n /= nbuf) return
    if (put /= 0) then
      a = nint(buf)
    else
      buf = real(a, c_double)
    end if
    xi = 0
  end function xi

  integer function xl(n, a, buf, nbuf, put)
    integer, intent(in) :: n, nbuf, put
    logical, intent(inout) :: a(n)
    real(c_double), intent(inout) :: buf(nbuf)
    xl = -1
    if (n /= nbuf) return
    if (put /= 0) then
      a = buf /= 0.
    else
      buf = merge(1._c_double, 0._c_double, a)
    end if
    xl = 0
  end function xl

  ! One field of kpp_3d_fields by its reference name, as doubles in Fortran order (integers and
  ! logicals converted).  Returns 0, or -1 for a size mismatch, -2 for an unknown name.
  integer(c_int) function ref_step_xfer(cname, nlen, buf, nbuf, put) bind(C, name="ref_step_xfer")
    integer(c_int), value :: nlen, nbuf, put
    character(kind=c_char), intent(in) :: cname(nlen)
    real(c_double), intent(inout) :: buf(nbuf)
    character(len=32) :: name
    integer :: i
    name = ''
    do i = 1, min(nlen, 32)
      name(i:i) = cname(i)
    end do
    associate(f => kpp_3d_fields)
      select case (trim(name))
      case ('U');           ref_step_xfer = xr(size(f%U), f%U, buf, nbuf, put)
      case ('X');           ref_step_xfer = xr(size(f%X), f%X, buf, nbuf, put)
      case ('Us');          ref_step_xfer = xr(size(f%Us), f%Us, buf, nbuf, put)
      case ('Xs');          ref_step_xfer = xr(size(f%Xs), f%Xs, buf, nbuf, put)
      case ('U_init');      ref_step_xfer = xr(size(f%U_init), f%U_init, buf, nbuf, put)
      case ('Rig');         ref_step_xfer = xr(size(f%Rig), f%Rig, buf, nbuf, put)
      case ('dbloc');       ref_step_xfer = xr(size(f%dbloc), f%dbloc, buf, nbuf, put)
      case ('Shsq');        ref_step_xfer = xr(size(f%Shsq), f%Shsq, buf, nbuf, put)
      case ('hmixd');       ref_step_xfer = xr(size(f%hmixd), f%hmixd, buf, nbuf, put)
      case ('rho');         ref_step_xfer = xr(size(f%rho), f%rho, buf, nbuf, put)
      case ('cp');          ref_step_xfer = xr(size(f%cp), f%cp, buf, nbuf, put)
      case ('buoy');        ref_step_xfer = xr(size(f%buoy), f%buoy, buf, nbuf, put)
      case ('ocdepth');     ref_step_xfer = xr(size(f%ocdepth), f%ocdepth, buf, nbuf, put)
      case ('f');           ref_step_xfer = xr(size(f%f), f%f, buf, nbuf, put)
      case ('swfrac');      ref_step_xfer = xr(size(f%swfrac), f%swfrac, buf, nbuf, put)
      case ('swdk_opt');    ref_step_xfer = xr(size(f%swdk_opt), f%swdk_opt, buf, nbuf, put)
      case ('difm');        ref_step_xfer = xr(size(f%difm), f%difm, buf, nbuf, put)
      case ('difs');        ref_step_xfer = xr(size(f%difs), f%difs, buf, nbuf, put)
      case ('dift');        ref_step_xfer = xr(size(f%dift), f%dift, buf, nbuf, put)
      case ('wU');          ref_step_xfer = xr(size(f%wU), f%wU, buf, nbuf, put)
      case ('wX');          ref_step_xfer = xr(size(f%wX), f%wX, buf, nbuf, put)
      case ('wXNT');        ref_step_xfer = xr(size(f%wXNT), f%wXNT, buf, nbuf, put)
      case ('ghat');        ref_step_xfer = xr(size(f%ghat), f%ghat, buf, nbuf, put)
      case ('relax_sst');   ref_step_xfer = xr(size(f%relax_sst), f%relax_sst, buf, nbuf, put)
      case ('fcorr');       ref_step_xfer = xr(size(f%fcorr), f%fcorr, buf, nbuf, put)
      case ('SST0');        ref_step_xfer = xr(size(f%SST0), f%SST0, buf, nbuf, put)
      case ('fcorr_twod');  ref_step_xfer = xr(size(f%fcorr_twod), f%fcorr_twod, buf, nbuf, put)
      case ('tinc_fcorr');  ref_step_xfer = xr(size(f%tinc_fcorr), f%tinc_fcorr, buf, nbuf, put)
      case ('sinc_fcorr');  ref_step_xfer = xr(size(f%sinc_fcorr), f%sinc_fcorr, buf, nbuf, put)
      case ('fcorr_withz'); ref_step_xfer = xr(size(f%fcorr_withz), f%fcorr_withz, buf, nbuf, put)
      case ('sfcorr_withz'); ref_step_xfer = xr(size(f%sfcorr_withz), f%sfcorr_withz, buf, nbuf, put)
      case ('advection');   ref_step_xfer = xr(size(f%advection), f%advection, buf, nbuf, put)
      case ('relax_sal');   ref_step_xfer = xr(size(f%relax_sal), f%relax_sal, buf, nbuf, put)
      case ('scorr');       ref_step_xfer = xr(size(f%scorr), f%scorr, buf, nbuf, put)
      case ('relax_ocnT');  ref_step_xfer = xr(size(f%relax_ocnT), f%relax_ocnT, buf, nbuf, put)
      case ('ocnTcorr');    ref_step_xfer = xr(size(f%ocnTcorr), f%ocnTcorr, buf, nbuf, put)
      case ('sal_clim');    ref_step_xfer = xr(size(f%sal_clim), f%sal_clim, buf, nbuf, put)
      case ('ocnT_clim');   ref_step_xfer = xr(size(f%ocnT_clim), f%ocnT_clim, buf, nbuf, put)
      case ('hmix');        ref_step_xfer = xr(size(f%hmix), f%hmix, buf, nbuf, put)
      case ('kmix');        ref_step_xfer = xr(size(f%kmix), f%kmix, buf, nbuf, put)
      case ('Tref');        ref_step_xfer = xr(size(f%Tref), f%Tref, buf, nbuf, put)
      case ('uref');        ref_step_xfer = xr(size(f%uref), f%uref, buf, nbuf, put)
      case ('vref');        ref_step_xfer = xr(size(f%vref), f%vref, buf, nbuf, put)
      case ('Ssurf');       ref_step_xfer = xr(size(f%Ssurf), f%Ssurf, buf, nbuf, put)
      case ('Sref');        ref_step_xfer = xr(size(f%Sref), f%Sref, buf, nbuf, put)
      case ('SSref');       ref_step_xfer = xr(size(f%SSref), f%SSref, buf, nbuf, put)
      case ('sflux');       ref_step_xfer = xr(size(f%sflux), f%sflux, buf, nbuf, put)
      case ('freeze_flag'); ref_step_xfer = xr(size(f%freeze_flag), f%freeze_flag, buf, nbuf, put)
      case ('reset_flag');  ref_step_xfer = xr(size(f%reset_flag), f%reset_flag, buf, nbuf, put)
      case ('dampu_flag');  ref_step_xfer = xr(size(f%dampu_flag), f%dampu_flag, buf, nbuf, put)
      case ('dampv_flag');  ref_step_xfer = xr(size(f%dampv_flag), f%dampv_flag, buf, nbuf, put)
      case ('bottom_temp'); ref_step_xfer = xr(size(f%bottom_temp), f%bottom_temp, buf, nbuf, put)
      case ('old');         ref_step_xfer = xi(size(f%old), f%old, buf, nbuf, put)
      case ('new');         ref_step_xfer = xi(size(f%new), f%new, buf, nbuf, put)
      case ('jerlov');      ref_step_xfer = xi(size(f%jerlov), f%jerlov, buf, nbuf, put)
      case ('nmodeadv');    ref_step_xfer = xi(size(f%nmodeadv), f%nmodeadv, buf, nbuf, put)
      case ('modeadv');     ref_step_xfer = xi(size(f%modeadv), f%modeadv, buf, nbuf, put)
      case ('l_ocean');     ref_step_xfer = xl(size(f%l_ocean), f%l_ocean, buf, nbuf, put)
      case ('l_initflag');  ref_step_xfer = xl(size(f%l_initflag), f%l_initflag, buf, nbuf, put)
      case ('run_physics'); ref_step_xfer = xl(size(f%run_physics), f%run_physics, buf, nbuf, put)
      case default;         ref_step_xfer = -2
      end select
    end associate
  end function ref_step_xfer

  ! nsteps calls of the reference's mckpp_physics_driver (ntime = ntime0, ntime0+1, ...).  The
  ! driver starts and stops named timers, which define themselves on first use in a table of
  ! max_timers entries (src/mckpp_timer.F90): the table is re-initialised for every run, and one
  ! run uses a handful of names however many steps it takes.
  subroutine ref_step_run(ntime0, nsteps) bind(C, name="ref_step_run")
    use mckpp_physics_driver_mod, only: mckpp_physics_driver
    use mckpp_time_control, only: ntime
    use mckpp_timer, only: mckpp_initialize_timers
    integer(c_int), value :: ntime0, nsteps
    integer :: n
    call mckpp_initialize_timers()
    do n = 0, nsteps - 1
      ntime = ntime0 + n
      call mckpp_physics_driver()
    end do
  end subroutine ref_step_run

  ! lv(1:2) = l_fluxdata l_rest;  rv(1:7) = flsn el startt spd dtsec lon0 lat0
  ! (column i lies at longitude lon0 + i - 1 on the one latitude lat0)
  subroutine ref_loop_config(lv, ndtocn_in, rv) bind(C, name="ref_loop_config")
    integer(c_int), intent(in) :: lv(2)
    integer(c_int), value :: ndtocn_in
    real(c_double), intent(in) :: rv(7)
    integer :: i
    kpp_const_fields%l_fluxdata = lv(1) /= 0
    kpp_const_fields%l_rest = lv(2) /= 0
    kpp_const_fields%L_RESTART = .false.
    kpp_const_fields%ndtocn = ndtocn_in
    kpp_const_fields%flsn = rv(1)
    kpp_const_fields%el = rv(2)
    kpp_const_fields%startt = rv(3)
    kpp_const_fields%spd = rv(4)
    kpp_const_fields%dtsec = rv(5)
    kpp_const_fields%forcing_file = 'ref_loop_fluxes.nc'
    do i = 1, npts
      kpp_3d_fields%dlon(i) = rv(6) + (i - 1)
    end do
    kpp_3d_fields%dlat = rv(7)
  end subroutine ref_loop_config

  ! times(1:ntimes) and flux(npts, 1, ntimes, 7) = taux tauy swf lwf lhf shf precip (copied by the stand-in)
  subroutine ref_loop_flux_file(ntimes, times, flux) bind(C, name="ref_loop_flux_file")
    use netcdf, only: standin_register, standin_clear
    integer(c_int), value :: ntimes
    real(c_double), intent(in) :: times(ntimes), flux(nx, ny, ntimes, 7)
    if (ntimes <= 0) then
      call standin_clear()
    else
      call standin_register(trim(kpp_const_fields%forcing_file), nx, ny, ntimes, kpp_3d_fields%dlon(1:nx), &
                            kpp_3d_fields%dlat(1:1), times, flux)
    end if
  end subroutine ref_loop_flux_file

  subroutine ref_loop_init() bind(C, name="ref_loop_init")
    use mckpp_time_control, only: mckpp_initialize_time
    use mckpp_fluxes_mod, only: mckpp_initialize_fluxes
    use mckpp_initialize_ocean, only: mckpp_initialize_ocean_model
    use mckpp_timer, only: mckpp_initialize_timers
    call mckpp_initialize_timers()
    call mckpp_initialize_time()
    call mckpp_initialize_fluxes()
    call mckpp_initialize_ocean_model()
  end subroutine ref_loop_init

  subroutine ref_loop_tri(tri0, tri1) bind(C, name="ref_loop_tri")
    real(c_double), intent(out) :: tri0(0:nz), tri1(0:nz)
    tri0 = kpp_const_fields%tri(0:nz, 0, 1)
    tri1 = kpp_const_fields%tri(0:nz, 1, 1)
  end subroutine ref_loop_tri

  subroutine ref_loop_run(nt_first, n) bind(C, name="ref_loop_run")
    use mckpp_time_control, only: mckpp_update_time
    use mckpp_fluxes_mod, only: mckpp_fluxes
    use mckpp_physics_driver_mod, only: mckpp_physics_driver
    use mckpp_timer, only: mckpp_initialize_timers
    integer(c_int), value :: nt_first, n
    integer :: nt
    call mckpp_initialize_timers()
    do nt = nt_first, nt_first + n - 1
      call mckpp_update_time(nt)
      if (mod(nt - 1, kpp_const_fields%ndtocn) == 0) call mckpp_fluxes()
      call mckpp_physics_driver()
    end do
  end subroutine ref_loop_run

end module ref_step_shim
