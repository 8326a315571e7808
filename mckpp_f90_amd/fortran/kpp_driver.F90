!> Forced column-physics run on the Fortran call surface, shaped like the
!! reference's main program (src/mckpp_ocean_model_3D.F90:23-70) minus file I/O:
!!   dimensions -> allocate -> grid -> lookup -> initial profiles ->
!!   mckpp_initialize_ocean_model -> DO nt: ntime, forcing, mckpp_physics_driver
!! Inputs come from a flat binary file written by the test harness so that the
!! bits are identical to the ones the C-ABI tests use; results go to a second
!! flat file.  Usage: kpp_driver <case.bin> <out.bin>
program kpp_driver
  use iso_c_binding
  use mckpp_parameters
  use mckpp_data_fields
  use mckpp_time_control
  use mckpp_hip_binding, only: MCKPP_F_SCALARS, mckpp_anc_epoch_c, MCKPP_ANC_SST0, MCKPP_ANC_OCNT_CLIM, MCKPP_EXP_F64
  use mckpp_physics_lookup_mod, only: mckpp_physics_lookup
  use mckpp_initialize_ocean, only: mckpp_initialize_ocean_model
  use mckpp_physics_driver_mod, only: mckpp_physics_driver, mckpp_physics_finalize
  use mckpp_physics_ocnstep_mod, only: mckpp_physics_ocnstep
  use mckpp_physics_verticalmixing_mod, only: mckpp_physics_verticalmixing
  use mckpp_fluxes_mod, only: mckpp_fluxes
  use mckpp_hip_session, only: mckpp_hip_ndevices, mckpp_hip_device_list, mckpp_hip_gather_field, mckpp_hip_sync_host, &
                               mckpp_hip_output_mask, mckpp_hip_host_behind, &
                               mckpp_hip_all_set_flux_series, mckpp_hip_all_run_forced, mckpp_hip_all_window_select, &
                               mckpp_hip_all_window_reset, mckpp_hip_all_window_accumulate, mckpp_hip_all_window_fetch, &
                               mckpp_hip_all_window_schedule, mckpp_hip_all_window_record_fetch, &
                               mckpp_hip_all_window_schedule_zoom, mckpp_hip_all_window_zoom, &
                               mckpp_hip_all_window_record_release, mckpp_hip_all_window_export, &
                               mckpp_hip_all_window_export_fetch, mckpp_hip_all_restart_schedule, &
                               mckpp_hip_all_restart_snapshots, mckpp_hip_all_restart_snapshot_save, &
                               mckpp_hip_all_restart_snapshot_release, mckpp_hip_all_step_log, &
                               mckpp_hip_all_set_ancillary_series, mckpp_hip_all_ancillary_schedule, &
                               mckpp_hip_push_ancillaries, mckpp_hip_ancillaries_every_step, &
                               mckpp_hip_all_flux_ring, mckpp_hip_all_flux_ring_put
  implicit none
  character(len=512) :: fin, fout
  integer :: u, nt, nsteps, ncol, nlev, use_1d, ipt, flags
  integer(c_int) :: hdr(8)
  real(c_double), allocatable :: sf6(:,:), mask(:), series(:,:,:)
  type(kpp_1d_type) :: q
  real(c_double) :: t0, t1
  real(c_double), allocatable :: vm_h(:), vm_k(:), vm_difm(:,:), vm_difs(:,:), vm_dift(:,:), vm_ghat(:,:)
  real(c_double) :: hmixn
  integer :: kmixn, snap_first, snap_last, ncut, nrec, r, i
  real(c_double), allocatable :: exp_h(:,:), exp_t(:,:,:)   ! flag 4096: the records fetched through the export
  character(len=16) :: snap_name
  integer(c_int32_t), allocatable :: zoom_pts(:)   ! flag 32768: the schedule's points
  integer(c_int64_t) :: zoom_npoints, zoom_bytes
  integer :: zoom_lev0, zoom_nlev
  ! flag 2048: records of SST0 (npts, nrec) and ocnT_clim (npts, nzp1, nrec) and the epochs of ocnT_clim
  integer, parameter :: anc_cad_sst = 3, anc_cad_ocnt = 2
  real(c_double), allocatable :: anc_sst(:,:), anc_ocnt(:,:,:)
  type(mckpp_anc_epoch_c), allocatable :: anc_ep_sst(:), anc_ep_ocnt(:)

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read (u) hdr
  ncol = hdr(1); nlev = hdr(2); nsteps = hdr(3); use_1d = hdr(4)
  ! flags: 1 forcing through mckpp_fluxes (constant forcing, L_FLUXDATA=.F.) every step; 2 L_VARY_BOTTOM_TEMP;
  !        4 after the run, mckpp_physics_verticalmixing on every column of the final state (appended to the output)
  !        8 hmix and T also through the output gather (appended); 16 the time loop as ONE forced run from flux
  !        records resident on the devices (constant forcing, the records mckpp_fluxes would assemble each step);
  !        32 the same step by step with an output window: mean hmix and maximum T of the run (appended)
  !        64 opt into the reduced per-step download (scalar group only) + mckpp_hip_sync_host before the output;
  !           without it every call of mckpp_physics_driver leaves all of kpp_3d_fields current, as the reference does
  !        128 itermax = 4 (columns run beyond itermax+1 passes: the reference's located warnings on stderr) with
  !           dlon = 0.5 ipt, dlat = -60 + 0.25 ipt
  !        256 flag 32's output (mean hmix, maximum T) from ONE forced run under an output schedule of period 2: every
  !           record of the run (appended, record after record)
  !        512 the time loop as ONE forced run under a restart schedule of period 2 (MOD(ntime, 2) == 0 of
  !           mckpp_restart_control); after it every snapshot s goes to <out.bin>.rst<s> (one file per shard)
  !        1024 the time loop as ONE forced run under a step log of ncol * nsteps records: with flag 128 the located
  !           warnings of every step of the run, not only of its last
  !        4096 with 256: the schedule's records through its export (land value -1): the steps as TWO forced runs, the
  !           second begun inside a window, and the first run's records fetched while the second is queued; the same
  !           appended records as flag 256 alone
  !        2048 L_RELAX_SST and L_RELAX_OCNT with SST0 changing every 3 steps (record after record) and ocnT_clim every 2
  !           (interpolated between two records, mckpp_boundary_interpolate_temp's sum), the records made from the
  !           case's own profiles.  With 16 the one forced run reads them from resident series under schedules; with 1
  !           the per-step driver gets the same fields through mckpp_hip_push_ancillaries at those cadences
  !        8192 with 16: ndtocn = 2 and flux records that change with their number r (from 0): swf = 200 + 25 r,
  !           taux = 0.01 (1 + 0.1 r); all of them resident (mckpp_hip_all_set_flux_series), the time loop ONE forced run
  !        16384 with 8192: the records through a flux ring of 2 slots instead: two records put, the forced run of their
  !           four steps, and so on - the next pair is put while that run is queued
  !        32768 with 256: the schedule zoomed to every third point in descending order (the last point first) and to
  !           levels 0..1; its records out(npoints) and out(npoints, 2) appended as flag 256's are
  flags = hdr(6)
  if (iand(flags, 64) /= 0) mckpp_hip_output_mask = MCKPP_F_SCALARS
  ! hdr(7) > 0: that many device shards; hdr(8) = 1 puts them all on HIP device 0 (one-GPU rehearsal of the
  ! multi-device path), otherwise devices 0 .. hdr(7)-1
  if (hdr(7) > 0) then
    mckpp_hip_ndevices = hdr(7)
    if (hdr(8) == 1) then
      allocate (mckpp_hip_device_list(hdr(7)))
      mckpp_hip_device_list = 0
    end if
  end if
  call mckpp_set_dimensions(ncol, 1, nlev, hdr(5))
  if (iand(flags, 128) /= 0) itermax = 4
  call mckpp_allocate_const_fields()
  call mckpp_allocate_3d_fields()
  read (u) kpp_const_fields%dto
  read (u) kpp_const_fields%zm, kpp_const_fields%hm, kpp_const_fields%dm
  read (u) kpp_3d_fields%U, kpp_3d_fields%X
  read (u) kpp_3d_fields%f, kpp_3d_fields%Sref, kpp_3d_fields%SSref, kpp_3d_fields%Ssurf, kpp_3d_fields%ocdepth
  read (u) kpp_3d_fields%jerlov
  allocate (mask(ncol), sf6(ncol, 6))
  read (u) mask
  read (u) sf6
  close (u)
  kpp_3d_fields%run_physics = mask > 0.5_c_double
  kpp_3d_fields%l_ocean = kpp_3d_fields%run_physics
  kpp_3d_fields%U_init = kpp_3d_fields%U
  if (iand(flags, 128) /= 0) then
    kpp_3d_fields%dlon = [(0.5_c_double * ipt, ipt = 1, ncol)]
    kpp_3d_fields%dlat = [(-60 + 0.25_c_double * ipt, ipt = 1, ncol)]
  end if
  if (iand(flags, 2) /= 0) then
    call mckpp_allocate_3d_optional()
    kpp_const_fields%L_VARY_BOTTOM_TEMP = .true.
    kpp_3d_fields%bottom_temp = kpp_3d_fields%X(:, nzp1, 1) + 0.125_c_double
  end if
  if (iand(flags, 2048) /= 0) then
    if (iand(flags, 2) == 0) call mckpp_allocate_3d_optional()
    kpp_const_fields%L_RELAX_SST = .true.
    kpp_const_fields%L_RELAX_OCNT = .true.
    kpp_3d_fields%relax_sst = 1 / (5 * 86400._c_double)
    kpp_3d_fields%relax_ocnT = 1 / (30 * 86400._c_double)
    call make_ancillary_records()
    call ancillaries_of_step(1)   ! epoch 0: the fields the run is initialised with
    mckpp_hip_ancillaries_every_step = .false.
  end if
  kpp_3d_fields%sflux = 0
  kpp_3d_fields%sflux(:, :, 5, 0) = 1e-20_c_double      ! mckpp_initialize_fluxes, src/mckpp_fluxes_mod.F90:19-32

  call mckpp_physics_lookup(kpp_const_fields)
  ntime = 0
  call mckpp_initialize_ocean_model()

  kpp_3d_fields%sflux(:, 1:6, 5, 0) = sf6
  call cpu_time(t0)
  if (iand(flags, 48 + 256 + 512 + 1024) /= 0) then   ! the reference's loop (src/mckpp_ocean_model_3D.F90:38-58) on the devices
    nrec = 1
    if (iand(flags, 8192) /= 0) nrec = (nsteps + 1) / 2
    allocate (series(ncol, 8, nrec))
    series(:, 1, :) = 0.01_c_double; series(:, 2, :) = 0; series(:, 3, :) = 200; series(:, 4, :) = 0
    series(:, 5, :) = -150; series(:, 6, :) = 0; series(:, 7, :) = 6e-5_c_double; series(:, 8, :) = 0
    if (iand(flags, 8192) /= 0) then
      do r = 0, nrec - 1
        series(:, 3, r + 1) = 200 + 25._c_double * r
        series(:, 1, r + 1) = 0.01_c_double * (1 + 0.1_c_double * r)
      end do
    end if
    if (iand(flags, 8192 + 16384) /= 8192 + 16384) call mckpp_hip_all_set_flux_series(0, nrec, series)
    if (iand(flags, 1024) /= 0) call mckpp_hip_all_step_log(ncol * nsteps, 0)
    if (iand(flags, 2048) /= 0) then   ! the records resident, every column-step reads its own epoch's
      call mckpp_hip_all_set_ancillary_series(MCKPP_ANC_SST0, 0, size(anc_sst, 2), anc_sst)
      call mckpp_hip_all_ancillary_schedule(MCKPP_ANC_SST0, 1, anc_cad_sst, 0, size(anc_ep_sst), anc_ep_sst)
      call mckpp_hip_all_set_ancillary_series(MCKPP_ANC_OCNT_CLIM, 0, size(anc_ocnt, 3), anc_ocnt)
      call mckpp_hip_all_ancillary_schedule(MCKPP_ANC_OCNT_CLIM, 1, anc_cad_ocnt, 0, size(anc_ep_ocnt), anc_ep_ocnt)
    end if
    if (iand(flags, 32) /= 0) then
      call mckpp_hip_all_window_select([4_c_int32_t, 2_c_int32_t])   ! MCKPP_OUT_HMIX, MCKPP_OUT_T
      call mckpp_hip_all_window_reset()
      do nt = 1, nsteps
        call mckpp_hip_all_run_forced(nt, 1, nsteps + 1)
        call mckpp_hip_all_window_accumulate()
      end do
    else if (iand(flags, 256) /= 0) then   ! the same output, accumulated inside the one forced run
      if (iand(flags, 32768) /= 0) then
        zoom_pts = [(int(ipt, c_int32_t), ipt = ncol - 1, 0, -3)]
        call mckpp_hip_all_window_schedule_zoom(0, 1, 2, nsteps / 2, [4_c_int32_t, 2_c_int32_t], [1_c_int32_t, 4_c_int32_t], &
                                                points=zoom_pts, lev0=0, nlev=2)
        call mckpp_hip_all_window_zoom(0, zoom_npoints, zoom_lev0, zoom_nlev, zoom_bytes)
        write (*, '(a,i0,a,i0,a,i0,a,i0,a)') 'kpp_driver: schedule 0 zoomed to ', zoom_npoints, ' points, levels ', zoom_lev0, &
              '..', zoom_lev0 + zoom_nlev - 1, ', ', zoom_bytes, ' bytes of records'
      else
      call mckpp_hip_all_window_schedule(0, 1, 2, nsteps / 2, [4_c_int32_t, 2_c_int32_t], &   ! MCKPP_OUT_HMIX, MCKPP_OUT_T
                                         [1_c_int32_t, 4_c_int32_t])                          ! MCKPP_WIN_MEAN, MCKPP_WIN_MAX
      end if
      if (iand(flags, 4096) /= 0 .and. nsteps >= 4 .and. iand(flags, 32768) == 0) then
        allocate (exp_h(ncol, nsteps / 2), exp_t(ncol, nzp1, nsteps / 2))
        call mckpp_hip_all_window_export(0, MCKPP_EXP_F64, -1._c_double)
        ncut = ior(nsteps / 2, 1)   ! odd: the window of steps ncut, ncut + 1 is cut by the two runs
        call mckpp_hip_all_run_forced(1, ncut, nsteps + 1)
        call mckpp_hip_all_run_forced(ncut + 1, nsteps - ncut, nsteps + 1)
        do nt = 0, ncut / 2 - 1   ! the first run's records, while the second run is queued
          call mckpp_hip_all_window_export_fetch(0, nt, 4, 0, exp_h(:, nt + 1))
          call mckpp_hip_all_window_export_fetch(0, nt, 2, 2, exp_t(:, :, nt + 1))
        end do
        if (ncut / 2 > 0) call mckpp_hip_all_window_record_release(0, ncut / 2 - 1)
        do nt = ncut / 2, nsteps / 2 - 1
          call mckpp_hip_all_window_export_fetch(0, nt, 4, 0, exp_h(:, nt + 1))
          call mckpp_hip_all_window_export_fetch(0, nt, 2, 2, exp_t(:, :, nt + 1))
        end do
      else
        call mckpp_hip_all_run_forced(1, nsteps, nsteps + 1)
      end if
    else if (iand(flags, 512) /= 0) then   ! restart output inside the one forced run
      call mckpp_hip_all_restart_schedule(1, 2, max(1, nsteps / 2))
      call mckpp_hip_all_run_forced(1, nsteps, nsteps + 1)
      call mckpp_hip_all_restart_snapshots(snap_first, snap_last)
      do nt = snap_first, snap_last
        write (snap_name, '(i0)') nt
        call mckpp_hip_all_restart_snapshot_save(nt, trim(fout)//'.rst'//trim(snap_name))
      end do
      call mckpp_hip_all_restart_snapshot_release(snap_last)
    else if (iand(flags, 8192 + 16384) == 8192 + 16384) then   ! the records through the ring, a pair per forced run
      call mckpp_hip_all_flux_ring(2)
      do r = 0, nrec - 1, 2
        do i = r, min(r + 1, nrec - 1)   ! (but for the first pair: while the run before is queued)
          call mckpp_hip_all_flux_ring_put(i, series(:, :, i + 1))
        end do
        call mckpp_hip_all_run_forced(2 * r + 1, min(4, nsteps - 2 * r), 2)
      end do
    else if (iand(flags, 8192) /= 0) then   ! ... and all of them resident
      call mckpp_hip_all_run_forced(1, nsteps, 2)
    else
      call mckpp_hip_all_run_forced(1, nsteps, nsteps + 1)   ! one flux update (step 1), as ndtocn > nsteps
    end if
    nsteps = 0
  end if
  do nt = 1, nsteps
    call mckpp_update_time(nt)
    if (iand(flags, 1) /= 0) call mckpp_fluxes()      ! ndtocn = 1 (src/mckpp_ocean_model_3D.F90:44-48)
    if (iand(flags, 2048) /= 0 .and. nt > 1) then     ! mckpp_boundary_update's place (src/mckpp_ocean_model_3D.F90:51-55)
      if (mod(nt - 1, anc_cad_sst) == 0 .or. mod(nt - 1, anc_cad_ocnt) == 0) then
        call ancillaries_of_step(nt)
        call mckpp_hip_push_ancillaries()
      end if
    end if
    if (use_1d == 0) then
      call mckpp_physics_driver()
    else
      ! the reference's inner loop body, one column at a time (physics_driver_mod.F90:46-63)
      do ipt = 1, npts
        if (.not. kpp_3d_fields%run_physics(ipt)) cycle
        call gather_1d(ipt, q)
        call mckpp_physics_ocnstep(q, kpp_const_fields)
        call scatter_1d(ipt, q)
      end do
    end if
  end do
  call cpu_time(t1)
  write (*, '(a,i0,a,i0,a,i0,a,f8.3,a)') 'kpp_driver: ', ncol, ' columns x ', nlev, ' levels, ', nsteps, &
        ' steps, ', t1 - t0, ' s host time'
  write (*, '(a,3es14.6)') 'kpp_driver: hmix min/mean/max ', minval(kpp_3d_fields%hmix, kpp_3d_fields%run_physics), &
        sum(kpp_3d_fields%hmix)/max(1, count(kpp_3d_fields%run_physics)), maxval(kpp_3d_fields%hmix)

  if (iand(flags, 64 + 48 + 256 + 512 + 1024) == 0 .and. mckpp_hip_host_behind() /= 0) then   ! the default mask: nothing may be stale
    write (0, '(a,i0)') 'kpp_driver: kpp_3d_fields is behind the device after mckpp_physics_driver: ', mckpp_hip_host_behind()
    error stop 2
  end if
  call mckpp_hip_sync_host()   ! what a reduced per-step download or the forced run left on the devices
  open (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write (u) kpp_3d_fields%U, kpp_3d_fields%X, kpp_3d_fields%Us, kpp_3d_fields%Xs
  write (u) kpp_3d_fields%hmix, kpp_3d_fields%kmix, kpp_3d_fields%hmixd, kpp_3d_fields%Tref, kpp_3d_fields%Ssurf
  write (u) kpp_3d_fields%old, kpp_3d_fields%new
  write (u) kpp_3d_fields%difm, kpp_3d_fields%ghat, kpp_3d_fields%rho
  if (iand(flags, 8) /= 0) then   ! the output gather (hmix, T) over the device interconnect instead of the download
    allocate (vm_h(ncol), vm_difm(ncol, nzp1))
    vm_h = -1; vm_difm = -1
    call mckpp_hip_gather_field(4, max(0, mckpp_hip_ndevices - 1), vm_h)
    call mckpp_hip_gather_field(2, 0, vm_difm)
    write (u) vm_h, vm_difm
    deallocate (vm_h, vm_difm)
  end if
  if (iand(flags, 32) /= 0) then
    allocate (vm_h(ncol), vm_difm(ncol, nzp1))
    vm_h = -1; vm_difm = -1
    call mckpp_hip_all_window_fetch(4, 0, vm_h)
    call mckpp_hip_all_window_fetch(2, 2, vm_difm)
    write (u) vm_h, vm_difm
    deallocate (vm_h, vm_difm)
  end if
  if (iand(flags, 256) /= 0) then
    if (allocated(zoom_pts)) then
      allocate (vm_h(size(zoom_pts)), vm_difm(size(zoom_pts), 2))
    else
      allocate (vm_h(ncol), vm_difm(ncol, nzp1))
    end if
    do nt = 0, hdr(3) / 2 - 1
      if (allocated(exp_h)) then
        write (u) exp_h(:, nt + 1), exp_t(:, :, nt + 1)
        cycle
      end if
      vm_h = -1; vm_difm = -1
      call mckpp_hip_all_window_record_fetch(0, nt, 4, 0, vm_h)
      call mckpp_hip_all_window_record_fetch(0, nt, 2, 2, vm_difm)
      write (u) vm_h, vm_difm
    end do
    call mckpp_hip_all_window_record_release(0, hdr(3) / 2 - 1)
    deallocate (vm_h, vm_difm)
  end if
  if (iand(flags, 4) /= 0) then
    allocate (vm_h(ncol), vm_k(ncol), vm_difm(ncol,0:nztmax), vm_difs(ncol,0:nztmax), vm_dift(ncol,0:nztmax), vm_ghat(ncol,nztmax))
    vm_h = 0; vm_k = 0; vm_difm = 0; vm_difs = 0; vm_dift = 0; vm_ghat = 0
    do ipt = 1, npts
      if (.not. kpp_3d_fields%run_physics(ipt)) cycle
      call gather_1d(ipt, q)
      call mckpp_physics_verticalmixing(q, kpp_const_fields, hmixn, kmixn)
      vm_h(ipt) = hmixn; vm_k(ipt) = kmixn
      vm_difm(ipt,:) = q%difm; vm_difs(ipt,:) = q%difs; vm_dift(ipt,:) = q%dift; vm_ghat(ipt,:) = q%ghat
    end do
    write (u) vm_h, vm_k, vm_difm, vm_difs, vm_dift, vm_ghat
  end if
  close (u)
  call mckpp_physics_finalize()

contains

  !> flag 2048: record r of SST0 is T(:,1) + 1.5 + r/4, of ocnT_clim T - 0.3 + r/8 (the case's starting T); SST0's epoch e
  !! is record e, ocnT_clim's is record(e/3 + 1) * w + record(e/3) * (1 - w) with w = mod(e, 3) / 3
  subroutine make_ancillary_records()
    integer :: r, e, nes, neo, nro
    nes = (hdr(3) + anc_cad_sst - 1) / anc_cad_sst
    neo = (hdr(3) + anc_cad_ocnt - 1) / anc_cad_ocnt
    nro = (neo - 1) / 3 + 2
    allocate (anc_sst(npts, nes), anc_ocnt(npts, nzp1, nro), anc_ep_sst(nes), anc_ep_ocnt(neo))
    do r = 1, nes
      anc_sst(:, r) = kpp_3d_fields%X(:, 1, 1) + 1.5_c_double + 0.25_c_double * (r - 1)
      anc_ep_sst(r) = mckpp_anc_epoch_c(r - 1, -1, 0._c_double, 0._c_double)
    end do
    do r = 1, nro
      anc_ocnt(:, :, r) = kpp_3d_fields%X(:, :, 1) - 0.3_c_double + 0.125_c_double * (r - 1)
    end do
    do e = 0, neo - 1
      anc_ep_ocnt(e + 1)%rec_prev = e / 3
      anc_ep_ocnt(e + 1)%rec_next = e / 3 + 1
      anc_ep_ocnt(e + 1)%w_next = mod(e, 3) / 3._c_double
      anc_ep_ocnt(e + 1)%w_prev = 1 - anc_ep_ocnt(e + 1)%w_next
    end do
  end subroutine make_ancillary_records

  !> ... and the fields of step n's epochs in kpp_3d_fields, as mckpp_boundary_update would leave them
  !! (src/mckpp_boundary_interpolate.F90:60)
  subroutine ancillaries_of_step(n)
    integer, intent(in) :: n
    type(mckpp_anc_epoch_c) :: ep
    kpp_3d_fields%SST0 = anc_sst(:, anc_ep_sst((n - 1) / anc_cad_sst + 1)%rec_prev + 1)
    ep = anc_ep_ocnt((n - 1) / anc_cad_ocnt + 1)
    kpp_3d_fields%ocnT_clim = anc_ocnt(:, :, ep%rec_next + 1) * ep%w_next + anc_ocnt(:, :, ep%rec_prev + 1) * ep%w_prev
  end subroutine ancillaries_of_step

  subroutine gather_1d(i, c)
    integer, intent(in) :: i
    type(kpp_1d_type), intent(inout) :: c
    call mckpp_allocate_1d_fields(c)
    c%U = kpp_3d_fields%U(i,:,:); c%X = kpp_3d_fields%X(i,:,:); c%U_init = kpp_3d_fields%U_init(i,:,:)
    c%Us = kpp_3d_fields%Us(i,:,:,:); c%Xs = kpp_3d_fields%Xs(i,:,:,:); c%hmixd = kpp_3d_fields%hmixd(i,:)
    c%sflux = kpp_3d_fields%sflux(i,:,:,:)
    c%f = kpp_3d_fields%f(i); c%ocdepth = kpp_3d_fields%ocdepth(i); c%Sref = kpp_3d_fields%Sref(i)
    c%SSref = kpp_3d_fields%SSref(i); c%Ssurf = kpp_3d_fields%Ssurf(i)
    c%hmix = kpp_3d_fields%hmix(i); c%kmix = kpp_3d_fields%kmix(i)
    c%old = kpp_3d_fields%old(i); c%new = kpp_3d_fields%new(i); c%jerlov = kpp_3d_fields%jerlov(i)
    c%l_ocean = kpp_3d_fields%l_ocean(i); c%l_initflag = kpp_3d_fields%l_initflag(i); c%point = i
    c%dlat = kpp_3d_fields%dlat(i); c%dlon = kpp_3d_fields%dlon(i)   ! src/mckpp_types_transfer.F90 (what the warnings name)
  end subroutine gather_1d

  subroutine scatter_1d(i, c)
    integer, intent(in) :: i
    type(kpp_1d_type), intent(in) :: c
    kpp_3d_fields%U(i,:,:) = c%U; kpp_3d_fields%X(i,:,:) = c%X
    kpp_3d_fields%Us(i,:,:,:) = c%Us; kpp_3d_fields%Xs(i,:,:,:) = c%Xs; kpp_3d_fields%hmixd(i,:) = c%hmixd
    kpp_3d_fields%hmix(i) = c%hmix; kpp_3d_fields%kmix(i) = c%kmix; kpp_3d_fields%Tref(i) = c%Tref
    kpp_3d_fields%Ssurf(i) = c%Ssurf; kpp_3d_fields%old(i) = c%old; kpp_3d_fields%new(i) = c%new
    kpp_3d_fields%difm(i,:) = c%difm; kpp_3d_fields%ghat(i,:) = c%ghat; kpp_3d_fields%rho(i,:) = c%rho
  end subroutine scatter_1d

end program kpp_driver
