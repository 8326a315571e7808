! TEST INFRASTRUCTURE - not part of the product path, own source.
!
! A stand-in for the `netcdf` module of netcdf-fortran.  It exists so that
! `USE netcdf` in the reference's mckpp_netcdf_read resolves, which lets
! oracle/Makefile target `ref` build the reference's physics step, its init
! and its flux reader from the reference's own sources.  It declares the names
! that module uses and nothing more.
!
! It serves ONE file, held in memory: the surface-flux file that
! oracle/ref_step_shim.F90 (ref_loop_flux_file) registers with standin_register,
!   dimensions  longitude (nx), latitude (ny), time (ntimes), each with its
!               coordinate variable of the same name,
!   variables   taux, tauy, swf, lwf, lhf, shf, precip as (nx, ny, ntimes),
! opened by the name it was registered under and read through nf90_get_var
! into a rank-1 real array, whole (a coordinate) or as the hyperslab that
! start/count name (a flux record).  That is all the reference's flux reader
! (src/mckpp_read_fluxes_mod.F90) asks of a file.  Every other call - another
! file name, an unknown dimension or variable, a hyperslab outside the
! registered extents or larger than the array it goes to, a read into an array
! of another rank or type, any call with nothing registered - fails: it returns
! a non-zero status and reads nothing.  The physics step never opens a file.
!
! Compiled with -fdefault-real-8 like the reference, so REAL is what its REAL is.

module netcdf
  implicit none
  private
  public :: nf90_noerr, nf90_nowrite, nf90_open, nf90_close, nf90_inq_dimid, nf90_inq_varid, &
            nf90_inquire_dimension, nf90_strerror, nf90_get_var
  public :: standin_register, standin_clear

  integer, parameter :: nf90_noerr = 0, nf90_nowrite = 0
  integer, parameter :: standin_err = -1   ! what every failing call returns
  integer, parameter :: the_ncid = 7       ! the one file

  ! variable ids: 1..3 the coordinates (= dimension ids), 4..10 the flux fields
  integer, parameter :: nvars = 10, ndims = 3
  character(len=9), parameter :: var_names(nvars) = [character(len=9) :: 'longitude', 'latitude', 'time', &
      'taux', 'tauy', 'swf', 'lwf', 'lhf', 'shf', 'precip']

  logical :: registered = .false., is_open = .false.
  character(len=200) :: file_name = ''
  integer :: dim_len(ndims) = 0
  real, allocatable :: lon(:), lat(:), times(:), flux(:, :, :, :)   ! flux(nx, ny, ntimes, 7)

  ! one specific per rank and type the reference's mckpp_netcdf_read reads into
  interface nf90_get_var
    module procedure get_var_real_1d, get_var_real_2d, get_var_real_3d, get_var_real_4d, &
                     get_var_int_1d, get_var_int_2d
  end interface nf90_get_var

contains

  ! the file `name`: coordinates lon_in(nx), lat_in(ny), times_in(ntimes) and flux_in(nx, ny, ntimes, 7) in the
  ! order taux, tauy, swf, lwf, lhf, shf, precip (copied: the caller's buffers need not outlive the call)
  subroutine standin_register(name, nx, ny, ntimes, lon_in, lat_in, times_in, flux_in)
    character(len=*), intent(in) :: name
    integer, intent(in) :: nx, ny, ntimes
    real, intent(in) :: lon_in(nx), lat_in(ny), times_in(ntimes), flux_in(nx, ny, ntimes, 7)
    call standin_clear()
    file_name = name
    dim_len = [nx, ny, ntimes]
    lon = lon_in
    lat = lat_in
    times = times_in
    flux = flux_in
    registered = .true.
  end subroutine standin_register

  subroutine standin_clear()
    registered = .false.
    is_open = .false.
    file_name = ''
    dim_len = 0
    if (allocated(lon)) deallocate(lon)
    if (allocated(lat)) deallocate(lat)
    if (allocated(times)) deallocate(times)
    if (allocated(flux)) deallocate(flux)
  end subroutine standin_clear

  logical function usable(ncid)
    integer, intent(in) :: ncid
    usable = registered .and. is_open .and. ncid == the_ncid
  end function usable

  integer function find_var(name)
    character(len=*), intent(in) :: name
    integer :: i
    find_var = 0
    do i = 1, nvars
      if (trim(name) == trim(var_names(i))) find_var = i
    end do
  end function find_var

  integer function nf90_open(path, mode, ncid)
    character(len=*), intent(in) :: path
    integer, intent(in) :: mode
    integer, intent(out) :: ncid
    ncid = -1
    nf90_open = standin_err
    if (.not. registered .or. mode /= nf90_nowrite) return
    if (trim(path) /= trim(file_name)) return
    is_open = .true.
    ncid = the_ncid
    nf90_open = nf90_noerr
  end function nf90_open

  integer function nf90_close(ncid)
    integer, intent(in) :: ncid
    nf90_close = standin_err
    if (.not. usable(ncid)) return
    is_open = .false.
    nf90_close = nf90_noerr
  end function nf90_close

  integer function nf90_inq_dimid(ncid, name, dimid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: dimid
    dimid = -1
    nf90_inq_dimid = standin_err
    if (.not. usable(ncid)) return
    if (find_var(name) < 1 .or. find_var(name) > ndims) return
    dimid = find_var(name)
    nf90_inq_dimid = nf90_noerr
  end function nf90_inq_dimid

  integer function nf90_inq_varid(ncid, name, varid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: varid
    varid = -1
    nf90_inq_varid = standin_err
    if (.not. usable(ncid)) return
    if (find_var(name) < 1) return
    varid = find_var(name)
    nf90_inq_varid = nf90_noerr
  end function nf90_inq_varid

  integer function nf90_inquire_dimension(ncid, dimid, name, len)
    integer, intent(in) :: ncid, dimid
    character(len=*), intent(out), optional :: name
    integer, intent(out), optional :: len
    if (present(len)) len = 0
    if (present(name)) name = ''
    nf90_inquire_dimension = standin_err
    if (.not. usable(ncid)) return
    if (dimid < 1 .or. dimid > ndims) return
    if (present(len)) len = dim_len(dimid)
    if (present(name)) name = var_names(dimid)
    nf90_inquire_dimension = nf90_noerr
  end function nf90_inquire_dimension

  function nf90_strerror(status) result(msg)
    integer, intent(in) :: status
    character(len=80) :: msg
    msg = 'netcdf stand-in: not the registered in-memory flux file, or outside it'
  end function nf90_strerror

  ! the only read that is served: values(:) <- a coordinate (start/count of one entry, or none: all of it)
  ! or the (count(1), count(2), count(3)) block at start(1:3) of a flux field, first index fastest
  integer function get_var_real_1d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    real, intent(inout) :: values(:)
    integer, intent(in), optional :: start(:), count(:)
    integer :: s(3), c(3), i, j, t, n, nd
    get_var_real_1d = standin_err
    if (.not. usable(ncid)) return
    if (varid < 1 .or. varid > nvars) return
    nd = merge(1, 3, varid <= ndims)
    s = 1
    if (nd == 1) then
      c = [dim_len(varid), 1, 1]
    else
      c = dim_len
    end if
    if (present(start)) then
      if (size(start) /= nd) return
      s(1:nd) = start
    end if
    if (present(count)) then
      if (size(count) /= nd) return
      c(1:nd) = count
    end if
    if (any(s < 1) .or. any(c < 1)) return
    if (nd == 1) then
      if (s(1) + c(1) - 1 > dim_len(varid)) return
    else
      if (any(s + c - 1 > dim_len)) return
    end if
    if (product(c) > size(values)) return
    if (nd == 1) then
      select case (varid)
      case (1); values(1:c(1)) = lon(s(1):s(1) + c(1) - 1)
      case (2); values(1:c(1)) = lat(s(1):s(1) + c(1) - 1)
      case (3); values(1:c(1)) = times(s(1):s(1) + c(1) - 1)
      end select
    else
      n = 0
      do t = s(3), s(3) + c(3) - 1
        do j = s(2), s(2) + c(2) - 1
          do i = s(1), s(1) + c(1) - 1
            n = n + 1
            values(n) = flux(i, j, t, varid - ndims)
          end do
        end do
      end do
    end if
    get_var_real_1d = nf90_noerr
  end function get_var_real_1d

  ! no registered variable is read into these: they exist so that the reference's generic calls resolve
  integer function get_var_real_2d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    real, intent(inout) :: values(:, :)
    integer, intent(in), optional :: start(:), count(:)
    get_var_real_2d = standin_err
  end function get_var_real_2d

  integer function get_var_real_3d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    real, intent(inout) :: values(:, :, :)
    integer, intent(in), optional :: start(:), count(:)
    get_var_real_3d = standin_err
  end function get_var_real_3d

  integer function get_var_real_4d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    real, intent(inout) :: values(:, :, :, :)
    integer, intent(in), optional :: start(:), count(:)
    get_var_real_4d = standin_err
  end function get_var_real_4d

  integer function get_var_int_1d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    integer, intent(inout) :: values(:)
    integer, intent(in), optional :: start(:), count(:)
    get_var_int_1d = standin_err
  end function get_var_int_1d

  integer function get_var_int_2d(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    integer, intent(inout) :: values(:, :)
    integer, intent(in), optional :: start(:), count(:)
    get_var_int_2d = standin_err
  end function get_var_int_2d

end module netcdf
