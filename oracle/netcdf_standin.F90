! TEST INFRASTRUCTURE - not part of the product path, own source.
!
! A stand-in for the `netcdf` module of netcdf-fortran.  It exists only so that
! `USE netcdf` in the reference's mckpp_netcdf_read resolves, which lets
! oracle/Makefile target `ref` build the reference's physics step (ocnstep and
! everything under it) from the reference's own sources.  It declares the names
! that module uses and nothing more, and EVERY call fails (returns a non-zero
! status and reads nothing).  The physics step never opens a file, so none of
! these routines is reached from oracle/ref_step_shim.F90.

module netcdf
  implicit none
  private
  public :: nf90_noerr, nf90_nowrite, nf90_open, nf90_close, nf90_inq_dimid, nf90_inq_varid, &
            nf90_inquire_dimension, nf90_strerror, nf90_get_var

  integer, parameter :: nf90_noerr = 0, nf90_nowrite = 0
  integer, parameter :: standin_err = -1   ! what every call returns

  interface nf90_get_var
    module procedure standin_get_var
  end interface nf90_get_var

contains

  integer function nf90_open(path, mode, ncid)
    character(len=*), intent(in) :: path
    integer, intent(in) :: mode
    integer, intent(out) :: ncid
    ncid = -1
    nf90_open = standin_err
  end function nf90_open

  integer function nf90_close(ncid)
    integer, intent(in) :: ncid
    nf90_close = standin_err
  end function nf90_close

  integer function nf90_inq_dimid(ncid, name, dimid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: dimid
    dimid = -1
    nf90_inq_dimid = standin_err
  end function nf90_inq_dimid

  integer function nf90_inq_varid(ncid, name, varid)
    integer, intent(in) :: ncid
    character(len=*), intent(in) :: name
    integer, intent(out) :: varid
    varid = -1
    nf90_inq_varid = standin_err
  end function nf90_inq_varid

  integer function nf90_inquire_dimension(ncid, dimid, name, len)
    integer, intent(in) :: ncid, dimid
    character(len=*), intent(out), optional :: name
    integer, intent(out), optional :: len
    if (present(len)) len = 0
    nf90_inquire_dimension = standin_err
  end function nf90_inquire_dimension

  function nf90_strerror(status) result(msg)
    integer, intent(in) :: status
    character(len=80) :: msg
    msg = 'netcdf stand-in: no netCDF library in this build'
  end function nf90_strerror

  integer function standin_get_var(ncid, varid, values, start, count)
    integer, intent(in) :: ncid, varid
    type(*), dimension(..), intent(inout) :: values
    integer, intent(in), optional :: start(:), count(:)
    standin_get_var = standin_err
  end function standin_get_var

end module netcdf
