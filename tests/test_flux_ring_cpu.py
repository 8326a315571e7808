"""CPU side of the flux-record ring (mckpp_hip_flux_ring): the six entry points refuse a null handle with a message that
names them, the Python wrappers refuse a misshapen record before the library is called, and the Fortran layer builds
with the new bindings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api  # noqa: F401

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    rec = np.zeros((8, 4))
    a, b = C.c_int(7), C.c_int(7)
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "flux_ring": lambda f: f(None, 2),
            "flux_ring_put": lambda f: f(None, 0, rec.ctypes.data_as(C.POINTER(C.c_double))),
            "flux_ring_records": lambda f: f(None, C.byref(a), C.byref(b)),
        }
        for name, call in calls.items():
            entry = pre + name
            assert call(getattr(lib, entry)) < 0, entry
            assert (entry + ": null handle").encode() in lib.mckpp_hip_last_error(), (entry, lib.mckpp_hip_last_error())
    assert (a.value, b.value) == (7, 7)


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_wrappers_check_the_record_first(api, cls):
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h = C.c_void_p()
    h._held = {}
    h._npts = 4
    for bad in (np.zeros(32), np.zeros((4, 8)), np.zeros((8, 5)), np.zeros((2, 8, 4))):
        with pytest.raises(ValueError, match=r"a record is fields\[8, npts"):
            h.flux_ring_put(0, bad)
    # well-formed calls reach the library (and fail there, for the null handle)
    with pytest.raises(api.MckppHipError, match="flux_ring_put: null handle"):
        h.flux_ring_put(0, np.zeros((8, 4)))
    with pytest.raises(api.MckppHipError, match="flux_ring: null handle"):
        h.flux_ring(2)
    with pytest.raises(api.MckppHipError, match="flux_ring_records: null handle"):
        h.flux_ring_records()


def test_fortran_layer_builds_with_the_ring_bindings(built, tmp_path):
    """A program on the session's new wrappers and the binding's new interfaces compiles and links against the layer."""
    src = tmp_path / "uses_ring.F90"
    src.write_text("""program uses_ring
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hip_flux_ring, mckpp_hip_flux_ring_put, mckpp_hip_flux_ring_records, &
                               mckpp_hip_multi_flux_ring, mckpp_hip_multi_flux_ring_put, mckpp_hip_multi_flux_ring_records
  use mckpp_hip_session, only: mckpp_hip_all_flux_ring, mckpp_hip_all_flux_ring_put, mckpp_hip_all_run_forced
  implicit none
  real(c_double) :: fields(10, 8)
  integer(c_int) :: rc, first, last
  fields = 0
  if (command_argument_count() > 0) then
    call mckpp_hip_all_flux_ring(2)
    call mckpp_hip_all_flux_ring_put(0, fields)
    call mckpp_hip_all_run_forced(1, 2, 2)
    call mckpp_hip_all_flux_ring(0)
    rc = mckpp_hip_flux_ring(c_null_ptr, 2_c_int)
    rc = mckpp_hip_flux_ring_put(c_null_ptr, 0_c_int, fields)
    rc = mckpp_hip_flux_ring_records(c_null_ptr, first, last)
    rc = mckpp_hip_multi_flux_ring(c_null_ptr, 2_c_int)
    rc = mckpp_hip_multi_flux_ring_put(c_null_ptr, 0_c_int, fields)
    rc = mckpp_hip_multi_flux_ring_records(c_null_ptr, first, last)
  end if
end program uses_ring
""")
    exe = tmp_path / "uses_ring"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
