"""CPU side of the step log (mckpp_hip_step_log): the eight new entry points refuse a null handle with a message that
names them, the Python wrappers refuse negative arguments before the library is called, and the Fortran layer builds
with the new bindings and mckpp_hip_all_step_log."""
import ctypes as C
import os
import subprocess

import pytest

import common as cm
from harness import api, null_ctx  # noqa: F401

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
    v = (C.c_int32 * 4)()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "step_log": lambda n: getattr(lib, n)(None, 16, 0),
            "step_log_count": lambda n: getattr(lib, n)(None, C.byref(a), C.byref(b), C.byref(c)),
            "step_log_fetch": lambda n: getattr(lib, n)(None, 4, v, v, v, v),
            "step_log_clear": lambda n: getattr(lib, n)(None),
        }
        for name, call in calls.items():
            entry = pre + name
            assert call(entry) < 0, entry
            assert (entry + ": null handle").encode() in lib.mckpp_hip_last_error(), (entry, lib.mckpp_hip_last_error())


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_wrappers_check_the_arguments_first(api, cls):
    h = null_ctx(api, getattr(api, cls))
    # refused by the wrapper: ValueError, the library is not called
    with pytest.raises(ValueError, match="capacity=-1"):
        h.step_log(-1)
    with pytest.raises(ValueError, match="min_passes=-13"):
        h.step_log(16, -13)
    assert h.step_logged is None
    # well-formed calls do reach the library (and fail there, for the null handle)
    pre = "multi_" if cls == "MckppHipMulti" else ""
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}step_log: null handle"):
        h.step_log(16, 13)
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}step_log: null handle"):
        h.step_log(0)   # (a cancel)
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}step_log_count: null handle"):
        h.step_log_count()
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}step_log_count: null handle"):
        h.step_log_fetch()   # (asks for the number of stored records first)
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}step_log_clear: null handle"):
        h.step_log_clear()
    assert h.step_logged is None


def test_fortran_layer_builds_with_the_step_log_bindings(built, tmp_path):
    """A program on the session's new wrapper and the binding's interfaces compiles and links against the layer."""
    src = tmp_path / "uses_step_log.F90"
    src.write_text("""program uses_step_log
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hip_step_log, mckpp_hip_step_log_count, mckpp_hip_step_log_fetch, &
                               mckpp_hip_step_log_clear, mckpp_hip_multi_step_log, mckpp_hip_multi_step_log_count, &
                               mckpp_hip_multi_step_log_fetch, mckpp_hip_multi_step_log_clear
  use mckpp_hip_session, only: mckpp_hip_all_step_log, mckpp_hip_all_run_forced
  implicit none
  integer(c_int64_t) :: n_events, n_stored
  integer(c_int32_t) :: status_or, nt(4), pt(4), st(4), np(4)
  integer(c_int) :: rc
  if (command_argument_count() > 0) then
    call mckpp_hip_all_step_log(1000, 13)
    call mckpp_hip_all_run_forced(1, 10, 1)
    call mckpp_hip_all_step_log(0, 0)
    rc = mckpp_hip_step_log(c_null_ptr, 16_c_int64_t, 0_c_int)
    rc = mckpp_hip_step_log_count(c_null_ptr, n_events, n_stored, status_or)
    rc = mckpp_hip_step_log_fetch(c_null_ptr, 4_c_int64_t, nt, pt, st, np)
    rc = mckpp_hip_step_log_clear(c_null_ptr)
    rc = mckpp_hip_multi_step_log(c_null_ptr, 16_c_int64_t, 0_c_int)
    rc = mckpp_hip_multi_step_log_count(c_null_ptr, n_events, n_stored, status_or)
    rc = mckpp_hip_multi_step_log_fetch(c_null_ptr, 4_c_int64_t, nt, pt, st, np)
    rc = mckpp_hip_multi_step_log_clear(c_null_ptr)
  end if
end program uses_step_log
""")
    exe = tmp_path / "uses_step_log"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
