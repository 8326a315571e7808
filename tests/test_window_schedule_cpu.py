"""CPU side of the output windows accumulated inside the step launches (mckpp_hip_window_schedule): the new entry
points refuse a null handle with a message that names them, the Python wrappers refuse an unknown field, an empty
operations mask and an op the schedule does not keep before the library is called, and the Fortran layer builds with
the new bindings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, null_ctx  # noqa: F401

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    f = np.array([2], dtype=np.int32)
    o = np.array([1], dtype=np.uint32)
    out = np.zeros(4)
    a, b = C.c_int64(), C.c_int64()
    fp, op = f.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_uint32))
    outp = out.ctypes.data_as(C.POINTER(C.c_double))
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "window_schedule": lambda n: getattr(lib, n)(None, 0, 1, 2, 2, fp, op, 1),
            "window_record_fetch": lambda n: getattr(lib, n)(None, 0, 0, 2, 0, outp),
            "window_record_release": lambda n: getattr(lib, n)(None, 0, 0),
            "window_records": lambda n: getattr(lib, n)(None, 0, C.byref(a), C.byref(b)),
        }
        for name, call in calls.items():
            entry = pre + name
            assert call(entry) < 0, entry
            assert entry.encode() in lib.mckpp_hip_last_error(), (entry, lib.mckpp_hip_last_error())


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_wrappers_check_fields_and_ops_first(api, cls):
    h = null_ctx(api, getattr(api, cls))
    out = np.zeros(4, order="F")
    # refused by the wrapper: ValueError, the library is not called
    with pytest.raises(ValueError, match="unknown output field"):
        h.window_schedule(0, 1, 2, 2, ["T", "no_such_field"], api.WIN_MEAN)
    with pytest.raises(ValueError, match="unknown output field"):
        h.window_schedule(0, 1, 2, 2, [len(api.OUT_FIELDS)], api.WIN_MEAN)
    with pytest.raises(ValueError, match="operations 0x0"):
        h.window_schedule(0, 1, 2, 2, ["T", "S"], [api.WIN_MEAN, 0])
    with pytest.raises(ValueError, match="operations 0x10"):
        h.window_schedule(0, 1, 2, 2, ["T"], 16)
    with pytest.raises(ValueError, match="not in output schedule 0"):
        h.window_record_fetch(0, 0, "T", api.OP_LAST, out)
    h._wsched = {0: {api.OUT["T"]: api.WIN_LAST | api.WIN_MAX}}   # what a successful window_schedule leaves
    with pytest.raises(ValueError, match="keeps no op 0"):
        h.window_record_fetch(0, 0, "T", api.OP_MEAN, out)
    with pytest.raises(ValueError, match="op 4"):
        h.window_record_fetch(0, 0, "T", 4, out)
    with pytest.raises(ValueError, match="unknown output field"):
        h.window_record_fetch(0, 0, "nope", api.OP_LAST, out)
    # well-formed calls do reach the library (and fail there, for the null handle)
    with pytest.raises(api.MckppHipError, match="window_record_fetch: null handle"):
        h.window_record_fetch(0, 0, "T", api.OP_MAX, out)
    with pytest.raises(api.MckppHipError, match="window_record_release: null handle"):
        h.window_record_release(0, 0)
    with pytest.raises(api.MckppHipError, match="window_records: null handle"):
        h.window_records(0)
    with pytest.raises(api.MckppHipError, match="window_schedule: null handle"):
        h.window_schedule(0, 1, 2, 2, ["T", "hmix"], api.WIN_LAST)
    with pytest.raises(ValueError, match="not in output schedule 0"):   # (the library has no schedule 0 either)
        h.window_record_fetch(0, 0, "T", api.OP_MAX, out)


def test_fortran_layer_builds_with_the_schedule_bindings(built, tmp_path):
    """A program on the session's new wrappers and the binding's constants compiles and links against the layer."""
    src = tmp_path / "uses_schedules.F90"
    src.write_text("""program uses_schedules
  use iso_c_binding
  use mckpp_hip_binding, only: MCKPP_WIN_MEAN, MCKPP_WIN_MIN, MCKPP_WIN_MAX, MCKPP_WIN_LAST, MCKPP_OP_LAST, &
                               MCKPP_OUT_T, MCKPP_OUT_HMIX, mckpp_hip_multi_window_schedule, &
                               mckpp_hip_multi_window_record_fetch, mckpp_hip_multi_window_record_release
  use mckpp_hip_session, only: mckpp_hip_all_window_schedule, mckpp_hip_all_window_record_fetch, &
                               mckpp_hip_all_window_record_release
  implicit none
  real(c_double) :: out(10)
  if (command_argument_count() > 0) then
    call mckpp_hip_all_window_schedule(0, 1, 3, 8, [int(MCKPP_OUT_T, c_int32_t), int(MCKPP_OUT_HMIX, c_int32_t)], &
                                       [ior(MCKPP_WIN_MEAN, ior(MCKPP_WIN_MIN, MCKPP_WIN_MAX)), MCKPP_WIN_LAST])
    call mckpp_hip_all_window_record_fetch(0, 0, MCKPP_OUT_HMIX, MCKPP_OP_LAST, out)
    call mckpp_hip_all_window_record_release(0, 0)
  end if
end program uses_schedules
""")
    exe = tmp_path / "uses_schedules"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
