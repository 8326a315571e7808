"""CPU side of the restart snapshots taken inside the step launches (mckpp_hip_restart_schedule): the eight new entry
points refuse a null handle with a message that names them, the Python wrappers refuse a negative period, no slots and
an origin before step 1 before the library is called, and the Fortran layer builds with the new bindings."""
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
    a, b = C.c_int64(), C.c_int64()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "restart_schedule": lambda n: getattr(lib, n)(None, 1, 12, 2),
            "restart_snapshots": lambda n: getattr(lib, n)(None, C.byref(a), C.byref(b)),
            "restart_snapshot_save": lambda n: getattr(lib, n)(None, 0, b"/nonexistent/snapshot"),
            "restart_snapshot_release": lambda n: getattr(lib, n)(None, 0),
        }
        for name, call in calls.items():
            entry = pre + name
            assert call(entry) < 0, entry
            assert entry.encode() in lib.mckpp_hip_last_error(), (entry, lib.mckpp_hip_last_error())


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_wrappers_check_the_schedule_first(api, cls):
    h = null_ctx(api, getattr(api, cls))
    # refused by the wrapper: ValueError, the library is not called
    with pytest.raises(ValueError, match="period=-1"):
        h.restart_schedule(1, -1, 2)
    with pytest.raises(ValueError, match="nslots=0"):
        h.restart_schedule(1, 12, 0)
    with pytest.raises(ValueError, match="nt_origin=0"):
        h.restart_schedule(0, 12, 2)
    assert h.restart_scheduled is None
    # well-formed calls do reach the library (and fail there, for the null handle)
    pre = "multi_" if cls == "MckppHipMulti" else ""
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}restart_schedule: null handle"):
        h.restart_schedule(1, 12, 2)
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}restart_schedule: null handle"):
        h.restart_schedule(1, 0, 0)   # (a cancel)
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}restart_snapshots: null handle"):
        h.restart_snapshots()
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}restart_snapshot_save: null handle"):
        h.restart_snapshot_save(0, "/nonexistent/snapshot")
    with pytest.raises(api.MckppHipError, match=f"mckpp_hip_{pre}restart_snapshot_release: null handle"):
        h.restart_snapshot_release(0)
    assert h.restart_scheduled is None


def test_fortran_layer_builds_with_the_restart_bindings(built, tmp_path):
    """A program on the session's new wrappers and the binding's interfaces compiles and links against the layer."""
    src = tmp_path / "uses_restarts.F90"
    src.write_text("""program uses_restarts
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hip_restart_schedule, mckpp_hip_restart_snapshots, mckpp_hip_restart_snapshot_save, &
                               mckpp_hip_restart_snapshot_release, mckpp_hip_multi_restart_schedule, &
                               mckpp_hip_multi_restart_snapshots, mckpp_hip_multi_restart_snapshot_save, &
                               mckpp_hip_multi_restart_snapshot_release
  use mckpp_hip_session, only: mckpp_hip_all_restart_schedule, mckpp_hip_all_restart_snapshots, &
                               mckpp_hip_all_restart_snapshot_save, mckpp_hip_all_restart_snapshot_release
  implicit none
  integer :: first_kept, last_complete, s
  integer(c_int64_t) :: a, b
  integer(c_int) :: rc
  if (command_argument_count() > 0) then
    call mckpp_hip_all_restart_schedule(1, 12, 2)
    call mckpp_hip_all_restart_snapshots(first_kept, last_complete)
    do s = first_kept, last_complete
      call mckpp_hip_all_restart_snapshot_save(s, 'restart')
    end do
    call mckpp_hip_all_restart_snapshot_release(last_complete)
    rc = mckpp_hip_restart_schedule(c_null_ptr, 1_c_int, 12_c_int, 2_c_int)
    rc = mckpp_hip_restart_snapshots(c_null_ptr, a, b)
    rc = mckpp_hip_restart_snapshot_save(c_null_ptr, 0_c_int64_t, 'restart'//c_null_char)
    rc = mckpp_hip_restart_snapshot_release(c_null_ptr, 0_c_int64_t)
  end if
end program uses_restarts
""")
    exe = tmp_path / "uses_restarts"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
