"""CPU side of the resident bottom temperature (mckpp_hip_set_bottomtemp).

What the GPU tests take as expected - the oracle stepped with orc.bottomtemp after every step - is held here to the
compiled reference's own driver with L_VARY_BOTTOM_TEMP (where oracle/_ref was built), on a longer and less regular case
than the recorded one: many steps, a stretched grid, land, a correction switch that writes the same rows.  And the
bindings: the ctypes signatures of the two new entry points match the header, they refuse a null handle, and the Fortran
layer builds with the new interfaces and mckpp_hip_all_set_bottomtemp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
import ref_step_cases as rc
from harness import api  # noqa: F401
from oracle import orc

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = os.path.join(cm.ROOT, "include", "mckpp_hip.h")

CASE = rc.Case(40, 69, 8, grid="stretched", land_every=5, switches=dict(L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1),
               pre=rc._fcorr_withz, bottom_temp=True)


@pytest.mark.parametrize("build,exp_mode", [("libm", 0), ("pexp", 1)])
def test_oracle_with_the_override_after_every_step_is_the_reference_driver(built, build, exp_mode):
    if not orc.have_ref_step():
        pytest.skip("the compiled reference step (oracle/_ref/libmckpp_ref_step*.so) is not built here")
    oc, ob, _, _ = rc.oracle_start(CASE, exp_mode=exp_mode)
    live = rc.run_reference(CASE, oc, ob, exp_mode)
    act = rc.active_columns(CASE)
    bt = rc.bottom_temp(CASE, ob)
    for nt in rc.run_oracle(CASE, oc, ob):
        r = live[nt - 1]
        for name in rc.STEP_FIELDS:
            a = rc.canonical(rc.field_of(ob, name, CASE.nz))[act]
            b = rc.canonical(rc.field_of(r, name, CASE.nz))[act]
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"{build} exp, step {nt}: {name}"
        assert np.array_equal(ob["T"][act, CASE.nz + 1], bt[act])
        # reach: the override's increment is not zero in the step that first meets the field (nothing else moves the
        # bottom level, so a constant field leaves tinc_fcorr(nzp1) = ocnTcorr(nzp1) = 0 from the second step on) ...
        assert np.all((ob["ocnTcorr"][act, CASE.nz + 1] != 0) == (nt == 1))
    # ... and the correction switch wrote the levels above
    assert np.any(ob["tinc_fcorr"][act, 1:CASE.nz] != 0)


def test_ctypes_signatures_match_the_header(api):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = api._lib()
    for name, handle in (("mckpp_hip_set_bottomtemp", "mckpp_hip_handle"), ("mckpp_hip_multi_set_bottomtemp", "mckpp_hip_multi_handle")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/mckpp_hip.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == [f"{handle} {'h' if handle == 'mckpp_hip_handle' else 'm'}", "const double *bottom_temp"], args
        f = getattr(lib, name)
        assert f.argtypes == [C.c_void_p, C.POINTER(C.c_double)] and f.restype is C.c_int
        # the host-applied form has the same signature
        assert getattr(lib, name.replace("set_", "")).argtypes == f.argtypes
    for cls in (api.MckppHip, api.MckppHipMulti):
        assert callable(getattr(cls, "set_bottomtemp"))


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    v = (C.c_double * 4)()
    assert lib.mckpp_hip_set_bottomtemp(None, v) < 0
    assert b"mckpp_hip_set_bottomtemp: null handle" in lib.mckpp_hip_last_error()
    assert lib.mckpp_hip_set_bottomtemp(None, None) < 0   # (a cancel)
    assert b"mckpp_hip_set_bottomtemp: null handle" in lib.mckpp_hip_last_error()
    assert lib.mckpp_hip_multi_set_bottomtemp(None, v) < 0
    assert b"mckpp_hip_multi_set_bottomtemp: null handle" == lib.mckpp_hip_last_error()
    for cls in (api.MckppHip, api.MckppHipMulti):
        h = cls.__new__(cls)
        h._h = C.c_void_p()
        with pytest.raises(api.MckppHipError, match="null"):
            h.set_bottomtemp(None)


def test_fortran_layer_builds_with_the_bottomtemp_bindings(built, tmp_path):
    """A program on the session's new wrapper and the binding's interfaces compiles and links against the layer; the
    driver module takes the session's word for whether a field is resident."""
    src = tmp_path / "uses_set_bottomtemp.F90"
    src.write_text("""program uses_set_bottomtemp
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hip_set_bottomtemp, mckpp_hip_multi_set_bottomtemp
  use mckpp_hip_session, only: mckpp_hip_all_set_bottomtemp, mckpp_hip_bottomtemp_resident, mckpp_hip_all_run_forced
  use mckpp_physics_driver_mod, only: mckpp_physics_driver
  implicit none
  real(c_double) :: bt(4)
  integer(c_int) :: rc
  bt = 1
  if (command_argument_count() > 0) then
    call mckpp_hip_all_set_bottomtemp(bt)
    if (mckpp_hip_bottomtemp_resident()) call mckpp_physics_driver()
    call mckpp_hip_all_run_forced(1, 10, 1)
    call mckpp_hip_all_set_bottomtemp()
    rc = mckpp_hip_set_bottomtemp(c_null_ptr, bt)
    rc = mckpp_hip_set_bottomtemp(c_null_ptr)
    rc = mckpp_hip_multi_set_bottomtemp(c_null_ptr, bt)
    rc = mckpp_hip_multi_set_bottomtemp(c_null_ptr)
  end if
end program uses_set_bottomtemp
""")
    exe = tmp_path / "uses_set_bottomtemp"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    drv = open(os.path.join(FDIR, "mckpp_physics_driver_mod.F90")).read()
    assert re.search(r"L_VARY_BOTTOM_TEMP\s*\.and\.\s*\.not\.\s*mckpp_hip_bottomtemp_resident\(\)", drv)
