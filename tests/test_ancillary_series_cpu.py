"""CPU side of the ancillary record series (mckpp_hip_set_ancillary_series, mckpp_hip_ancillary_schedule): the ctypes
mirror of mckpp_anc_epoch_c has the C layout, the new entry points fail with a message where there is no context,
mckpp_host_interp_weights is mckpp_boundary_interpolate's arithmetic (src/mckpp_boundary_interpolate.F90:25-35, :49-50) -
held to a restatement written here, no compiled reference builds that routine - and the Fortran layer builds with the
new interfaces, wrappers and the driver's flag 2048."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api  # noqa: F401

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = os.path.join(cm.ROOT, "include", "mckpp_hip.h")


def test_epoch_struct_and_kinds_match_the_header(api, tmp_path):
    fields = [f[0] for f in api._AncEpochC._fields_]
    kinds = ["SST0", "FCORR_TWOD", "FCORR_WITHZ", "SFCORR_WITHZ", "OCNT_CLIM", "SAL_CLIM", "BOTTOM_TEMP", "COUNT"]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_anc_epoch_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_anc_epoch_c, {f}));' for f in fields]
    body += [f'printf("{k} %d\\n", (int)MCKPP_ANC_{k});' for k in kinds]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._AncEpochC) == 24
    got = dict(line.split() for line in out[1:] if line)
    for f in fields:
        assert int(got[f]) == getattr(api._AncEpochC, f).offset, f
    for k in kinds:
        assert int(got[k]) == getattr(api, "ANC_" + k), k
    assert set(api.ANC_3D) == {api.ANC_FCORR_WITHZ, api.ANC_SFCORR_WITHZ, api.ANC_OCNT_CLIM, api.ANC_SAL_CLIM}


def test_new_entry_points_fail_with_a_message_without_a_context(api):
    lib = api._lib()
    v = (C.c_double * 8)()
    ep = (api._AncEpochC * 2)()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        msg = (pre + "set_ancillary_series: null handle").encode()
        assert getattr(lib, pre + "set_ancillary_series")(None, api.ANC_SST0, 0, 2, v) < 0
        assert msg == lib.mckpp_hip_last_error()
        assert getattr(lib, pre + "set_ancillary_series")(None, api.ANC_SST0, 0, 0, None) < 0
        assert msg == lib.mckpp_hip_last_error()
        msg = (pre + "ancillary_schedule: null handle").encode()
        assert getattr(lib, pre + "ancillary_schedule")(None, api.ANC_OCNT_CLIM, 1, 2, 0, 2, ep) < 0
        assert msg == lib.mckpp_hip_last_error()
        assert getattr(lib, pre + "ancillary_schedule")(None, api.ANC_OCNT_CLIM, 1, 2, 0, 0, None) < 0
        assert msg == lib.mckpp_hip_last_error()
    for cls in (api.MckppHip, api.MckppHipMulti):
        h = cls.__new__(cls)
        h._h = C.c_void_p()
        h._held = {}
        h._npts = 4
        with pytest.raises(api.MckppHipError, match="null"):
            h.set_ancillary_series(api.ANC_SST0, 0, np.zeros((2, 4)))
        with pytest.raises(api.MckppHipError, match="null"):
            h.set_ancillary_series(api.ANC_SST0, 0, None)
        with pytest.raises(api.MckppHipError, match="null"):
            h.ancillary_schedule(api.ANC_OCNT_CLIM, 1, 2, [0, (0, 1, 0.5, 0.5)])
        with pytest.raises(api.MckppHipError, match="null"):
            h.ancillary_schedule(api.ANC_OCNT_CLIM, 1, 2, None)
        with pytest.raises(ValueError, match="set_ancillary_series: kind"):
            h.set_ancillary_series(api.ANC_OCNT_CLIM, 0, np.zeros((2, 4)))   # a 3-D kind takes [nrec, nzp1, npts]
        h._h = C.c_void_p()


def _weights(time, ndtupd, dto, spd, period):
    """src/mckpp_boundary_interpolate.F90:25-35, :49-50 restated: true_time, prev_time, next_time are INTEGER (a REAL
    assigned to one is truncated toward zero: math.trunc), FLOOR is math.floor."""
    true_time = math.trunc(time)                                                              # :25
    ndays = ndtupd * dto / spd                                                                # :26
    prev_time = math.trunc(math.floor((true_time + ndays / 2) / ndays) * ndays - ndays * 0.5)   # :29
    if prev_time < 0:
        prev_weight = (ndays - abs(true_time - prev_time)) / ndays                            # :31
        prev_time = prev_time + period                                                        # :32
    else:
        prev_weight = (ndays - (true_time - prev_time)) / ndays                               # :34
    next_time = math.trunc(prev_time + ndays)                                                 # :49
    return prev_time, next_time, prev_weight, 1 - prev_weight                                 # :50


WEIGHT_CASES = [
    # time, ndtupd, dto, period
    (304.0, 24, 3600.0, 360), (304.7, 24, 3600.0, 360),   # daily records: the integer time makes the weights 0 / 1
    (304.25, 720, 3600.0, 360),                           # monthly records: 11/30 of the previous one
    (5.0, 720, 3600.0, 360),                              # before the first mid-month: the period is added
    (17.3, 36, 1200.0, 360), (0.0, 36, 1200.0, 360), (359.9, 36, 1200.0, 360), (12.5, 2160, 1200.0, 360),
]


def test_interp_weights_are_the_references_arithmetic(api):
    for time, ndtupd, dto, period in WEIGHT_CASES:
        got = api.interp_weights(time, ndtupd, dto, 86400.0, period)
        assert got == _weights(time, ndtupd, dto, 86400.0, period), (time, ndtupd, dto, got)
        assert api.MckppHip.interp_weights(time, ndtupd, dto, 86400.0, period) == got
    assert api.interp_weights(304.0, 24, 3600.0)[2:] == (0.0, 1.0) == api.interp_weights(304.7, 24, 3600.0)[2:]
    assert api.interp_weights(304.7, 24, 3600.0)[:2] == (303, 304)
    assert api.interp_weights(304.25, 720, 3600.0)[:3] == (285, 315, 11.0 / 30.0)
    pt, nx, wp, wn = api.interp_weights(5.0, 720, 3600.0, period=360)
    assert (pt, nx, wp, wn) == (345, 375, (30.0 - 20.0) / 30.0, 1 - (30.0 - 20.0) / 30.0) and wp == 1.0 / 3.0
    # dto = 1200, ndtupd = 36: records half a day apart - every quantity of :29 is truncated
    assert api.interp_weights(17.3, 36, 1200.0, period=360) == _weights(17.3, 36, 1200.0, 86400.0, 360) == (16, 16, -1.0, 2.0)


def test_fortran_layer_builds_with_the_ancillary_bindings(built, tmp_path):
    src = tmp_path / "uses_ancillary_series.F90"
    src.write_text("""program uses_ancillary_series
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hip_set_ancillary_series, mckpp_hip_multi_set_ancillary_series, &
                               mckpp_hip_ancillary_schedule, mckpp_hip_multi_ancillary_schedule, mckpp_anc_epoch_c, &
                               mckpp_host_interp_weights, MCKPP_ANC_SST0, MCKPP_ANC_OCNT_CLIM, MCKPP_ANC_BOTTOM_TEMP, MCKPP_ANC_COUNT
  use mckpp_hip_session, only: mckpp_hip_all_set_ancillary_series, mckpp_hip_all_ancillary_schedule
  implicit none
  real(c_double) :: recs(4, 2), wp, wn
  type(mckpp_anc_epoch_c) :: ep(2)
  integer(c_int) :: rc
  integer(c_int32_t) :: pt, nx
  recs = 1
  ep(1) = mckpp_anc_epoch_c(0, -1, 0._c_double, 0._c_double)
  ep(2) = mckpp_anc_epoch_c(0, 1, 0.5_c_double, 0.5_c_double)
  call mckpp_host_interp_weights(5._c_double, 720, 3600._c_double, 86400._c_double, 360, pt, nx, wp, wn)
  if (pt /= 345 .or. nx /= 375 .or. wp /= 1._c_double / 3._c_double .or. MCKPP_ANC_COUNT /= 7) error stop 3
  if (command_argument_count() > 0) then
    call mckpp_hip_all_set_ancillary_series(MCKPP_ANC_SST0, 0, 2, recs)
    call mckpp_hip_all_ancillary_schedule(MCKPP_ANC_SST0, 1, 3, 0, 1, ep)
    call mckpp_hip_all_ancillary_schedule(MCKPP_ANC_SST0, 1, 3, 0, 0)
    call mckpp_hip_all_set_ancillary_series(MCKPP_ANC_SST0, 0, 0)
    rc = mckpp_hip_set_ancillary_series(c_null_ptr, MCKPP_ANC_BOTTOM_TEMP, 0, 2, recs)
    rc = mckpp_hip_multi_set_ancillary_series(c_null_ptr, MCKPP_ANC_BOTTOM_TEMP, 0, 0)
    rc = mckpp_hip_ancillary_schedule(c_null_ptr, MCKPP_ANC_OCNT_CLIM, 1, 2, 0, 2, ep)
    rc = mckpp_hip_multi_ancillary_schedule(c_null_ptr, MCKPP_ANC_OCNT_CLIM, 1, 2, 0, 0)
  end if
end program uses_ancillary_series
""")
    exe = tmp_path / "uses_ancillary_series"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-Wl,-rpath," + os.path.join(cm.ROOT, "mckpp_f90_amd"),
                        "-o", str(exe)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    r = subprocess.run([str(exe)], capture_output=True, text=True)   # (no argument: the host helper only, no device)
    assert r.returncode == 0, r.stderr + r.stdout
    drv = open(os.path.join(FDIR, "kpp_driver.F90")).read()
    assert "iand(flags, 2048)" in drv and "mckpp_hip_all_ancillary_schedule(MCKPP_ANC_OCNT_CLIM" in drv
