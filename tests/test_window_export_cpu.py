"""CPU side of the packed export of output records (mckpp_hip_window_export): the eight entry points refuse a null
handle with a message that names them, the Python wrappers refuse bad arguments before the library is called, the host
merge of the shards' planes (mckpp_host_export_merge) equals numpy, and the Fortran layer builds with the new bindings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, null_ctx  # noqa: F401

FDIR = os.path.join(cm.ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
NP = {"f8": np.float64, "f4": np.float32}


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    out = np.zeros(4)
    n, rb = C.c_int32(), C.c_int64()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "window_export": lambda f: f(None, 0, api.EXP_F64, 1e20),
            "window_export_layout": lambda f: f(None, 0, C.byref(n), None, None, None, None, C.byref(rb)),
            "window_export_fetch": lambda f: f(None, 0, 0, 2, 0, out.ctypes.data),
            "window_export_fetch_record": lambda f: f(None, 0, 0, out.ctypes.data, out.nbytes),
        }
        for name, call in calls.items():
            entry = pre + name
            assert call(getattr(lib, entry)) < 0, entry
            assert (entry + ": null handle").encode() in lib.mckpp_hip_last_error(), (entry, lib.mckpp_hip_last_error())


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_wrappers_check_their_arguments_first(api, cls):
    h = null_ctx(api, getattr(api, cls))
    out8, out4 = np.zeros((4, 3), order="F"), np.zeros((4, 3), dtype=np.float32, order="F")
    # refused by the wrapper: ValueError, the library is not called
    for bad in ("f2", "float64", np.float32, 8):
        with pytest.raises(ValueError, match="export dtype"):
            h.window_export(0, bad)
    with pytest.raises(ValueError, match="not in output schedule 0"):
        h.window_export_fetch(0, 0, "T", api.OP_LAST, out8)
    h._wsched = {0: {api.OUT["T"]: api.WIN_LAST | api.WIN_MAX}}   # what a successful window_schedule leaves
    with pytest.raises(ValueError, match="has no export"):
        h.window_export_fetch(0, 0, "T", api.OP_LAST, out8)
    with pytest.raises(ValueError, match="has no export"):
        h.window_export_fetch_record(0, 0, np.zeros(16))
    h._wexport = {0: api.EXP_F32}                                  # ... and a successful window_export(0, "f4")
    with pytest.raises(ValueError, match="unknown output field"):
        h.window_export_fetch(0, 0, "nope", api.OP_LAST, out4)
    with pytest.raises(ValueError, match="op 4"):
        h.window_export_fetch(0, 0, "T", 4, out4)
    with pytest.raises(ValueError, match="keeps no op 0"):
        h.window_export_fetch(0, 0, "T", api.OP_MEAN, out4)
    with pytest.raises(ValueError, match="holds float32, not float64"):
        h.window_export_fetch(0, 0, "T", api.OP_LAST, out8)
    with pytest.raises(ValueError, match="holds float32"):
        h.window_export_fetch(0, 0, "T", api.OP_LAST, [0.0] * 12)
    with pytest.raises(ValueError, match="Fortran order"):
        h.window_export_fetch(0, 0, "T", api.OP_LAST, np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="holds float32, not float64"):
        h.window_export_fetch_record(0, 0, np.zeros(16))
    with pytest.raises(ValueError, match="one-dimensional"):
        h.window_export_fetch_record(0, 0, out4)
    # well-formed calls do reach the library (and fail there, for the null handle)
    with pytest.raises(api.MckppHipError, match="window_export_fetch: null handle"):
        h.window_export_fetch(0, 0, "T", api.OP_MAX, out4)
    with pytest.raises(api.MckppHipError, match="window_export_fetch_record: null handle"):
        h.window_export_fetch_record(0, 0, np.zeros(16, dtype=np.float32))
    with pytest.raises(api.MckppHipError, match="window_export_layout: null handle"):
        h.window_export_layout(0)
    with pytest.raises(api.MckppHipError, match="window_export: null handle"):
        h.window_export(0, "f8")
    with pytest.raises(ValueError, match="has no export"):   # (the refused call has dropped what this object knew of)
        h.window_export_fetch(0, 0, "T", api.OP_MAX, out4)
    with pytest.raises(api.MckppHipError, match="window_export: null handle"):
        h.window_export(0, None)


@pytest.mark.parametrize("dtype", ["f8", "f4"])
@pytest.mark.parametrize("nlev", [1, 70])
def test_host_export_merge_equals_numpy(api, dtype, nlev):
    """Shards of 0, 1 and 65 columns dealt over 80 points, 14 of them land."""
    rng = np.random.default_rng(5 + nlev)
    npts, land = 80, -2.5e19
    ocean = rng.permutation(npts)[:66]
    points = [np.sort(ocean[:0]), np.sort(ocean[:1]), np.sort(ocean[1:])]
    assert [len(p) for p in points] == [0, 1, 65]
    planes = [rng.standard_normal((len(p), nlev)).astype(NP[dtype]) for p in points]
    want = np.full((npts, nlev), NP[dtype](land), dtype=NP[dtype], order="F")
    for p, v in zip(points, planes):
        want[p, :] = v
    got = api.host_export_merge(npts, nlev, dtype, land, points, planes)
    assert got.dtype == NP[dtype] and got.flags["F_CONTIGUOUS"]
    assert np.array_equal(got.view(np.uint64 if dtype == "f8" else np.uint32), want.view(np.uint64 if dtype == "f8" else np.uint32))
    # no shard at all: every point is land
    none = api.host_export_merge(npts, nlev, dtype, land, [], [])
    assert np.all(none == NP[dtype](land))


def test_host_export_merge_refuses_bad_arguments(api):
    lib = api._lib()
    out = np.zeros(8)
    pts = np.array([0, 9], dtype=np.int32)
    pl = np.zeros(2)
    ncol = (C.c_int64 * 1)(2)
    pp, pv = (C.c_void_p * 1)(pts.ctypes.data), (C.c_void_p * 1)(pl.ctypes.data)
    assert lib.mckpp_host_export_merge(8, 1, api.EXP_F64, 0.0, 1, ncol, pp, pv, out.ctypes.data) < 0
    assert b"mckpp_host_export_merge: a point outside 0..7" in lib.mckpp_hip_last_error()
    assert np.all(out == 0)
    assert lib.mckpp_host_export_merge(8, 1, 7, 0.0, 1, ncol, pp, pv, out.ctypes.data) < 0
    assert b"mckpp_host_export_merge: dtype 7" in lib.mckpp_hip_last_error()
    assert lib.mckpp_host_export_merge(8, 0, api.EXP_F64, 0.0, 1, ncol, pp, pv, out.ctypes.data) < 0
    assert b"mckpp_host_export_merge: bad argument" in lib.mckpp_hip_last_error()


def test_fortran_layer_builds_with_the_export_bindings(built, tmp_path):
    """A program on the session's new wrappers and the binding's constants compiles and links against the layer."""
    src = tmp_path / "uses_export.F90"
    src.write_text("""program uses_export
  use iso_c_binding
  use mckpp_hip_binding, only: MCKPP_EXP_OFF, MCKPP_EXP_F64, MCKPP_EXP_F32, MCKPP_OP_LAST, MCKPP_OUT_T, MCKPP_OUT_HMIX, &
                               mckpp_hip_multi_window_export, mckpp_hip_multi_window_export_layout, &
                               mckpp_hip_multi_window_export_fetch, mckpp_hip_multi_window_export_fetch_record
  use mckpp_hip_session, only: mckpp_hip_all_window_export, mckpp_hip_all_window_export_fetch, &
                               mckpp_hip_all_window_export_fetch_record
  implicit none
  real(c_double), target :: h8(10), t8(10, 3)
  real(c_float), target :: h4(10), t4(10, 3)
  integer(c_int32_t), target :: nplanes
  integer(c_int64_t), target :: record_bytes
  integer(c_int) :: rc
  if (command_argument_count() > 0) then
    call mckpp_hip_all_window_export(0, MCKPP_EXP_F64, 1e20_c_double)
    call mckpp_hip_all_window_export_fetch(0, 0, MCKPP_OUT_HMIX, MCKPP_OP_LAST, h8)
    call mckpp_hip_all_window_export_fetch(0, 0, MCKPP_OUT_T, MCKPP_OP_LAST, t8)
    call mckpp_hip_all_window_export(0, MCKPP_EXP_F32, 1e20_c_double)
    call mckpp_hip_all_window_export_fetch(0, 0, MCKPP_OUT_HMIX, MCKPP_OP_LAST, h4)
    call mckpp_hip_all_window_export_fetch(0, 0, MCKPP_OUT_T, MCKPP_OP_LAST, t4)
    call mckpp_hip_all_window_export_fetch_record(0, 0, c_loc(t4), int(sizeof(t4), c_int64_t))
    rc = mckpp_hip_multi_window_export_layout(c_null_ptr, 0, c_loc(nplanes), c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                              c_loc(record_bytes))
    call mckpp_hip_all_window_export(0, MCKPP_EXP_OFF, 0._c_double)
  end if
end program uses_export
""")
    exe = tmp_path / "uses_export"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
