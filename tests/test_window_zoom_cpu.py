"""CPU side of the zoomed output schedules (include/mckpp_hip_zoom.h): the library exports what the companion header
declares, api._SIGNATURES_ZOOM states those functions type by type (the first two tables still describe their own
headers), the zoom struct has the C layout, every new handle-taking entry refuses a null handle by its own name, the
Python wrappers refuse a malformed zoom before the library is reached, mckpp_host_zoom_box is the numpy box, and the
Fortran layer builds with the new interfaces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, bound_as, null_ctx, prototypes  # noqa: F401

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip.h")
DEVICE_HEADER = os.path.join(ROOT, "include", "mckpp_hip_device.h")
ZOOM_HEADER = os.path.join(ROOT, "include", "mckpp_hip_zoom.h")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("window_schedule_zoom", "window_zoom")
HOST = ("mckpp_host_zoom_box",)


def test_library_exports_every_function_of_the_zoom_header(api):
    protos = prototypes(ZOOM_HEADER)
    assert sorted(protos) == sorted([pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED] + list(HOST))
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_zoom.h but not exported"


def test_zoom_signatures_match_the_zoom_header(api):
    protos = prototypes(ZOOM_HEADER)
    table = api._signatures_zoom()
    assert sorted(table) == sorted(protos)
    lib = api._lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), f"{name} takes {len(params)} parameters, {len(argtypes)} bound"
        for i, (p, t) in enumerate(zip(params, argtypes)):
            assert bound_as(p, t), f"{name}: parameter {i} is {p}, bound as {t}"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), f"{name}: _bind left another signature"
    # every handle function has its twin, which is the single form after the handle, and is stated once in the table
    src = re.sub(r"/\*.*?\*/", "", open(ZOOM_HEADER).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_ZOOM[one][2] and multi not in api._SIGNATURES_ZOOM
    for n in HOST:
        assert not api._SIGNATURES_ZOOM[n][2]


def test_the_first_two_tables_still_describe_their_headers(api):
    first, device, zoom = prototypes(HEADER), prototypes(DEVICE_HEADER), prototypes(ZOOM_HEADER)
    assert sorted(api._signatures()) == sorted(first)
    assert sorted(api._signatures_device()) == sorted(device)
    assert not set(zoom) & (set(first) | set(device)), "a zoom function declared in another header"
    assert not set(api._signatures_zoom()) & (set(api._signatures()) | set(api._signatures_device()))


def test_zoom_struct_layout_matches_the_header(api, tmp_path):
    fields = [f[0] for f in api._WinZoomC._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{ZOOM_HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_win_zoom_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_win_zoom_c, {f}));' for f in fields]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._WinZoomC)
    seen = []
    for line in filter(None, out[1:]):
        name, off = line.split()
        assert getattr(api._WinZoomC, name).offset == int(off), name
        seen.append(name)
    assert seen == ["points", "npoints", "lev0", "nlev"]


def test_every_zoom_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over the third table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_zoom().items():
        if res is not C.c_int or not argtypes or argtypes[0] is not api._H:
            continue
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_wrappers_refuse_a_bad_zoom_before_the_library(api, cls):
    """on an object without a device context whatever reaches the library fails there with "null handle": a bad zoom
    must be a ValueError before that, a well-formed call must get there"""
    h = null_ctx(api, getattr(api, cls))
    h._npts, h._nzp1 = 50, 41
    sched = (1, 1, 2, 4, ("T", "hmix"), api.WIN_MEAN)
    bad = {
        "twice, at positions 1 and 3": dict(points=[4, 7, 9, 7]),
        "point 50 at position 2 is outside 0..49": dict(points=[4, 7, 50]),
        "point -1 at position 0": dict(points=[-1, 7]),
        "an empty point list": dict(points=[]),
        "integer point numbers": dict(points=[1.5, 2.0]),
        "levels (lev0=30, nlev=12)": dict(levels=(30, 12)),
        "levels (lev0=3, nlev=-1)": dict(levels=(3, -1)),
        "levels (lev0=-1, nlev=2)": dict(levels=(-1, 2)),
        "levels (lev0=4, nlev=0)": dict(levels=(4, 0)),
    }
    for text, kw in bad.items():
        with pytest.raises(ValueError, match=re.escape(text)):
            h.window_schedule_zoom(*sched, **kw)
    with pytest.raises(ValueError, match="unknown output field"):   # (the checks of window_schedule come first)
        h.window_schedule_zoom(1, 1, 2, 4, ("nothing",), api.WIN_MEAN, points=[1])
    for kw in (dict(), dict(points=[49, 0, 7]), dict(points=np.arange(50)[::-1], levels=(29, 12)), dict(levels=(0, 0)),
               dict(levels=(40, 1))):
        with pytest.raises(api.MckppHipError, match=r"window_schedule_zoom: null handle"):
            h.window_schedule_zoom(*sched, **kw)
    assert 1 not in h._scheds()   # (a refused schedule is not recorded)
    with pytest.raises(api.MckppHipError, match=r"window_zoom: null handle"):
        h.window_zoom(1)
    # what a successful window_schedule_zoom leaves: the fetches check the array against the zoom's shape
    kept = api._Kept({api.OUT["T"]: api.WIN_MEAN, api.OUT["hmix"]: api.WIN_MEAN})
    kept.zoom = (3, 12)
    h._wsched = {1: kept}
    h._wexport = {1: api.EXP_F64}
    for fetch in (h.window_record_fetch, h.window_export_fetch):
        with pytest.raises(ValueError, match=re.escape("a plane of T is out(3, 12), 36 values, not 2050")):
            fetch(1, 0, "T", api.OP_MEAN, np.zeros((50, 41), order="F"))
        with pytest.raises(ValueError, match=re.escape("a plane of hmix is out(3), 3 values, not 50")):
            fetch(1, 0, "hmix", api.OP_MEAN, np.zeros(50))
        with pytest.raises(api.MckppHipError, match="null handle"):
            fetch(1, 0, "T", api.OP_MEAN, np.zeros((3, 12), order="F"))
        with pytest.raises(api.MckppHipError, match="null handle"):
            fetch(1, 0, "hmix", api.OP_MEAN, np.zeros(3))


def test_zoom_box_is_the_numpy_box(api):
    nx, ny = 7, 5
    grid = np.arange(nx * ny).reshape((ny, nx))   # point number j * nx + i
    boxes = [(0, nx, 0, ny), (0, 1, 0, 1), (nx - 1, 1, ny - 1, 1), (0, 3, 1, 2), (4, 3, 0, 5), (2, 2, 3, 2), (0, nx, 4, 1),
             (6, 1, 0, ny)]
    for ib, ni, jb, nj in boxes:
        got = api.zoom_box(nx, ny, ib, ni, jb, nj)
        assert got.dtype == np.int32 and np.array_equal(got, grid[jb:jb + nj, ib:ib + ni].ravel()), (ib, ni, jb, nj)
    for ib, ni, jb, nj in [(5, 3, 0, 1), (0, 1, 4, 2), (-1, 2, 0, 1), (0, 1, -1, 1), (0, 0, 0, 1), (0, 1, 0, 0), (7, 1, 0, 1)]:
        with pytest.raises(api.MckppHipError, match=r"^mckpp_host_zoom_box: box .* is not within the grid of 7 x 5 points"):
            api.zoom_box(nx, ny, ib, ni, jb, nj)
    with pytest.raises(api.MckppHipError, match=r"^mckpp_host_zoom_box: grid 0 x 5"):
        api.zoom_box(0, 5, 0, 1, 0, 1)
    lib = api._lib()
    assert lib.mckpp_host_zoom_box(7, 5, 0, 1, 0, 1, None) < 0
    assert lib.mckpp_hip_last_error() == b"mckpp_host_zoom_box: null argument"


def test_fortran_layer_builds_with_the_zoom_bindings(built, tmp_path):
    """A program on the session's new wrappers and the binding's new interfaces compiles and links against the layer."""
    src = tmp_path / "uses_zoom.F90"
    src.write_text("""program uses_zoom
  use iso_c_binding
  use mckpp_hip_binding, only: MCKPP_WIN_MEAN, MCKPP_WIN_LAST, MCKPP_OUT_T, MCKPP_OUT_HMIX, mckpp_win_zoom_c, &
                               mckpp_hip_multi_window_schedule_zoom, mckpp_hip_multi_window_zoom, mckpp_host_zoom_box
  use mckpp_hip_session, only: mckpp_hip_all_window_schedule_zoom, mckpp_hip_all_window_zoom
  implicit none
  integer(c_int32_t) :: box(6)
  integer(c_int64_t) :: npoints, ring_bytes
  integer :: lev0, nlev
  type(mckpp_win_zoom_c) :: z
  z = mckpp_win_zoom_c(c_null_ptr, 0_c_int64_t, 0_c_int32_t, 1_c_int32_t)
  if (mckpp_host_zoom_box(5_c_int64_t, 4_c_int64_t, 1_c_int64_t, 3_c_int64_t, 2_c_int64_t, 2_c_int64_t, box) /= 0) error stop 1
  if (any(box /= [11, 12, 13, 16, 17, 18])) error stop 2
  if (command_argument_count() > 0) then
    call mckpp_hip_all_window_schedule_zoom(0, 1, 3, 8, [int(MCKPP_OUT_T, c_int32_t), int(MCKPP_OUT_HMIX, c_int32_t)], &
                                            [MCKPP_WIN_MEAN, MCKPP_WIN_LAST], points=box, lev0=0, nlev=1)
    call mckpp_hip_all_window_schedule_zoom(1, 1, 3, 8, [int(MCKPP_OUT_T, c_int32_t)], [MCKPP_WIN_LAST], nlev=z%nlev)
    call mckpp_hip_all_window_zoom(0, npoints, lev0, nlev, ring_bytes)
  end if
end program uses_zoom
""")
    exe = tmp_path / "uses_zoom"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(cm.ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    r = subprocess.run([str(exe)], capture_output=True, text=True)   # (no argument: the host box alone runs)
    assert r.returncode == 0, r.stderr + r.stdout
