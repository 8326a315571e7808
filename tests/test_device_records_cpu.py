"""CPU side of the records of output schedules into device arrays (include/mckpp_hip_device_records.h): the library
exports what the fourth header declares, api._SIGNATURES_RECORDS states those functions type by type (the other three
tables still describe their own headers), the plane struct has the C layout, both entry points refuse a null handle by
their own name, the Python method refuses a malformed call before the library is reached, and the Fortran layer builds
with the new interfaces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, bound_as, null_ctx, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADERS = {n: os.path.join(ROOT, "include", f) for n, f in (("first", "mckpp_hip.h"), ("device", "mckpp_hip_device.h"),
                                                           ("zoom", "mckpp_hip_zoom.h"), ("records", "mckpp_hip_device_records.h"))}
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("records_dev",)
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)


def test_library_exports_every_function_of_the_records_header(api):
    protos = prototypes(HEADERS["records"])
    assert sorted(protos) == NAMES
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_device_records.h but not exported"
    src = open(HEADERS["records"]).read()
    assert '#include "mckpp_hip_device.h"' in src


def test_records_signatures_match_the_records_header(api):
    protos = prototypes(HEADERS["records"])
    table = api._signatures_records()
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
    # every function has its twin, which is the single form after the handle, and is stated once in the table
    src = re.sub(r"/\*.*?\*/", "", open(HEADERS["records"]).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_RECORDS[one][2] and multi not in api._SIGNATURES_RECORDS


def test_the_other_three_tables_still_describe_their_headers(api):
    protos = {n: prototypes(h) for n, h in HEADERS.items()}
    tables = {"first": api._signatures(), "device": api._signatures_device(), "zoom": api._signatures_zoom(),
              "records": api._signatures_records()}
    for n in HEADERS:
        assert sorted(tables[n]) == sorted(protos[n]), n
        for other in HEADERS:
            if other != n:
                assert not set(protos[n]) & set(protos[other]), f"a function declared in both the {n} and the {other} header"
                assert not set(tables[n]) & set(tables[other])


def test_record_plane_struct_layout_matches_the_header(api, tmp_path):
    fields = [f[0] for f in api._DevRecordPlaneC._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADERS["records"]}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_dev_record_plane_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_dev_record_plane_c, {f}));' for f in fields]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._DevRecordPlaneC)
    seen = []
    for line in filter(None, out[1:]):
        name, off = line.split()
        assert getattr(api._DevRecordPlaneC, name).offset == int(off), name
        seen.append(name)
    assert seen == ["sched", "field", "op", "lev0", "nlev", "dtype", "fill_land", "rec", "land_value", "out"]


def test_both_entry_points_refuse_a_null_handle_by_their_own_name(api):
    """the sweep of tests/test_entry_cpu.py over the fourth table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_records().items():
        if res is not C.c_int or not argtypes or argtypes[0] is not api._H:
            continue
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES
    planes = (api._DevRecordPlaneC * 1)()
    for name in NAMES:   # ... and with a table
        assert getattr(lib, name)(None, 1, planes, None) == -1
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_the_library(api, cls):
    """on an object without a device context whatever reaches the library fails there with "null handle": a malformed
    plane must be a ValueError before that, a well-formed call must get there"""
    h = null_ctx(api, getattr(api, cls))
    npts, nzp1 = 12, 41
    h._npts, h._nzp1 = npts, nzp1
    every = api.WIN_MEAN | api.WIN_MIN | api.WIN_MAX | api.WIN_LAST
    unzoomed = api._Kept({api.OUT["T"]: api.WIN_MIN | api.WIN_LAST, api.OUT["hmix"]: every})
    zoomed = api._Kept({api.OUT["T"]: every, api.OUT["hmix"]: api.WIN_MEAN})
    zoomed.zoom = (5, 12)
    h._wsched = {0: unzoomed, 2: zoomed}
    dev = FakeDeviceArray
    out3, out1, z3, z1 = dev((nzp1, npts)), dev((npts,)), dev((12, 5)), dev((1, 5), "<f4")
    bad = {
        "a plane of four": ([(0, 1, "T", 1)], r"planes\[0\] is \(sched, rec, field, op, out\)"),
        "a plane of six": ([(0, 1, "T", 1, out1, 0)], r"planes\[0\] is \(sched, rec, field, op, out\)"),
        "an unknown field": ([(0, 1, "sst", 1, out1, 0, 1)], r"planes\[0\]: unknown output field"),
        "a field that is not in the schedule": ([(0, 1, "S", 1, out1, 0, 1)], r"planes\[0\]: field S is not in output schedule 0"),
        "a schedule that is not set": ([(1, 1, "T", 1, out1, 0, 1)], r"planes\[0\]: field T is not in output schedule 1"),
        "an op the schedule does not keep": ([(0, 1, "T", api.OP_MEAN, out1, 0, 1)], r"planes\[0\]: output schedule 0 keeps no op 0 of field T"),
        "an unknown op": ([(0, 1, "T", 4, out1, 0, 1)], r"planes\[0\]: op 4"),
        "a negative record": ([(0, -1, "T", 1, out1, 0, 1)], r"planes\[0\]: record -1"),
        "a level range outside the axis": ([(0, 1, "T", 1, out3, 1, nzp1)], r"levels 1 \.\. 41 of field T, of which output schedule 0 keeps 41"),
        "a range outside a zoom's levels": ([(2, 1, "T", 1, z3, 0, 13)], r"levels 0 \.\. 12 of field T, of which output schedule 2 keeps 12"),
        "a range of a two-dimensional field": ([(0, 1, "hmix", 0, dev((2, npts)), 0, 2)], "of field hmix, of which output schedule 0 keeps 1"),
        "no level": ([(0, 1, "T", 1, out1, 0, 0)], "keeps 41"),
        "a negative first level": ([(0, 1, "T", 1, out1, -1, 1)], "keeps 41"),
        "more levels than the zoom keeps, from the array": ([(2, 1, "T", 1, dev((13, 5)))], "keeps 12"),
        "a numpy array": ([(0, 1, "T", 1, np.zeros(npts), 0, 1)], "a host array"),
        "an integer array": ([(0, 1, "T", 1, dev((npts,), "<i8"), 0, 1)], "element type <i8"),
        "an array sized to the grid for a zoom": ([(2, 1, "T", 1, dev((12, npts)), 0, 12)], "the call takes 60 elements"),
        "an array that is too small": ([(0, 1, "T", 3, dev((nzp1, npts - 1)), 0, nzp1)], "the call takes 492 elements"),
        "a non-contiguous array": ([(0, 1, "T", 1, dev((2, npts), strides=(8, 16)), 0, 2)], "not C-contiguous"),
        "a second plane that is wrong": ([(0, 1, "T", 1, out1, 0, 1), (0, 1, "T", 1, out1, 41, 1)], r"planes\[1\]"),
        "65 planes": ([(0, 1, "T", 1, out1, 0, 1)] * 65, "65 planes, at most 64"),
    }
    for what, (planes, msg) in bad.items():
        with pytest.raises(ValueError, match=msg):
            h.records_dev(planes)
    with pytest.raises(ValueError, match="stream"):
        h.records_dev([(0, 1, "T", 1, out1, 0, 1)], stream="0")
    good = [[(0, 1, "T", 1, out1, 0, 1)], [(0, 7, "T", api.OP_LAST, out3), (2, 0, api.OUT["hmix"], api.OP_MEAN, z1)],
            [(2, 1, "T", 2, z3), (2, 1, "T", 0, dev((2, 5)), 10, 2)], [(0, 1, "hmix", 3, out1)] * 64]
    for planes in good:
        with pytest.raises(api.MckppHipError, match=r"records_dev: null handle"):
            h.records_dev(planes, fill_land=False)


def test_python_method_builds_the_plane_table(api, monkeypatch):
    calls = []

    class Stub:
        """a library whose entry points all succeed"""

        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 0
            return entry

    monkeypatch.setattr(api, "_lib", lambda: Stub())
    h = api.MckppHip.__new__(api.MckppHip)
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, 12, 41
    kept = api._Kept({api.OUT["T"]: api.WIN_MEAN | api.WIN_LAST, api.OUT["hmix"]: api.WIN_MAX})
    kept.zoom = (5, 12)
    h._wsched = {3: kept}
    a, b = FakeDeviceArray((2, 5), ptr=0x7000000), FakeDeviceArray((5,), "<f4", ptr=0x8000000)
    h.records_dev([(3, 6, "T", api.OP_LAST, a, 10, 2), (3, 2, "hmix", api.OP_MAX, b)], land_value=-2.0)
    h.records_dev([(3, 0, "T", api.OP_MEAN, a)], fill_land=False)
    assert [c[0] for c in calls] == ["mckpp_hip_records_dev"] * 2
    n, tab, stream = calls[0][1][1:]
    got = [tuple(getattr(tab[k], f[0]) for f in api._DevRecordPlaneC._fields_) for k in range(n)]
    assert got == [(3, api.OUT["T"], 3, 10, 2, api.EXP_F64, 1, 6, -2.0, 0x7000000),
                   (3, api.OUT["hmix"], 2, 0, 1, api.EXP_F32, 1, 2, -2.0, 0x8000000)]
    assert stream.value is None
    t = calls[1][1][2][0]
    assert (t.lev0, t.nlev, t.fill_land, t.rec, t.op) == (0, 2, 0, 0, 0)
    assert h._dev_held[-3:] == [a, b, a] and h._held == {}   # kept the way fetch_dev keeps them, not through _hold
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_records_bindings(built, tmp_path):
    """A program that uses the two new interfaces and the plane type compiles and links against the layer."""
    src = tmp_path / "uses_records.F90"
    src.write_text("""program uses_records
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_dev_record_plane_c, MCKPP_OUT_T, MCKPP_EXP_F64, &
    mckpp_hip_records_dev, mckpp_hip_multi_records_dev
  implicit none
  type(mckpp_dev_record_plane_c) :: planes(1)
  integer(c_int) :: rc
  planes(1) = mckpp_dev_record_plane_c(0, MCKPP_OUT_T, 0, 0, 1, MCKPP_EXP_F64, 1, 5_c_int64_t, 1.0e20_c_double, c_null_ptr)
  if (planes(1)%rec /= 5) error stop 1
  if (command_argument_count() > 0) then
    rc = mckpp_hip_records_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_multi_records_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
  end if
end program uses_records
""")
    exe = tmp_path / "uses_records"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
