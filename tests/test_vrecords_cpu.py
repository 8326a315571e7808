"""CPU side of completed records on a caller axis (include/mckpp_hip_vrecords.h): the header declares exactly the six
functions and the host rule and the library exports them, api._SIGNATURES_VRECORDS states them type by type and is
disjoint from the other ten tables, the two structs have the C layout, both handles have the methods, every entry point
refuses a null handle by its own name, the plane builders of the Python layer put a tuple into the table in the order
the header has and refuse a malformed call before the library is reached, the Fortran layer builds with the new types
and interfaces - and the level rule, the one piece of the feature that needs no GPU, is what a numpy statement from
tests/vaxis_ref.py's levels_read gives, from the library and from a stand-alone program built under the address and
undefined-behaviour sanitizers, on the model axes and the caller axes of tests/test_vrecords_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import common as cm
import hgrid_ref as hr
import ref_loop_cases as lc
import vaxis_ref as vr
from harness import api, bound_as, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray
from test_hv_cpu import _Stub

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip_vrecords.h")
CSRC = os.path.join(ROOT, "mckpp_f90_amd", "csrc")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("vrecords_vaxis_dev", "vrecords_vaxis_host", "vrecords_hv_dev")
HOST_NAMES = ["mckpp_host_vrecords_rule"]
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
STRUCTS = {
    "mckpp_vaxis_record_plane_c": ("_VaxisRecordPlaneC", ["sched", "field", "op", "axis", "dtype", "fill_land", "rec", "land_value",
                                                          "out"]),
    "mckpp_hv_record_plane_c": ("_HvRecordPlaneC", ["sched", "field", "op", "axis", "dtype", "grid", "norm", "fill_land", "rec",
                                                    "land_value", "out"]),
}
CASES = ("every_step_nz40", "sweep_nd3", "deep_nz100_nd4")
KEPT = (2, 7)     # (lev0, nlev) of the listed schedule of tests/test_remap_gpu.py's Recorded: model levels 2 .. 8


# ---------------------------------------------------------------------------
# the axes of tests/test_vrecords_gpu.py, and the rule in numpy
# ---------------------------------------------------------------------------
def model_levels(tag):
    """zm(1:nzp1) of a case"""
    case = lc.CASES[tag]
    return np.array(lc.hip_raw(case)[0].zm[:case.nz + 1], dtype=np.float64)


def caller_axes(zm, kept=KEPT):
    """tests/vaxis_ref.py's axes and four more:
      tiles100   100 levels strictly inside the column: two 64-level tiles of caller levels, the second partly empty
      clamps     two levels above zm(1) and two below zm(nzp1) around one inside: both clamps, twice each
      inside     strictly between the first and the last kept level of a zoom `kept`: it reads kept levels only
      one_out    `inside` and one level more, just below the last kept level: its last caller level reads one level
                 outside the zoom"""
    zm = np.asarray(zm, dtype=np.float64)
    lo, hi = kept[0], kept[0] + kept[1] - 1
    out = dict(vr.axes(zm))
    out["tiles100"] = zm[0] + (zm[-1] - zm[0]) * (np.arange(100) + 0.5) / 100.0
    out["clamps"] = np.array([zm[0] + 2.0, zm[0] + 1.0, 0.5 * (zm[3] + zm[4]), zm[-1] - 1.0, zm[-1] - 2.0])
    out["inside"] = zm[lo] + (zm[hi] - zm[lo]) * (np.arange(9) + 1.0) / 10.0
    out["one_out"] = np.append(out["inside"], 0.5 * (zm[hi] + zm[hi + 1]))
    for z in out.values():
        assert np.isfinite(z).all() and (np.diff(z) < 0).all()
    return out


def first_outside(zm, z, lev0, nlev):
    """The level rule in numpy, from vaxis_ref.levels_read: None if every model level an axis reads is one of
    lev0 .. lev0 + nlev - 1, else (caller level, model level) of the first read outside them."""
    for j, levels in enumerate(vr.levels_read(zm, z)):
        for lev in levels:
            if not lev0 <= lev < lev0 + nlev:
                return j, lev
    return None


# ---------------------------------------------------------------------------
# the header, the tables, the structs
# ---------------------------------------------------------------------------
def test_library_exports_exactly_the_functions_of_the_vrecords_header(api):
    protos = prototypes(HEADER)
    assert sorted(protos) == sorted(NAMES + HOST_NAMES)
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_vrecords.h but not exported"
    text = open(HEADER).read()
    for inc in ("mckpp_hip_vaxis.h", "mckpp_hip_device_records.h", "mckpp_hip_remap.h"):
        assert f'#include "{inc}"' in text
    assert re.search(r"#define\s+MCKPP_VRECORDS_PLANES_MAX\s+64\b", text)
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_(?:multi_)?vrecords_[a-z_0-9]+)\b", syms)))
    assert exported == sorted(NAMES + HOST_NAMES)
    # what the header has to say of the order of operations
    for phrase in ("interpolation of the minima", "NOT the minimum of the", "exact arithmetic only", "RECORD VALUE FIRST",
                   "Out of scope"):
        assert phrase in text, phrase


def test_vrecords_signatures_match_the_vrecords_header(api):
    protos = prototypes(HEADER)
    table = api._signatures_vrecords()
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
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_VRECORDS[one][2] and multi not in api._SIGNATURES_VRECORDS
    assert sorted(api._SIGNATURES_VRECORDS) == sorted(["mckpp_hip_" + n for n in TWINNED] + HOST_NAMES)
    # the eleventh table: no function of this header in another one
    others = [api._signatures(), api._signatures_device(), api._signatures_zoom(), api._signatures_records(),
              api._signatures_put(), api._signatures_reduce(), api._signatures_vaxis(), api._signatures_hgrid(),
              api._signatures_remap(), api._signatures_hv()]
    assert len(others) == 10 and not any(set(table) & set(o) for o in others)


@pytest.mark.parametrize("ctype", sorted(STRUCTS))
def test_struct_layouts_match_the_header(api, tmp_path, ctype):
    cls, want = getattr(api, STRUCTS[ctype][0]), STRUCTS[ctype][1]
    fields = [f[0] for f in cls._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
            f'printf("%zu\\n", sizeof({ctype}));']
    body += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(cls)
    seen = []
    for line in filter(None, out[1:]):
        name, off = line.split()
        assert getattr(cls, name).offset == int(off), name
        seen.append(name)
    assert seen == want


def test_both_handles_have_the_methods(api):
    for cls in (api.MckppHip, api.MckppHipMulti):
        assert issubclass(cls, api._AxisRecords)
        for n in ("vaxis_records_dev", "vaxis_records_host", "hv_records_dev"):
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over this table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_vrecords().items():
        if name in HOST_NAMES:
            continue
        assert res is C.c_int and argtypes[0] is api._H, name
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES


# ---------------------------------------------------------------------------
# the level rule
# ---------------------------------------------------------------------------
def _rule_cases():
    """(what, zm, z, lev0, nlev) on the model axes of the three cases: every caller axis against the whole axis, the
    zoom of the GPU tests, a single kept level and ranges that end at either end of the column"""
    for tag in CASES:
        zm = model_levels(tag)
        n = len(zm)
        for name, z in caller_axes(zm).items():
            for lev0, nlev in ((0, n), KEPT, (0, 1), (n - 1, 1), (0, 30), (n - 5, 5), (3, 1)):
                yield f"{tag} {name} {lev0}+{nlev}", zm, z, lev0, nlev
        # one double per row: an axis above the column reads level 0 alone, one below it the last level alone
        yield f"{tag} above", zm, np.array([zm[0] + 2.0, zm[0] + 1.0]), 0, 1
        yield f"{tag} below", zm, np.array([zm[-1] - 1.0, zm[-1] - 2.0]), n - 1, 1


def test_the_axes_of_the_gpu_tests_are_what_they_claim():
    for tag in CASES:
        zm = model_levels(tag)
        n = len(zm)
        assert n == lc.CASES[tag].nz + 1 and (np.diff(zm) < 0).all()
        ax = caller_axes(zm)
        branch = {a: list(vr.carried_brackets(zm, z)[0]) for a, z in ax.items()}
        assert len(ax["fine130"]) > 128 and 64 < len(ax["tiles100"]) < 128            # level tiles on the tx side
        assert set(branch["tiles100"]) == {vr.BRACKET}
        assert branch["clamps"] == [vr.ABOVE, vr.ABOVE, vr.BRACKET, vr.BELOW, vr.BELOW]  # both clamps
        assert sum(z in zm for z in ax["equal"]) >= 4                                  # the equality branch
        # every axis is accepted by the whole axis; the zoom accepts `inside` and of the others none
        lo, hi = KEPT[0], KEPT[0] + KEPT[1] - 1
        for a, z in ax.items():
            assert first_outside(zm, z, 0, n) is None, (tag, a)
            assert (first_outside(zm, z, *KEPT) is None) == (a == "inside"), (tag, a)
        read = sorted({lev for lv in vr.levels_read(zm, ax["inside"]) for lev in lv})
        assert read[0] == lo and read[-1] == hi and lo > 0, "`inside` reads rebased source levels, the first and the last kept one"
        assert first_outside(zm, ax["one_out"], *KEPT) == (len(ax["one_out"]) - 1, hi + 1)
        # a single kept level: an axis whose entries all read that one level, and no other
        assert first_outside(zm, [zm[0] + 2.0, zm[0] + 1.0], 0, 1) is None
        assert first_outside(zm, [zm[0] + 1.0, 0.5 * (zm[0] + zm[1])], 0, 1) == (1, 1)
        if n > 64:
            assert max(lev for lv in vr.levels_read(zm, ax["fine130"]) for lev in lv) >= 64   # source rows past one 64-level tile


def test_the_rule_of_the_library_is_the_numpy_statement(api):
    some = {True: 0, False: 0}
    for what, zm, z, lev0, nlev in _rule_cases():
        branch, kin, _, _ = api.host_vaxis_map(zm, z)
        want = first_outside(zm, z, lev0, nlev)
        assert api.host_vrecords_rule(branch, kin, lev0, nlev) == want, what
        some[want is None] += 1
    assert some[True] > 20 and some[False] > 20
    for bad in (dict(branch=[], kin=[], lev0=0, nlev=1), dict(branch=[2], kin=[0], lev0=0, nlev=0),
                dict(branch=[2, 2], kin=[0], lev0=0, nlev=1)):
        with pytest.raises(ValueError, match="host_vrecords_rule"):
            api.host_vrecords_rule(**bad)


def test_the_rule_on_its_own_under_the_sanitizers(tmp_path):
    """tests/vrecords_rule_main.cpp with mckpp_vaxis_map.cpp, built with -fsanitize=address,undefined and run as it is,
    on the same cases; every array of the program is a heap block of exactly its length"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "vrecords_rule")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", os.path.join(ROOT, "tests", "vrecords_rule_main.cpp"),
                           os.path.join(CSRC, "mckpp_vaxis_map.cpp"), "-o", exe])
    cases = list(_rule_cases())
    lines = []
    for _, zm, z, lev0, nlev in cases:
        lines.append(f"{len(zm)} {len(z)} {lev0} {nlev}")
        lines.append(" ".join(float(v).hex() for v in zm))
        lines.append(" ".join(float(v).hex() for v in z))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    assert len(out) == len(cases) + 1
    for (what, zm, z, lev0, nlev), line in zip(cases, out):
        want = first_outside(zm, z, lev0, nlev)
        assert tuple(int(v) for v in line.split()) == ((0, -1, -1) if want is None else (1,) + want), what


# ---------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_the_plane_builders_check_and_order_a_tuple_before_any_library_call(api, cls, monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(api, "_lib", lambda: stub)
    npts, nzp1, n, nlist = 12, 41, 5, 4
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    pre = h._pre
    h.hgrid_define(0, n, None, hr.csr([[(j, 1.0)] for j in range(n)]))
    h.vaxis_define(0, [0.0, -10.0, -50.0])
    h.vaxis_define(2, [-1.0, -2.0])
    every = api.WIN_MEAN | api.WIN_MIN | api.WIN_MAX | api.WIN_LAST
    h.window_schedule(0, 1, 3, 2, ("T", "S", "hmix"), every)
    h.window_schedule_zoom(1, 1, 3, 2, ("T", "difm"), api.WIN_MEAN, points=np.arange(nlist, dtype=np.int32), levels=(2, 7))
    del stub.calls[:]
    dev = FakeDeviceArray
    t3, f32, l2 = dev((3, npts), ptr=0x9000000), dev((3, npts), "<f4", ptr=0x8000000), dev((2, nlist))
    g3, g2 = dev((3, n), ptr=0x6000000), dev((2, n), "<f4", ptr=0x5000000)
    h3, h32 = np.zeros((3, npts)), np.zeros((2, nlist), dtype=np.float32)
    bad_dev = {
        "a numpy array": ([(0, 0, "T", 0, 0, h3)], "a host array"),
        "an undefined axis": ([(0, 0, "T", 0, 0, t3), (0, 0, "T", 0, 1, t3)], r"planes\[1\]: axis 1 is not defined"),
        "a two-dimensional field": ([(0, 0, "hmix", 0, 0, t3)], r"planes\[0\]: field hmix is two-dimensional"),
        "an interface field": ([(1, 0, "difm", 0, 0, l2)], r"planes\[0\]: field difm lives on the interface axis"),
        "an unknown field": ([(0, 0, "sst", 0, 0, t3)], r"planes\[0\]: unknown output field"),
        "a schedule that is not set": ([(2, 0, "T", 0, 0, t3)], r"planes\[0\]: .*schedule 2"),
        "a field the schedule does not keep": ([(1, 0, "S", 0, 0, t3)], r"planes\[0\]: "),
        "an op the schedule does not keep": ([(1, 0, "T", 3, 2, l2)], r"planes\[0\]: "),
        "a negative record": ([(0, -1, "T", 0, 0, t3)], r"planes\[0\]: record -1"),
        "the grid's points for a listed schedule": ([(1, 0, "T", 0, 2, dev((2, npts)))], r"out has shape \(2, 12\); .* is \(2, 4\)"),
        "points and levels swapped": ([(0, 0, "T", 0, 0, dev((npts, 3)))], r"out has shape \(12, 3\)"),
        "another axis' levels": ([(0, 0, "T", 0, 2, t3)], r"out has shape \(3, 12\); .* is \(2, 12\)"),
        "an array of integers": ([(0, 0, "T", 0, 0, dev((3, npts), "<i4"))], "element type <i4"),
        "a plane of five": ([(0, 0, "T", 0, t3)], r"planes\[0\] is \(sched, rec, field, op, axis, out\)"),
        "65 planes": ([(0, 0, "T", 0, 0, t3)] * 65, "65 planes, at most 64"),
    }
    for what, (planes, msg) in bad_dev.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_records_dev(planes)
        assert stub.calls == [], what
    bad_host = {
        "an array in device memory": ([(0, 0, "T", 0, 0, t3)], "an array in device memory"),
        "an undefined axis": ([(0, 0, "T", 0, 5, h3)], r"planes\[0\]: axis 5 is not defined"),
        "a two-dimensional field": ([(0, 0, "T", 0, 0, h3), (0, 0, "hmix", 0, 0, h3)], r"planes\[1\]: field hmix is two-dimensional"),
        "another axis' levels": ([(0, 0, "T", 0, 2, h3)], r"out has shape \(3, 12\)"),
        "an array of integers": ([(0, 0, "T", 0, 0, np.zeros((3, npts), dtype=np.int64))], "element type <i8"),
        "a plane of seven": ([(0, 0, "T", 0, 0, 0, h3)], r"planes\[0\] is \(sched, rec, field, op, axis, out\)"),
    }
    for what, (planes, msg) in bad_host.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_records_host(planes)
        assert stub.calls == [], what
    bad_hv = {
        "a numpy array": ([(0, 0, "T", 0, 0, 0, np.zeros((3, n)))], {}, "a host array"),
        "an undefined grid": ([(0, 0, "T", 0, 3, 0, g3)], {}, r"planes\[0\]: grid 3 is not defined"),
        "an undefined axis": ([(0, 0, "T", 0, 0, 1, g3)], {}, r"planes\[0\]: axis 1 is not defined"),
        "a two-dimensional field": ([(0, 0, "hmix", 0, 0, 0, g3)], {}, r"planes\[0\]: field hmix is two-dimensional"),
        "an array of the model's size": ([(0, 0, "T", 0, 0, 0, t3)], {}, r"out has shape \(3, 12\); axis 0 on grid 0 is \(3, 5\)"),
        "an unknown norm": ([(0, 0, "T", 0, 0, 0, g3)], dict(norm="area"), "norm 'area'"),
        "grid and axis left out": ([(0, 0, "T", 0, 0, g3)], {}, r"planes\[0\] is \(sched, rec, field, op, grid, axis, out\)"),
        "65 planes": ([(0, 0, "T", 0, 0, 0, g3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_hv.items():
        with pytest.raises(ValueError, match=msg):
            h.hv_records_dev(planes, **kw)
        assert stub.calls == [], what
    # well-formed calls reach the library with the right tables: the tuple's order, the dtype from the array
    F64, F32, O = api.EXP_F64, api.EXP_F32, api.OUT
    h.vaxis_records_dev([(0, 1, "T", 0, 0, t3), (0, 0, "S", 2, 0, f32)], land_value=-1.0)
    h.vaxis_records_dev([(1, 1, "T", 0, 2, l2)], fill_land=False)
    h.vaxis_records_host([(0, 1, "S", 3, 0, h3), (1, 0, "T", 0, 2, h32)], land_value=2.0)
    h.hv_records_dev([(0, 1, "T", 1, 0, 0, g3), (1, 0, "T", 0, 0, 2, g2)], norm="used", fill_land=False)
    names = ["vrecords_vaxis_dev", "vrecords_vaxis_dev", "vrecords_vaxis_host", "vrecords_hv_dev"]
    assert [c[0] for c in stub.calls] == [pre + x for x in names]
    fields = STRUCTS["mckpp_vaxis_record_plane_c"][1]

    def table(call):
        return [tuple(getattr(call[1][2][k], f) for f in fields) for k in range(call[1][1])]

    assert table(stub.calls[0]) == [(0, O["T"], 0, 0, F64, 1, 1, -1.0, 0x9000000), (0, O["S"], 2, 0, F32, 1, 0, -1.0, 0x8000000)]
    assert table(stub.calls[1]) == [(1, O["T"], 0, 2, F64, 0, 1, 1e20, 0x7000000)]
    assert len(stub.calls[1][1]) == 4 and len(stub.calls[2][1]) == 3        # a stream with the device form, none with the host's
    assert table(stub.calls[2]) == [(0, O["S"], 3, 0, F64, 1, 1, 2.0, h3.ctypes.data), (1, O["T"], 0, 2, F32, 1, 0, 2.0, h32.ctypes.data)]
    fields = STRUCTS["mckpp_hv_record_plane_c"][1]
    assert table(stub.calls[3]) == [(0, O["T"], 1, 0, F64, 0, 1, 0, 1, 1e20, 0x6000000), (1, O["T"], 0, 2, F32, 0, 1, 0, 0, 1e20, 0x5000000)]
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_vrecords_bindings(built, tmp_path):
    """A program that uses the two types, the constant and the six interfaces compiles and links against the layer."""
    src = tmp_path / "uses_vrecords.F90"
    src.write_text("""program uses_vrecords
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_vaxis_record_plane_c, mckpp_hv_record_plane_c, MCKPP_OUT_T, MCKPP_EXP_F32, MCKPP_EXP_F64, &
    MCKPP_VRECORDS_PLANES_MAX, MCKPP_HGRID_NORM_USED, mckpp_hip_vrecords_vaxis_dev, mckpp_hip_vrecords_vaxis_host, &
    mckpp_hip_vrecords_hv_dev, mckpp_hip_multi_vrecords_vaxis_dev, mckpp_hip_multi_vrecords_vaxis_host, &
    mckpp_hip_multi_vrecords_hv_dev
  implicit none
  type(mckpp_vaxis_record_plane_c) :: v(1)
  type(mckpp_hv_record_plane_c) :: hv(1)
  integer(c_int) :: rc
  v(1) = mckpp_vaxis_record_plane_c(1, MCKPP_OUT_T, 0, 5, MCKPP_EXP_F32, 1, 7_c_int64_t, 1.0e20_c_double, c_null_ptr)
  hv(1) = mckpp_hv_record_plane_c(1, MCKPP_OUT_T, 0, 6, MCKPP_EXP_F64, 2, MCKPP_HGRID_NORM_USED, 1, 8_c_int64_t, &
                                  1.0e20_c_double, c_null_ptr)
  if (v(1)%axis /= 5 .or. v(1)%rec /= 7 .or. hv(1)%axis /= 6 .or. hv(1)%grid /= 2 .or. hv(1)%rec /= 8) error stop 1
  if (MCKPP_VRECORDS_PLANES_MAX /= 64) error stop 2
  if (command_argument_count() > 0) then
    rc = mckpp_hip_vrecords_vaxis_dev(c_null_ptr, 1, v, c_null_ptr)
    rc = mckpp_hip_vrecords_vaxis_host(c_null_ptr, 1, v)
    rc = mckpp_hip_vrecords_hv_dev(c_null_ptr, 1, hv, c_null_ptr)
    rc = mckpp_hip_multi_vrecords_vaxis_dev(c_null_ptr, 1, v, c_null_ptr)
    rc = mckpp_hip_multi_vrecords_vaxis_host(c_null_ptr, 1, v)
    rc = mckpp_hip_multi_vrecords_hv_dev(c_null_ptr, 1, hv, c_null_ptr)
  end if
end program uses_vrecords
""")
    exe = tmp_path / "uses_vrecords"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
