"""CPU side of the caller's vertical axes (include/mckpp_hip_vaxis.h): the library exports what the header declares and
nothing else of those names, api._SIGNATURES_VAXIS states those functions type by type (the other tables still describe
their own headers), the three structs have the C layout, every entry point refuses a null handle by its own name, the
Python methods refuse a malformed call before the library is reached and hand a well-formed one over as the right
table, the Fortran layer builds with the new types and interfaces - and mckpp_host_vaxis_map, the one piece of the
feature that needs no GPU, fills the table that tests/vaxis_ref.py's restatement of the reference gives, from the
library and from a stand-alone program built under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import common as cm
import vaxis_ref as vr
from harness import api, bound_as, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADERS = {n: os.path.join(ROOT, "include", f) for n, f in (
    ("first", "mckpp_hip.h"), ("device", "mckpp_hip_device.h"), ("zoom", "mckpp_hip_zoom.h"),
    ("records", "mckpp_hip_device_records.h"), ("put", "mckpp_hip_put.h"), ("reduce", "mckpp_hip_reduce.h"),
    ("vaxis", "mckpp_hip_vaxis.h"))}
CSRC = os.path.join(ROOT, "mckpp_f90_amd", "csrc")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("vaxis_define", "vaxis_put_dev", "vaxis_put_host", "vaxis_init_profiles_dev", "vaxis_init_profiles_host",
           "vaxis_fetch_dev")
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
HOST_NAMES = ["mckpp_host_vaxis_map"]
STRUCTS = {
    "mckpp_vaxis_put_plane_c": ("_VaxisPutPlaneC", ["field", "axis", "dtype", "op", "flags", "skip_value", "in"]),
    "mckpp_vaxis_profiles_c": ("_VaxisProfilesC", ["axis_vel", "axis_temp", "axis_sal", "dtype", "tk0", "u", "v", "temp", "sal"]),
    "mckpp_vaxis_dev_plane_c": ("_VaxisDevPlaneC", ["field", "axis", "dtype", "fill_land", "land_value", "out"]),
}
GRIDS = {"uniform40": 40, "uniform100": 100}     # the grids of every_step_nz40 / sweep_nd3 and of deep_nz100_nd4


def _zm(nz):
    return np.ascontiguousarray(cm.grid_for(nz, "uniform")[0][1:nz + 2])


def _pairs():
    """(what, source levels, target levels): every axis of vaxis_ref.axes against both grids, in both directions - the
    in table (the axis as source, zm as targets) and the out table (zm as source)"""
    for g, nz in GRIDS.items():
        zm = _zm(nz)
        for name, z in vr.axes(zm).items():
            yield f"{g} {name} in", z, zm
            yield f"{g} {name} out", zm, z


def test_library_exports_exactly_the_functions_of_the_vaxis_header(api):
    protos = prototypes(HEADERS["vaxis"])
    assert sorted(protos) == sorted(NAMES + HOST_NAMES)
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_vaxis.h but not exported"
    src = open(HEADERS["vaxis"]).read()
    assert '#include "mckpp_hip_put.h"' in src
    # ... and nothing of these names that the header does not declare
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_(?:multi_)?vaxis_[a-z_0-9]+)\b", syms)))
    assert exported == sorted(NAMES + HOST_NAMES)


def test_vaxis_signatures_match_the_vaxis_header(api):
    protos = prototypes(HEADERS["vaxis"])
    table = api._signatures_vaxis()
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
    src = re.sub(r"/\*.*?\*/", "", open(HEADERS["vaxis"]).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_VAXIS[one][2] and multi not in api._SIGNATURES_VAXIS
    assert not api._SIGNATURES_VAXIS["mckpp_host_vaxis_map"][2]
    # the constants of the header are the Python layer's
    for name, value in re.findall(r"\b(MCKPP_VAXIS_[A-Z]+)\s*=\s*(\d+)", src):
        assert getattr(api, name[len("MCKPP_"):]) == int(value), name
    full = open(HEADERS["vaxis"]).read()
    assert re.search(r"#define\s+MCKPP_VAXES\s+8\b", full) and api.VAXES == 8
    assert re.search(r"#define\s+MCKPP_VAXIS_LEVELS_MAX\s+1024\b", full) and api.VAXIS_LEVELS_MAX == 1024
    assert re.search(r"#define\s+MCKPP_VAXIS_PLANES_MAX\s+64\b", full)


def test_the_other_tables_still_describe_their_headers(api):
    protos = {n: prototypes(h) for n, h in HEADERS.items()}
    tables = {"first": api._signatures(), "device": api._signatures_device(), "zoom": api._signatures_zoom(),
              "records": api._signatures_records(), "put": api._signatures_put(), "reduce": api._signatures_reduce(),
              "vaxis": api._signatures_vaxis()}
    assert len(protos["first"]) == 114
    for n in HEADERS:
        assert sorted(tables[n]) == sorted(protos[n]), n
        for other in HEADERS:
            if other != n:
                assert not set(protos[n]) & set(protos[other]), f"a function declared in both the {n} and the {other} header"
                assert not set(tables[n]) & set(tables[other])


@pytest.mark.parametrize("ctype", sorted(STRUCTS))
def test_struct_layouts_match_the_header(api, tmp_path, ctype):
    cls, want = getattr(api, STRUCTS[ctype][0]), STRUCTS[ctype][1]
    fields = [f[0] for f in cls._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADERS["vaxis"]}"', "int main(void){",
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


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over this table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_vaxis().items():
        if name in HOST_NAMES:
            continue
        assert res is C.c_int and argtypes[0] is api._H, name
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES
    z = (C.c_double * 2)(0.0, -1.0)
    put, out, prof = (api._VaxisPutPlaneC * 1)(), (api._VaxisDevPlaneC * 1)(), api._VaxisProfilesC()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):   # ... and with arguments
        for n, args in (("vaxis_define", (0, 2, z)), ("vaxis_put_dev", (1, put, None)), ("vaxis_put_host", (1, put)),
                        ("vaxis_init_profiles_dev", (C.byref(prof), None)), ("vaxis_init_profiles_host", (C.byref(prof),)),
                        ("vaxis_fetch_dev", (1, out, None))):
            assert getattr(lib, pre + n)(None, *args) == -1
            assert lib.mckpp_hip_last_error() == (pre + n + ": null handle").encode()


# ---------------------------------------------------------------------------
# the axis table, without a GPU
# ---------------------------------------------------------------------------
def test_the_axes_reach_every_branch():
    """what the axes of vaxis_ref.axes are chosen for, on both grids"""
    A, B, K = vr.ABOVE, vr.BELOW, vr.BRACKET
    for g, nz in GRIDS.items():
        zm = _zm(nz)
        ax = vr.axes(zm)
        assert (np.diff(zm) < 0).all() and len(zm) == nz + 1
        b, k = vr.carried_brackets(ax["two"], zm)
        assert len(ax["two"]) == 2 and (b == K).all() and (k == 0).all()
        b, k = vr.carried_brackets(ax["coarse7"], zm)
        assert (b == A).sum() >= 3 and (b == B).sum() >= 3 and max(np.bincount(k[b == K])) >= 3 and len(set(k[b == K])) == 6
        b, k = vr.carried_brackets(ax["fine130"], zm)
        assert len(ax["fine130"]) == 130 > 2 * 64 and (b == K).all() and (np.diff(k) > 1).any()
        b, k = vr.carried_brackets(zm, ax["fine130"])     # the out table of the same axis: both clamps, shared brackets
        assert (b == A).any() and (b == B).any() and (np.diff(k[b == K]) == 0).any()
        z = ax["equal"]
        assert z[0] == zm[0] and z[-1] == zm[-1] and len(set(z[1:-1]) & set(zm[1:-1])) == 2
        for zs, zt in ((z, zm), (zm, z)):
            b, k = vr.carried_brackets(zs, zt)
            assert (b == K).all(), "equality belongs to the bracket branch"
            assert k[0] == 0 and zt[0] - zs[0] == 0.0                      # on the first level: kin = 0, t = 0
            assert k[-1] == len(zs) - 2 and zt[-1] == zs[-1]               # on the last: the last pair
            inner = [j for j in range(1, len(zt) - 1) if zt[j] in zs]
            assert len(inner) >= 2 and all(zs[k[j] + 1] == zt[j] for j in inner)   # on an interior one: it ends the pair


def test_host_vaxis_map_fills_the_restatements_table(api):
    """branch and kin are the reference's carried search and the header's smallest-index rule, which agree; t and dz are
    the one subtraction each, bit for bit"""
    n = 0
    for what, zs, zt in _pairs():
        branch, kin, t, dz = api.host_vaxis_map(zs, zt)
        for rule in (vr.carried_brackets, vr.smallest_brackets):
            b, k = rule(zs, zt)
            assert np.array_equal(branch, b) and np.array_equal(kin, k), (what, rule.__name__)
        br = branch == vr.BRACKET
        assert np.array_equal(t[br], (zt - zs[kin])[br]) and np.array_equal(dz[br], (zs[kin] - zs[np.minimum(kin + 1, len(zs) - 1)])[br]), what
        assert (t[~br] == 0.0).all() and (dz[~br] == 1.0).all(), what
        assert (kin[branch == vr.ABOVE] == 0).all() and (kin[branch == vr.BELOW] == len(zs) - 1).all(), what
        assert (kin[br] + 1 < len(zs)).all() and (kin >= 0).all(), what
        n += 1
    assert n == 16


def test_host_vaxis_map_refuses_what_is_no_axis(api):
    good = np.array([0.0, -1.0, -2.0])
    for bad in ([0.0], [0.0, 0.0], [0.0, 1.0], [0.0, -1.0, -1.0], [0.0, float("nan")], [float("inf"), 0.0], []):
        with pytest.raises(ValueError, match="host_vaxis_map"):
            api.host_vaxis_map(bad, good)
        if len(bad) != 1:     # (one target is a table; one source level is no axis)
            with pytest.raises(ValueError, match="host_vaxis_map"):
                api.host_vaxis_map(good, bad)
    assert api.host_vaxis_map(good, [-0.5])[1][0] == 0


def test_the_map_on_its_own_under_the_sanitizers(tmp_path):
    """tests/vaxis_map_main.cpp with mckpp_vaxis_map.cpp, built with -fsanitize=address,undefined and run as it is, on
    the same axes; every array of the program is a heap block of exactly its length"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "vaxis_map")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", os.path.join(ROOT, "tests", "vaxis_map_main.cpp"),
                           os.path.join(CSRC, "mckpp_vaxis_map.cpp"), "-o", exe])
    pairs = list(_pairs())
    bad = [("not decreasing", np.array([0.0, -2.0, -1.0]), np.array([-0.5])), ("nan", np.array([0.0, -1.0]), np.array([np.nan]))]
    lines = []
    for _, zs, zt in pairs + bad:
        lines.append(f"{len(zs)} {len(zt)}")
        lines.append(" ".join(float(z).hex() for z in zs))
        lines.append(" ".join(float(z).hex() for z in zt))
    (tmp_path / "axes.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(tmp_path / "axes.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(r.stdout.split("\n"))
    for what, zs, zt in pairs:
        assert next(out) == "0", what
        b, k = vr.carried_brackets(zs, zt)
        for j in range(len(zt)):
            branch, kin, t, dz = next(out).split()
            assert (int(branch), int(kin)) == (b[j], k[j]), (what, j)
            if b[j] == vr.BRACKET:
                assert float.fromhex(t) == zt[j] - zs[k[j]] and float.fromhex(dz) == zs[k[j]] - zs[k[j] + 1], (what, j)
    assert [next(out) for _ in bad] == ["-1", "-1"]


# ---------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------
class _Stub:
    """a library whose entry points all succeed, and which keeps what they were called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _table(args, fields):
    n, tab = args[1], args[2]
    return [tuple(getattr(tab[k], f) for f in fields) for k in range(n)]


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_any_library_call(api, cls, monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(api, "_lib", lambda: stub)
    npts, nzp1 = 12, 41
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    pre = h._pre
    # axes
    bad_axes = {
        "an axis number past the last": ((8, [0.0, -1.0]), "axis 8"),
        "a negative axis number": ((-1, [0.0, -1.0]), "axis -1"),
        "a bool": ((True, [0.0, -1.0]), "axis True"),
        "one level": ((0, [0.0]), r"shape \(1,\)"),
        "two dimensions": ((0, np.zeros((2, 2))), r"shape \(2, 2\)"),
        "1025 levels": ((0, -np.arange(1025.0)), r"shape \(1025,\)"),
        "a NaN": ((0, [0.0, float("nan")]), "not finite"),
        "an increasing axis": ((0, [-5.0, -1.0]), "does not strictly decrease"),
        "a repeated level": ((0, [0.0, -1.0, -1.0]), "does not strictly decrease"),
    }
    for what, (args, msg) in bad_axes.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_define(*args)
        assert stub.calls == [], what
    h.vaxis_define(0, [0.0, -10.0, -200.0])
    h.vaxis_define(3, -np.arange(130.0))
    h.vaxis_define(5, [1.0, 0.0])
    h.vaxis_define(5, None)
    assert [c[0] for c in stub.calls] == [pre + "vaxis_define"] * 4
    assert [c[1][1:3] for c in stub.calls] == [(0, 3), (3, 130), (5, 2), (5, 0)] and h._vaxes() == {0: 3, 3: 130}
    del stub.calls[:]
    dev = FakeDeviceArray
    d3, d130, f3 = dev((3, npts)), dev((130, npts), ptr=0x9000000), dev((3, npts), "<f4", ptr=0x8000000)
    n3, n130 = np.zeros((3, npts)), np.zeros((130, npts), dtype=np.float32)
    nan = float("nan")
    bad_dev = {
        "a numpy array": ([("T", 0, n3)], {}, "a host array"),
        "an integer array": ([("T", 0, dev((3, npts), "<i8"))], {}, "element type <i8"),
        "a non-contiguous array": ([("T", 0, dev((3, npts), strides=(8, 24)))], {}, "not C-contiguous"),
        "an array of the model's size": ([("T", 0, dev((nzp1, npts)))], {}, f"the call takes {3 * npts} elements"),
        "an array of another axis": ([("T", 3, d3)], {}, f"the call takes {130 * npts} elements"),
        "an undefined axis": ([("T", 1, d3)], {}, r"planes\[0\]: axis 1 is not defined"),
        "a dropped axis": ([("u", 0, d3), ("T", 5, d3)], {}, r"planes\[1\]: axis 5 is not defined"),
        "an axis that is no number": ([("T", "0", d3)], {}, "axis '0' is not defined"),
        "an unknown field": ([("sst", 0, d3)], {}, r"planes\[0\]: unknown output field"),
        "hmix": ([("hmix", 0, d3)], {}, r"planes\[0\]: field hmix is an output of the step, not state"),
        "rho": ([("T", 0, d3), ("rho", 0, d3)], {}, r"planes\[1\]: field rho is an output of the step, not state"),
        "two planes on one field": ([("T", 0, d3), ("u", 0, d3), ("T", 3, d130)], {}, r"planes\[2\] and planes\[0\] write T"),
        "S over S_anom": ([("S_anom", 0, d3), ("S", 0, d3)], {}, r"planes\[1\] and planes\[0\] write S"),
        "a NaN skip value": ([("T", 0, d3)], dict(skip=nan), "skip is NaN"),
        "an unknown op": ([("T", 0, d3)], dict(op="mul"), "op 'mul'"),
        "a plane of two": ([("T", d3)], {}, r"planes\[0\] is \(field, axis, array\)"),
        "a plane of four": ([("T", 0, d3, 0)], {}, r"planes\[0\] is \(field, axis, array\)"),
        "65 planes": ([("T", 0, d3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_dev.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_put_dev(planes, **kw)
        assert stub.calls == [], what
    with pytest.raises(ValueError, match="stream"):
        h.vaxis_put_dev([("T", 0, d3)], stream="0")
    bad_host = {
        "a device array": ([("T", 0, d3)], {}, "an array in device memory"),
        "a list": ([("T", 0, [0.0] * 3 * npts)], {}, "no numpy array"),
        "a Fortran-ordered array": ([("T", 0, np.zeros((3, npts), order="F"))], {}, "not C-contiguous"),
        "an array of another size": ([("T", 3, n3)], {}, f"the call takes {130 * npts} elements"),
        "two planes on one field": ([("v", 0, n3), ("v", 3, n130)], {}, r"planes\[1\] and planes\[0\] write v"),
        "an undefined axis": ([("T", 7, n3)], {}, "axis 7 is not defined"),
    }
    for what, (planes, kw, msg) in bad_host.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_put_host(planes, **kw)
        assert stub.calls == [], what
    bad_fetch = {
        "a numpy array": ([("T", 0, n3)], "a host array"),
        "hmix": ([("hmix", 0, d3)], r"planes\[0\]: field hmix is two-dimensional"),
        "a flux on the interfaces": ([("T", 0, d3), ("wT", 0, d3)], r"planes\[1\]: field wT lives on the interface axis"),
        "a diffusivity": ([("difm", 0, d3)], r"field difm lives on the interface axis"),
        "a forcing field": ([("solar_in", 0, d3)], "field solar_in is two-dimensional"),
        "an undefined axis": ([("rho", 2, d3)], r"planes\[0\]: axis 2 is not defined"),
        "an array of the model's size": ([("rho", 3, dev((nzp1, npts)))], f"the call takes {130 * npts} elements"),
        "an integer array": ([("T", 0, dev((3, npts), "<i4"))], "element type <i4"),
        "a plane of two": ([("T", d3)], r"planes\[0\] is \(field, axis, out\)"),
        "65 planes": ([("T", 0, d3)] * 65, "65 planes, at most 64"),
    }
    for what, (planes, msg) in bad_fetch.items():
        with pytest.raises(ValueError, match=msg):
            h.vaxis_fetch_dev(planes)
        assert stub.calls == [], what
    bad_init = {
        "a numpy array": (dict(u=n3), {}, "vaxis_init_profiles_dev: u: a host array"),
        "an undefined axis": ({}, dict(axis_temp=4), "temp: axis 4 is not defined"),
        "sal on another axis' size": ({}, dict(axis_sal=3), f"sal: shape \\(3, {npts}\\), the call takes {130 * npts} elements"),
        "mixed element types": (dict(v=f3), {}, "element types"),
        "a tk0 that is not finite": ({}, dict(tk0=nan), "tk0 is not finite"),
    }
    for what, (arrays, kw, msg) in bad_init.items():
        a = {**dict(u=d3, v=d3, temp=d3, sal=d3), **arrays}
        with pytest.raises(ValueError, match=msg):
            h.vaxis_init_profiles_dev(a["u"], a["v"], a["temp"], a["sal"], **{**dict(axis_vel=0, axis_temp=0, axis_sal=0), **kw})
        assert stub.calls == [], what
    with pytest.raises(ValueError, match="vaxis_init_profiles_host: temp: an array in device memory"):
        h.vaxis_init_profiles_host(n3, n3, d3, n3, 0, 0, 0)
    assert stub.calls == []
    # well-formed calls reach the library with the right tables
    F64, F32, O = api.EXP_F64, api.EXP_F32, api.OUT
    PUT, OUTP = STRUCTS["mckpp_vaxis_put_plane_c"][1], STRUCTS["mckpp_vaxis_dev_plane_c"][1]
    h.vaxis_put_dev([("T", 0, d3), ("S", 3, d130), ("u", 0, f3)])
    h.vaxis_put_dev([("S_anom", 0, f3)], op="add", time_levels=True, skip=1e20, fence=True)
    h.vaxis_put_host([("v", 0, n3), ("T", 3, n130)], op=api.PUT_ADD, skip=0.0)
    h.vaxis_put_dev([])
    h.vaxis_fetch_dev([("T", 0, d3), ("rho", 3, d130), ("S", 0, f3)], land_value=-1.0)
    h.vaxis_fetch_dev([("dbloc", 0, d3)], fill_land=False)
    h.vaxis_init_profiles_dev(d3, d3, d130, d3, 0, 3, 0)
    h.vaxis_init_profiles_host(n130, n130, n130, n130, 3, 3, 3, tk0=273.0)
    names = ["vaxis_put_dev", "vaxis_put_dev", "dev_fence", "vaxis_put_host", "vaxis_put_dev", "vaxis_fetch_dev", "vaxis_fetch_dev",
             "vaxis_init_profiles_dev", "vaxis_init_profiles_host"]
    assert [c[0] for c in stub.calls] == [pre + n for n in names]
    a = stub.calls[0][1]
    assert _table(a, PUT) == [(O["T"], 0, F64, 0, 0, 0.0, 0x7000000), (O["S"], 3, F64, 0, 0, 0.0, 0x9000000),
                              (O["u"], 0, F32, 0, 0, 0.0, 0x8000000)]
    assert a[3].value is None and len(a) == 4
    assert _table(stub.calls[1][1], PUT) == [(O["S_anom"], 0, F32, 1, 3, 1e20, 0x8000000)]
    b = stub.calls[3][1]
    assert _table(b, PUT) == [(O["v"], 0, F64, 1, 1, 0.0, n3.ctypes.data), (O["T"], 3, F32, 1, 1, 0.0, n130.ctypes.data)] and len(b) == 3
    assert stub.calls[4][1][1] == 0
    assert _table(stub.calls[5][1], OUTP) == [(O["T"], 0, F64, 1, -1.0, 0x7000000), (O["rho"], 3, F64, 1, -1.0, 0x9000000),
                                             (O["S"], 0, F32, 1, -1.0, 0x8000000)]
    assert _table(stub.calls[6][1], OUTP) == [(O["dbloc"], 0, F64, 0, 1e20, 0x7000000)]
    p = stub.calls[7][1][1]._obj     # (what byref holds)
    assert (p.axis_vel, p.axis_temp, p.axis_sal, p.dtype, p.tk0, p.u, p.v, p.temp, p.sal) == \
        (0, 3, 0, F64, 273.15, 0x7000000, 0x7000000, 0x9000000, 0x7000000)
    assert len(stub.calls[7][1]) == 3 and len(stub.calls[8][1]) == 2
    p = stub.calls[8][1][1]._obj
    assert (p.axis_vel, p.dtype, p.tk0, p.sal) == (3, F32, 273.0, n130.ctypes.data)
    assert h._held == {} and d3 in h._dev_held
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_vaxis_bindings(built, tmp_path):
    """A program that uses the three types, the constants and every interface compiles and links against the layer, and
    the table it gets from mckpp_host_vaxis_map is the restatement's."""
    src = tmp_path / "uses_vaxis.F90"
    src.write_text("""program uses_vaxis
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_vaxis_put_plane_c, mckpp_vaxis_profiles_c, mckpp_vaxis_dev_plane_c, MCKPP_OUT_T, &
    MCKPP_EXP_F64, MCKPP_EXP_F32, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, MCKPP_VAXES, MCKPP_VAXIS_LEVELS_MAX, MCKPP_VAXIS_PLANES_MAX, &
    MCKPP_VAXIS_ABOVE, MCKPP_VAXIS_BELOW, MCKPP_VAXIS_BRACKET, mckpp_host_vaxis_map, &
    mckpp_hip_vaxis_define, mckpp_hip_vaxis_put_dev, mckpp_hip_vaxis_put_host, mckpp_hip_vaxis_init_profiles_dev, &
    mckpp_hip_vaxis_init_profiles_host, mckpp_hip_vaxis_fetch_dev, mckpp_hip_multi_vaxis_define, mckpp_hip_multi_vaxis_put_dev, &
    mckpp_hip_multi_vaxis_put_host, mckpp_hip_multi_vaxis_init_profiles_dev, mckpp_hip_multi_vaxis_init_profiles_host, &
    mckpp_hip_multi_vaxis_fetch_dev
  implicit none
  type(mckpp_vaxis_put_plane_c) :: planes(1)
  type(mckpp_vaxis_dev_plane_c) :: outs(1)
  type(mckpp_vaxis_profiles_c) :: prof
  real(c_double) :: zs(3), zt(5), t(5), dz(5)
  integer(c_int32_t) :: branch(5), kin(5)
  integer(c_int) :: rc
  planes(1) = mckpp_vaxis_put_plane_c(MCKPP_OUT_T, 2, MCKPP_EXP_F64, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, 1.0e20_c_double, c_null_ptr)
  outs(1) = mckpp_vaxis_dev_plane_c(MCKPP_OUT_T, 2, MCKPP_EXP_F32, 1, 1.0e20_c_double, c_null_ptr)
  prof = mckpp_vaxis_profiles_c(0, 1, 2, MCKPP_EXP_F64, 273.15_c_double, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
  if (planes(1)%axis /= 2 .or. outs(1)%fill_land /= 1 .or. prof%axis_sal /= 2) error stop 1
  if (MCKPP_VAXES /= 8 .or. MCKPP_VAXIS_LEVELS_MAX /= 1024 .or. MCKPP_VAXIS_PLANES_MAX /= 64) error stop 2
  zs = [0.0_c_double, -10.0_c_double, -30.0_c_double]
  zt = [1.0_c_double, 0.0_c_double, -10.0_c_double, -30.0_c_double, -31.0_c_double]
  rc = mckpp_host_vaxis_map(3, zs, 5, zt, branch, kin, t, dz)
  if (rc /= 0) error stop 3
  if (any(branch /= [MCKPP_VAXIS_ABOVE, MCKPP_VAXIS_BRACKET, MCKPP_VAXIS_BRACKET, MCKPP_VAXIS_BRACKET, MCKPP_VAXIS_BELOW])) error stop 4
  if (any(kin /= [0, 0, 0, 1, 2]) .or. t(3) /= -10.0_c_double .or. dz(4) /= 20.0_c_double) error stop 5
  if (command_argument_count() > 0) then
    rc = mckpp_hip_vaxis_define(c_null_ptr, 0, 3, zs)
    rc = mckpp_hip_vaxis_put_dev(c_null_ptr, 1, planes, c_null_ptr)
    rc = mckpp_hip_vaxis_put_host(c_null_ptr, 1, planes)
    rc = mckpp_hip_vaxis_init_profiles_dev(c_null_ptr, prof, c_null_ptr)
    rc = mckpp_hip_vaxis_init_profiles_host(c_null_ptr, prof)
    rc = mckpp_hip_vaxis_fetch_dev(c_null_ptr, 1, outs, c_null_ptr)
    rc = mckpp_hip_multi_vaxis_define(c_null_ptr, 0, 3, zs)
    rc = mckpp_hip_multi_vaxis_put_dev(c_null_ptr, 1, planes, c_null_ptr)
    rc = mckpp_hip_multi_vaxis_put_host(c_null_ptr, 1, planes)
    rc = mckpp_hip_multi_vaxis_init_profiles_dev(c_null_ptr, prof, c_null_ptr)
    rc = mckpp_hip_multi_vaxis_init_profiles_host(c_null_ptr, prof)
    rc = mckpp_hip_multi_vaxis_fetch_dev(c_null_ptr, 1, outs, c_null_ptr)
  end if
end program uses_vaxis
""")
    exe = tmp_path / "uses_vaxis"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
