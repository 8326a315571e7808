"""CPU side of records out and state in on the caller's horizontal grids (include/mckpp_hip_remap.h): the header
declares exactly the four functions and the library exports them, api._SIGNATURES_REMAP states them type by type and is
disjoint from the other eight tables, the two structs have the C layout, both handles have the methods, every entry
point refuses a null handle by its own name, the Python methods refuse a malformed call before the library is reached,
and the Fortran layer builds with the new types and interfaces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
import hgrid_ref as hr
from harness import api, bound_as, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip_remap.h")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("remap_records_dev", "remap_put_dev")
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
STRUCTS = {
    "mckpp_remap_record_plane_c": ("_RemapRecordPlaneC", ["sched", "field", "op", "lev0", "nlev", "dtype", "grid", "norm",
                                                           "fill_land", "rec", "land_value", "out"]),
    "mckpp_remap_put_plane_c": ("_RemapPutPlaneC", ["field", "lev0", "nlev", "dtype", "op", "flags", "grid", "skip_value", "in"]),
}


def test_library_exports_exactly_the_functions_of_the_remap_header(api):
    protos = prototypes(HEADER)
    assert sorted(protos) == NAMES
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_remap.h but not exported"
    text = open(HEADER).read()
    for inc in ("mckpp_hip_hgrid.h", "mckpp_hip_device_records.h", "mckpp_hip_put.h"):
        assert f'#include "{inc}"' in text
    assert re.search(r"#define\s+MCKPP_REMAP_PLANES_MAX\s+64\b", text)
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_(?:multi_)?remap_[a-z_0-9]+)\b", syms)))
    assert exported == NAMES     # and no host function: mckpp_host_hgrid_apply and _slices state the host side


def test_remap_signatures_match_the_remap_header(api):
    protos = prototypes(HEADER)
    table = api._signatures_remap()
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
        assert api._SIGNATURES_REMAP[one][2] and multi not in api._SIGNATURES_REMAP
    assert sorted(api._SIGNATURES_REMAP) == sorted("mckpp_hip_" + n for n in TWINNED)
    # the ninth table: no function of this header in another one
    others = [api._signatures(), api._signatures_device(), api._signatures_zoom(), api._signatures_records(),
              api._signatures_put(), api._signatures_reduce(), api._signatures_vaxis(), api._signatures_hgrid()]
    assert len(others) == 8 and not any(set(table) & set(o) for o in others)


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
        for n in TWINNED:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over this table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_remap().items():
        assert res is C.c_int and argtypes[0] is api._H, name
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES


class _Stub:
    """a library whose entry points all succeed, and which keeps what they were called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_any_library_call(api, cls, monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(api, "_lib", lambda: stub)
    npts, nzp1, n = 12, 41, 5
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    pre = h._pre
    h.hgrid_define(0, n, hr.csr([[(p % n, 1.0)] for p in range(npts)]), hr.csr([[(j, 1.0)] for j in range(n)]))
    h.hgrid_define(1, 7, hr.csr([[(0, 1.0)]] * npts))
    O, MEAN, LAST = api.OUT, api.OP_MEAN, api.OP_LAST
    whole, zoomed = api._Kept({O["T"]: 0b1001, O["hmix"]: 0b0001}), api._Kept({O["T"]: 0b0001})
    zoomed.zoom = (6, 2)      # six listed points, two levels
    h._scheds().update({0: whole, 1: zoomed})
    del stub.calls[:]
    dev = FakeDeviceArray
    one, t3, f32 = dev((1, n)), dev((3, n), ptr=0x9000000), dev((1, n), "<f4", ptr=0x8000000)
    bad_records = {
        "a numpy array": ([(0, 0, "T", MEAN, 0, np.zeros((1, n)))], {}, "a host array"),
        "an undefined grid": ([(0, 0, "T", MEAN, 0, t3), (0, 0, "T", MEAN, 3, t3)], {}, r"planes\[1\]: grid 3 is not defined"),
        "a schedule that is not set": ([(2, 0, "T", MEAN, 0, t3)], {}, r"planes\[0\]: field T is not in output schedule 2"),
        "a field not kept": ([(0, 0, "S", MEAN, 0, t3)], {}, r"planes\[0\]: field S is not in output schedule 0"),
        "an op not kept": ([(0, 0, "T", api.OP_MIN, 0, t3)], {}, "keeps no op 1 of field T"),
        "a negative record": ([(0, -1, "T", MEAN, 0, t3)], {}, r"planes\[0\]: record -1"),
        "levels past the axis": ([(0, 0, "T", MEAN, 0, t3, 40, 3)], {}, r"levels 40 \.\. 42 of field T"),
        "levels past the zoom's": ([(1, 0, "T", MEAN, 0, t3)], {}, r"levels 0 \.\. 2 of field T, of which output schedule 1 keeps 2"),
        "two levels of hmix": ([(0, 0, "hmix", MEAN, 0, dev((2, n)))], {}, "schedule 0 keeps 1"),
        "an array of the model's size": ([(0, 0, "T", MEAN, 0, dev((3, npts)), 0, 3)], {}, r"out has shape \(3, 12\)"),
        "points and levels swapped": ([(0, 0, "T", MEAN, 0, dev((n, 3)), 0, 3)], {}, r"out has shape \(5, 3\)"),
        "an array of integers": ([(0, 0, "T", MEAN, 0, dev((3, n), "<i4"))], {}, "element type <i4"),
        "an unknown norm": ([(0, 0, "T", MEAN, 0, t3)], dict(norm="area"), "norm 'area'"),
        "a plane of five": ([(0, 0, "T", MEAN, t3)], {}, r"planes\[0\] is \(sched, rec, field, op, grid, out\)"),
        "65 planes": ([(0, 0, "T", MEAN, 0, t3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_records.items():
        with pytest.raises(ValueError, match=msg):
            h.remap_records_dev(planes, **kw)
        assert stub.calls == [], what
    bad_put = {
        "a numpy array": ([("T", 0, np.zeros((1, n)))], {}, "a host array"),
        "an undefined grid": ([("T", 0, t3), ("S", 2, t3)], {}, r"planes\[1\]: grid 2 is not defined"),
        "an output of the step": ([("hmix", 0, one)], {}, r"planes\[0\]: field hmix is an output of the step"),
        "an unknown field": ([("sst", 0, one)], {}, r"planes\[0\]: unknown output field"),
        "levels past the axis": ([("T", 0, t3, 39)], {}, r"planes\[0\]: levels 39 \.\. 41 of field T"),
        "an array of the model's size": ([("T", 0, dev((3, npts)))], {}, r"the array has shape \(3, 12\)"),
        "an unknown op": ([("T", 0, t3)], dict(op="mul"), "op 'mul'"),
        "a NaN skip": ([("T", 0, t3)], dict(skip=float("nan")), "skip is NaN"),
        "S and S_anom at the same levels": ([("S", 0, t3), ("S_anom", 0, one, 2)], {}, r"planes\[1\] and planes\[0\] write S"),
        "a plane of two": ([("T", t3)], {}, r"planes\[0\] is \(field, grid, array\)"),
        "65 planes": ([("T", 0, t3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_put.items():
        with pytest.raises(ValueError, match=msg):
            h.remap_put_dev(planes, **kw)
        assert stub.calls == [], what
    # well-formed calls reach the library with the right tables
    F64, F32 = api.EXP_F64, api.EXP_F32
    h.remap_records_dev([(0, 4, "T", LAST, 0, t3), (0, 4, "hmix", MEAN, 0, f32), (1, 2, "T", MEAN, 0, one, 1, 1)],
                        norm="used", land_value=-1.0)
    h.remap_records_dev([(0, 0, "T", MEAN, 0, f32, 40, 1)], fill_land=False)
    h.remap_put_dev([("T", 0, t3, 38), ("S_anom", 0, f32)], op="add", time_levels=True, skip=1e20, fence=True)
    h.remap_put_dev([("u", 1, dev((2, 7)))])
    names = ["remap_records_dev", "remap_records_dev", "remap_put_dev", "dev_fence", "remap_put_dev"]
    assert [c[0] for c in stub.calls] == [pre + x for x in names]
    fields = STRUCTS["mckpp_remap_record_plane_c"][1]
    tab = stub.calls[0][1]
    assert [tuple(getattr(tab[2][k], f) for f in fields) for k in range(tab[1])] == [
        (0, O["T"], LAST, 0, 3, F64, 0, 1, 1, 4, -1.0, 0x9000000), (0, O["hmix"], MEAN, 0, 1, F32, 0, 1, 1, 4, -1.0, 0x8000000),
        (1, O["T"], MEAN, 1, 1, F64, 0, 1, 1, 2, -1.0, 0x7000000)]
    tab = stub.calls[1][1]
    assert tuple(getattr(tab[2][0], f) for f in fields) == (0, O["T"], MEAN, 40, 1, F32, 0, 0, 0, 0, 1e20, 0x8000000)
    fields = STRUCTS["mckpp_remap_put_plane_c"][1]
    tab = stub.calls[2][1]
    assert [tuple(getattr(tab[2][k], f) for f in fields) for k in range(tab[1])] == [
        (O["T"], 38, 3, F64, api.PUT_ADD, api.PUT_SKIP | api.PUT_TIME_LEVELS, 0, 1e20, 0x9000000),
        (O["S_anom"], 0, 1, F32, api.PUT_ADD, api.PUT_SKIP | api.PUT_TIME_LEVELS, 0, 1e20, 0x8000000)]
    tab = stub.calls[4][1]
    assert tuple(getattr(tab[2][0], f) for f in fields) == (O["u"], 0, 2, F64, api.PUT_SET, 0, 1, 0.0, 0x7000000)
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_remap_bindings(built, tmp_path):
    """A program that uses the two types, the constant and the four interfaces compiles and links against the layer."""
    src = tmp_path / "uses_remap.F90"
    src.write_text("""program uses_remap
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_remap_record_plane_c, mckpp_remap_put_plane_c, MCKPP_OUT_T, MCKPP_EXP_F32, MCKPP_EXP_F64, &
    MCKPP_REMAP_PLANES_MAX, MCKPP_HGRID_NORM_USED, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, mckpp_hip_remap_records_dev, &
    mckpp_hip_remap_put_dev, mckpp_hip_multi_remap_records_dev, mckpp_hip_multi_remap_put_dev
  implicit none
  type(mckpp_remap_record_plane_c) :: recs(1)
  type(mckpp_remap_put_plane_c) :: puts(1)
  integer(c_int) :: rc
  recs(1) = mckpp_remap_record_plane_c(1, MCKPP_OUT_T, 0, 0, 1, MCKPP_EXP_F32, 2, MCKPP_HGRID_NORM_USED, 1, 7_c_int64_t, &
                                       1.0e20_c_double, c_null_ptr)
  puts(1) = mckpp_remap_put_plane_c(MCKPP_OUT_T, 0, 1, MCKPP_EXP_F64, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, 3, 1.0e20_c_double, c_null_ptr)
  if (recs(1)%grid /= 2 .or. recs(1)%rec /= 7 .or. puts(1)%grid /= 3 .or. MCKPP_REMAP_PLANES_MAX /= 64) error stop 1
  if (command_argument_count() > 0) then
    rc = mckpp_hip_remap_records_dev(c_null_ptr, 1, recs, c_null_ptr)
    rc = mckpp_hip_remap_put_dev(c_null_ptr, 1, puts, c_null_ptr)
    rc = mckpp_hip_multi_remap_records_dev(c_null_ptr, 1, recs, c_null_ptr)
    rc = mckpp_hip_multi_remap_put_dev(c_null_ptr, 1, puts, c_null_ptr)
  end if
end program uses_remap
""")
    exe = tmp_path / "uses_remap"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
