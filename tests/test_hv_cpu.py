"""CPU side of a caller grid and a caller axis in one call (include/mckpp_hip_hv.h): the header declares exactly the four
functions and the library exports them and no other of their pattern, api._SIGNATURES_HV states them type by type and
is disjoint from the other nine tables, the two structs have the C layout, both handles have the methods, every entry
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
HEADER = os.path.join(ROOT, "include", "mckpp_hip_hv.h")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("hv_fetch_dev", "hv_put_dev")
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
STRUCTS = {
    "mckpp_hv_plane_c": ("_HvPlaneC", ["field", "axis", "dtype", "grid", "norm", "fill_land", "land_value", "out"]),
    "mckpp_hv_put_plane_c": ("_HvPutPlaneC", ["field", "axis", "dtype", "op", "flags", "grid", "skip_value", "in"]),
}


def test_library_exports_exactly_the_functions_of_the_hv_header(api):
    protos = prototypes(HEADER)
    assert sorted(protos) == NAMES
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_hv.h but not exported"
    text = open(HEADER).read()
    for inc in ("mckpp_hip_remap.h", "mckpp_hip_vaxis.h"):
        assert f'#include "{inc}"' in text
    assert re.search(r"#define\s+MCKPP_HV_PLANES_MAX\s+64\b", text)
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_(?:multi_)?hv_[a-z_0-9]+)\b", syms)))
    assert exported == NAMES     # and no host function: mckpp_host_hgrid_apply and mckpp_host_vaxis_map state the host side


def test_hv_signatures_match_the_hv_header(api):
    protos = prototypes(HEADER)
    table = api._signatures_hv()
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
        assert api._SIGNATURES_HV[one][2] and multi not in api._SIGNATURES_HV
    assert sorted(api._SIGNATURES_HV) == sorted("mckpp_hip_" + n for n in TWINNED)
    # the tenth table: no function of this header in another one
    others = [api._signatures(), api._signatures_device(), api._signatures_zoom(), api._signatures_records(),
              api._signatures_put(), api._signatures_reduce(), api._signatures_vaxis(), api._signatures_hgrid(),
              api._signatures_remap()]
    assert len(others) == 9 and not any(set(table) & set(o) for o in others)


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
        assert issubclass(cls, api._GridAxis)
        for n in TWINNED:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over this table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_hv().items():
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
    h.vaxis_define(0, [0.0, -10.0, -50.0])
    h.vaxis_define(2, [-1.0, -2.0])
    del stub.calls[:]
    dev = FakeDeviceArray
    t3, f32, two7 = dev((3, n), ptr=0x9000000), dev((3, n), "<f4", ptr=0x8000000), dev((2, 7))
    bad_fetch = {
        "a numpy array": ([("T", 0, 0, np.zeros((3, n)))], {}, "a host array"),
        "an undefined grid": ([("T", 0, 0, t3), ("T", 3, 0, t3)], {}, r"planes\[1\]: grid 3 is not defined"),
        "an undefined axis": ([("T", 0, 1, t3)], {}, r"planes\[0\]: axis 1 is not defined"),
        "a two-dimensional field": ([("hmix", 0, 0, t3)], {}, r"planes\[0\]: field hmix is two-dimensional"),
        "an interface field": ([("T", 0, 0, t3), ("wu", 0, 0, t3)], {}, r"planes\[1\]: field wu lives on the interface axis"),
        "an unknown field": ([("sst", 0, 0, t3)], {}, r"planes\[0\]: unknown output field"),
        "an array of the model's size": ([("T", 0, 0, dev((3, npts)))], {}, r"out has shape \(3, 12\)"),
        "points and levels swapped": ([("T", 0, 0, dev((n, 3)))], {}, r"out has shape \(5, 3\)"),
        "another axis' levels": ([("T", 0, 2, t3)], {}, r"out has shape \(3, 5\); axis 2 on grid 0 is \(2, 5\)"),
        "an array of integers": ([("T", 0, 0, dev((3, n), "<i4"))], {}, "element type <i4"),
        "an unknown norm": ([("T", 0, 0, t3)], dict(norm="area"), "norm 'area'"),
        "a plane of three": ([("T", 0, t3)], {}, r"planes\[0\] is \(field, grid, axis, out\)"),
        "65 planes": ([("T", 0, 0, t3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_fetch.items():
        with pytest.raises(ValueError, match=msg):
            h.hv_fetch_dev(planes, **kw)
        assert stub.calls == [], what
    bad_put = {
        "a numpy array": ([("T", 0, 0, np.zeros((3, n)))], {}, "a host array"),
        "an undefined grid": ([("T", 0, 0, t3), ("S", 2, 0, t3)], {}, r"planes\[1\]: grid 2 is not defined"),
        "an undefined axis": ([("T", 0, 5, t3)], {}, r"planes\[0\]: axis 5 is not defined"),
        "an output of the step": ([("rho", 0, 0, t3)], {}, r"planes\[0\]: field rho is an output of the step"),
        "an unknown field": ([("sst", 0, 0, t3)], {}, r"planes\[0\]: unknown output field"),
        "an array of the model's size": ([("T", 0, 0, dev((3, npts)))], {}, r"the array has shape \(3, 12\)"),
        "an unknown op": ([("T", 0, 0, t3)], dict(op="mul"), "op 'mul'"),
        "a NaN skip": ([("T", 0, 0, t3)], dict(skip=float("nan")), "skip is NaN"),
        "S and S_anom": ([("S", 0, 0, t3), ("u", 0, 0, t3), ("S_anom", 1, 2, two7)], {}, r"planes\[2\] and planes\[0\] write S"),
        "a plane of three": ([("T", 0, t3)], {}, r"planes\[0\] is \(field, grid, axis, array\)"),
        "65 planes": ([("T", 0, 0, t3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_put.items():
        with pytest.raises(ValueError, match=msg):
            h.hv_put_dev(planes, **kw)
        assert stub.calls == [], what
    # well-formed calls reach the library with the right tables
    F64, F32, O = api.EXP_F64, api.EXP_F32, api.OUT
    h.hv_fetch_dev([("T", 0, 0, t3), ("rho", 0, 0, f32)], norm="used", land_value=-1.0)
    h.hv_fetch_dev([("S", 1, 2, two7)], fill_land=False)
    h.hv_put_dev([("T", 0, 0, t3), ("S_anom", 0, 0, f32)], op="add", time_levels=True, skip=1e20, fence=True)
    h.hv_put_dev([("u", 1, 2, two7)])
    names = ["hv_fetch_dev", "hv_fetch_dev", "hv_put_dev", "dev_fence", "hv_put_dev"]
    assert [c[0] for c in stub.calls] == [pre + x for x in names]
    fields = STRUCTS["mckpp_hv_plane_c"][1]
    tab = stub.calls[0][1]
    assert [tuple(getattr(tab[2][k], f) for f in fields) for k in range(tab[1])] == [
        (O["T"], 0, F64, 0, 1, 1, -1.0, 0x9000000), (O["rho"], 0, F32, 0, 1, 1, -1.0, 0x8000000)]
    tab = stub.calls[1][1]
    assert tuple(getattr(tab[2][0], f) for f in fields) == (O["S"], 2, F64, 1, 0, 0, 1e20, 0x7000000)
    fields = STRUCTS["mckpp_hv_put_plane_c"][1]
    tab = stub.calls[2][1]
    assert [tuple(getattr(tab[2][k], f) for f in fields) for k in range(tab[1])] == [
        (O["T"], 0, F64, api.PUT_ADD, api.PUT_SKIP | api.PUT_TIME_LEVELS, 0, 1e20, 0x9000000),
        (O["S_anom"], 0, F32, api.PUT_ADD, api.PUT_SKIP | api.PUT_TIME_LEVELS, 0, 1e20, 0x8000000)]
    tab = stub.calls[4][1]
    assert tuple(getattr(tab[2][0], f) for f in fields) == (O["u"], 2, F64, api.PUT_SET, 0, 1, 0.0, 0x7000000)
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_hv_bindings(built, tmp_path):
    """A program that uses the two types, the constant and the four interfaces compiles and links against the layer."""
    src = tmp_path / "uses_hv.F90"
    src.write_text("""program uses_hv
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hv_plane_c, mckpp_hv_put_plane_c, MCKPP_OUT_T, MCKPP_EXP_F32, MCKPP_EXP_F64, &
    MCKPP_HV_PLANES_MAX, MCKPP_HGRID_NORM_USED, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, mckpp_hip_hv_fetch_dev, &
    mckpp_hip_hv_put_dev, mckpp_hip_multi_hv_fetch_dev, mckpp_hip_multi_hv_put_dev
  implicit none
  type(mckpp_hv_plane_c) :: outs(1)
  type(mckpp_hv_put_plane_c) :: puts(1)
  integer(c_int) :: rc
  outs(1) = mckpp_hv_plane_c(MCKPP_OUT_T, 5, MCKPP_EXP_F32, 2, MCKPP_HGRID_NORM_USED, 1, 1.0e20_c_double, c_null_ptr)
  puts(1) = mckpp_hv_put_plane_c(MCKPP_OUT_T, 6, MCKPP_EXP_F64, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, 3, 1.0e20_c_double, c_null_ptr)
  if (outs(1)%grid /= 2 .or. outs(1)%axis /= 5 .or. puts(1)%grid /= 3 .or. puts(1)%axis /= 6) error stop 1
  if (MCKPP_HV_PLANES_MAX /= 64) error stop 2
  if (command_argument_count() > 0) then
    rc = mckpp_hip_hv_fetch_dev(c_null_ptr, 1, outs, c_null_ptr)
    rc = mckpp_hip_hv_put_dev(c_null_ptr, 1, puts, c_null_ptr)
    rc = mckpp_hip_multi_hv_fetch_dev(c_null_ptr, 1, outs, c_null_ptr)
    rc = mckpp_hip_multi_hv_put_dev(c_null_ptr, 1, puts, c_null_ptr)
  end if
end program uses_hv
""")
    exe = tmp_path / "uses_hv"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
