"""CPU side of the state set or incremented in place (include/mckpp_hip_put.h): the library exports what the fifth
header declares, api._SIGNATURES_PUT states those functions type by type (the other four tables still describe their own
headers), the plane struct has the C layout, every entry point refuses a null handle by its own name, the Python methods
refuse a malformed call before the library is reached and hand a well-formed one over as the right table, and the
Fortran layer builds with the new type and interfaces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, bound_as, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADERS = {n: os.path.join(ROOT, "include", f) for n, f in (
    ("first", "mckpp_hip.h"), ("device", "mckpp_hip_device.h"), ("zoom", "mckpp_hip_zoom.h"),
    ("records", "mckpp_hip_device_records.h"), ("put", "mckpp_hip_put.h"))}
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("put_dev", "put_host")
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
STRUCT_FIELDS = ["field", "lev0", "nlev", "dtype", "op", "flags", "skip_value", "in"]


def test_library_exports_exactly_the_functions_of_the_put_header(api):
    protos = prototypes(HEADERS["put"])
    assert sorted(protos) == NAMES
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_put.h but not exported"
    src = open(HEADERS["put"]).read()
    assert '#include "mckpp_hip_device.h"' in src
    # ... and nothing of this name that the header does not declare
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_hip_(?:multi_)?put_[a-z_0-9]+)\b", syms)))
    assert exported == NAMES


def test_put_signatures_match_the_put_header(api):
    protos = prototypes(HEADERS["put"])
    table = api._signatures_put()
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
    src = re.sub(r"/\*.*?\*/", "", open(HEADERS["put"]).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_PUT[one][2] and multi not in api._SIGNATURES_PUT
    # the constants of the header are the Python layer's
    for name, value in re.findall(r"\b(MCKPP_PUT_[A-Z_]+)\s*=\s*(\d+)", src):
        assert getattr(api, name[len("MCKPP_"):]) == int(value), name
    assert re.search(r"#define\s+MCKPP_PUT_PLANES_MAX\s+64\b", src)


def test_the_other_four_tables_still_describe_their_headers(api):
    protos = {n: prototypes(h) for n, h in HEADERS.items()}
    tables = {"first": api._signatures(), "device": api._signatures_device(), "zoom": api._signatures_zoom(),
              "records": api._signatures_records(), "put": api._signatures_put()}
    for n in HEADERS:
        assert sorted(tables[n]) == sorted(protos[n]), n
        for other in HEADERS:
            if other != n:
                assert not set(protos[n]) & set(protos[other]), f"a function declared in both the {n} and the {other} header"
                assert not set(tables[n]) & set(tables[other])


def test_put_plane_struct_layout_matches_the_header(api, tmp_path):
    fields = [f[0] for f in api._PutPlaneC._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADERS["put"]}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_put_plane_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_put_plane_c, {f}));' for f in fields]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._PutPlaneC)
    seen = []
    for line in filter(None, out[1:]):
        name, off = line.split()
        assert getattr(api._PutPlaneC, name).offset == int(off), name
        seen.append(name)
    assert seen == STRUCT_FIELDS


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over the fifth table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_put().items():
        assert res is C.c_int and argtypes[0] is api._H, name
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES
    planes = (api._PutPlaneC * 1)()
    for name in NAMES:   # ... and with a table
        args = (None, 1, planes, None) if name.endswith("_dev") else (None, 1, planes)
        assert getattr(lib, name)(*args) == -1
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name


class _Stub:
    """a library whose entry points all succeed, and which keeps what they were called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _table(args):
    n, tab = args[1], args[2]
    return [tuple(getattr(tab[k], f) for f in STRUCT_FIELDS) for k in range(n)]


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_any_library_call(api, cls, monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(api, "_lib", lambda: stub)
    npts, nzp1 = 12, 41
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    dev = FakeDeviceArray
    d3, d1, d5 = dev((nzp1, npts)), dev((npts,)), dev((5, npts), "<f4", ptr=0x8000000)
    n3, n1 = np.zeros((nzp1, npts)), np.zeros(npts, dtype=np.float32)
    nan = float("nan")
    # (planes, keywords, message): refused by put_dev with device arrays ...
    bad_dev = {
        "a numpy array": ([("T", n3)], {}, "a host array"),
        "an integer array": ([("T", dev((npts,), "<i8"))], {}, "element type <i8"),
        "a non-contiguous array": ([("T", dev((2, npts), strides=(8, 16)), 0, 2)], {}, "not C-contiguous"),
        "an array of another size": ([("T", d3, 0, 2)], {}, "the call takes 24 elements"),
        "a level range outside the axis": ([("T", d3, 1, nzp1)], {}, r"planes\[0\]: levels 1 \.\. 41 of field T, whose axis has 41"),
        "a first level past what the array adds": ([("u", d5, 37)], {}, r"levels 37 \.\. 41 of field u"),
        "no level": ([("T", d1, 0, 0)], {}, "whose axis has 41"),
        "a negative first level": ([("v", d1, -1, 1)], {}, "whose axis has 41"),
        "more levels than the axis, from the array": ([("S", dev((nzp1 + 1, npts)))], {}, "whose axis has 41"),
        "an unknown field": ([("sst", d1)], {}, r"planes\[0\]: unknown output field"),
        "hmix": ([("hmix", d1)], {}, r"planes\[0\]: field hmix is an output of the step, not state"),
        "rho": ([("T", d1), ("rho", d3)], {}, r"planes\[1\]: field rho is an output of the step, not state"),
        "a field number that is no state": ([(api.OUT["difm"], d3)], {}, "field difm is an output of the step"),
        "overlapping planes": ([("T", d3), ("u", d1), ("T", d5, 36)], {}, r"planes\[2\] and planes\[0\] write T at overlapping levels 36 \.\. 40 and 0 \.\. 40"),
        "S over S_anom": ([("S_anom", d5, 3), ("S", d1, 7)], {}, r"planes\[1\] and planes\[0\] write S at overlapping levels"),
        "a NaN skip value": ([("T", d1)], dict(skip=nan), "skip is NaN"),
        "an unknown op": ([("T", d1)], dict(op="mul"), "op 'mul'"),
        "a plane of one": ([("T",)], {}, r"planes\[0\] is \(field, array\)"),
        "a plane of five": ([("T", d1, 0, 1, 0)], {}, r"planes\[0\] is \(field, array\)"),
        "65 planes": ([("T", d1)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_dev.items():
        with pytest.raises(ValueError, match=msg):
            h.put_dev(planes, **kw)
        assert stub.calls == [], what
    with pytest.raises(ValueError, match="stream"):
        h.put_dev([("T", d1)], stream="0")
    assert stub.calls == []
    # ... and by put_host with numpy arrays
    bad_host = {
        "a device array": ([("T", d3)], {}, "an array in device memory"),
        "a list": ([("T", [0.0] * npts, 0, 1)], {}, "no numpy array"),
        "an integer array": ([("T", np.zeros(npts, dtype=np.int64))], {}, "element type <i8"),
        "a Fortran-ordered array": ([("T", np.zeros((2, npts), order="F"))], {}, "not C-contiguous"),
        "an array of another size": ([("T", n3, 0, 2)], {}, "the call takes 24 elements"),
        "rho": ([("rho", n3)], {}, "field rho is an output of the step, not state"),
        "overlapping planes": ([("v", n3), ("v", n1, 40)], {}, r"planes\[1\] and planes\[0\] write v at overlapping levels 40 \.\. 40 and 0 \.\. 40"),
        "a NaN skip value": ([("T", n1)], dict(skip=np.float64("nan")), "skip is NaN"),
        "a level range outside the axis": ([("T", n1, 41)], {}, r"levels 41 \.\. 41 of field T"),
    }
    for what, (planes, kw, msg) in bad_host.items():
        with pytest.raises(ValueError, match=msg):
            h.put_host(planes, **kw)
        assert stub.calls == [], what
    # well-formed calls reach the library with the right table
    F64, F32, O = api.EXP_F64, api.EXP_F32, api.OUT
    h.put_dev([("T", d3), ("S", d5, 36), ("u", d1)])
    h.put_dev([("S_anom", d5, 2, 5), ("S", d1, 7)], op="add", time_levels=True, skip=1e20, fence=True)
    h.put_host([("v", n3), ("T", n1, 40, 1)], op=api.PUT_ADD, skip=0.0)
    h.put_host([(O["T"], n1)], time_levels=True)
    h.put_dev([])
    pre = h._pre
    assert [c[0] for c in stub.calls] == [pre + n for n in ("put_dev", "put_dev", "dev_fence", "put_host", "put_host", "put_dev")]
    a = stub.calls[0][1]
    assert _table(a) == [(O["T"], 0, nzp1, F64, 0, 0, 0.0, 0x7000000), (O["S"], 36, 5, F32, 0, 0, 0.0, 0x8000000),
                         (O["u"], 0, 1, F64, 0, 0, 0.0, 0x7000000)]
    assert a[3].value is None and len(a) == 4
    assert _table(stub.calls[1][1]) == [(O["S_anom"], 2, 5, F32, 1, 3, 1e20, 0x8000000), (O["S"], 7, 1, F64, 1, 3, 1e20, 0x7000000)]
    b = stub.calls[3][1]
    assert _table(b) == [(O["v"], 0, nzp1, F64, 1, 1, 0.0, n3.ctypes.data), (O["T"], 40, 1, F32, 1, 1, 0.0, n1.ctypes.data)]
    assert len(b) == 3
    assert _table(stub.calls[4][1]) == [(O["T"], 0, 1, F32, 0, 2, 0.0, n1.ctypes.data)]
    assert stub.calls[5][1][1] == 0
    assert h._held == {} and d3 in h._dev_held   # device arrays kept the way fetch_dev keeps them, host arrays not at all
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_put_bindings(built, tmp_path):
    """A program that uses the plane type, the constants and the four interfaces compiles and links against the layer."""
    src = tmp_path / "uses_put.F90"
    src.write_text("""program uses_put
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_put_plane_c, MCKPP_OUT_T, MCKPP_OUT_S, MCKPP_EXP_F64, MCKPP_EXP_F32, &
    MCKPP_PUT_SET, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, MCKPP_PUT_TIME_LEVELS, MCKPP_PUT_PLANES_MAX, &
    mckpp_hip_put_dev, mckpp_hip_put_host, mckpp_hip_multi_put_dev, mckpp_hip_multi_put_host
  implicit none
  type(mckpp_put_plane_c) :: planes(2)
  integer(c_int) :: rc
  planes(1) = mckpp_put_plane_c(MCKPP_OUT_T, 0, 1, MCKPP_EXP_F64, MCKPP_PUT_ADD, MCKPP_PUT_SKIP, 1.0e20_c_double, c_null_ptr)
  planes(2) = mckpp_put_plane_c(MCKPP_OUT_S, 0, 41, MCKPP_EXP_F32, MCKPP_PUT_SET, &
                                ior(MCKPP_PUT_SKIP, MCKPP_PUT_TIME_LEVELS), 0.0_c_double, c_null_ptr)
  if (planes(2)%flags /= 3 .or. planes(1)%op /= 1 .or. MCKPP_PUT_PLANES_MAX /= 64) error stop 1
  if (command_argument_count() > 0) then
    rc = mckpp_hip_put_dev(c_null_ptr, 2_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_put_host(c_null_ptr, 2_c_int32_t, planes)
    rc = mckpp_hip_multi_put_dev(c_null_ptr, 2_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_multi_put_host(c_null_ptr, 2_c_int32_t, planes)
  end if
end program uses_put
""")
    exe = tmp_path / "uses_put"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
