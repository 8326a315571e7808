"""CPU side of the device-array interface (include/mckpp_hip_device.h): the library exports what the companion header
declares, api._SIGNATURES_DEVICE states those functions type by type (and api._signatures() still describes mckpp_hip.h
alone), the plane struct has the C layout, the Python methods refuse a malformed call before the library is reached, and
the Fortran layer builds with the new interfaces.  The header parser and the binding rules are those of
tests/test_abi_cpu.py, re-stated here for the companion header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
from harness import api, bound_as, prototypes  # noqa: F401

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip.h")
DEVICE_HEADER = os.path.join(ROOT, "include", "mckpp_hip_device.h")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
NEW = ("fluxes_dev", "flux_ring_put_dev", "fetch_dev", "dev_fence")


def test_library_exports_every_function_of_the_companion_header(api):
    protos = prototypes(DEVICE_HEADER)
    assert sorted(protos) == sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in NEW)
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_device.h but not exported"


def test_device_signatures_match_the_companion_header(api):
    protos = prototypes(DEVICE_HEADER)
    table = api._signatures_device()
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
    src = re.sub(r"/\*.*?\*/", "", open(DEVICE_HEADER).read(), flags=re.S)
    for n in NEW:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_DEVICE[one][2] and multi not in api._SIGNATURES_DEVICE


def test_the_first_table_still_describes_the_first_header(api):
    protos = prototypes(HEADER)
    assert sorted(api._signatures()) == sorted(protos)
    assert not set(api._signatures()) & set(api._signatures_device())
    assert not set(prototypes(DEVICE_HEADER)) & set(protos), "a device-array function declared in mckpp_hip.h"


def test_plane_struct_layout_matches_the_header(api, tmp_path):
    fields = [f[0] for f in api._DevPlaneC._fields_]
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{DEVICE_HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_dev_plane_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_dev_plane_c, {f}));' for f in fields]
    body.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._DevPlaneC)
    seen = []
    for line in filter(None, out[1:]):
        name, off = line.split()
        assert getattr(api._DevPlaneC, name).offset == int(off), name
        seen.append(name)
    assert seen == ["field", "lev0", "nlev", "dtype", "fill_land", "land_value", "out"]


def test_new_entry_points_refuse_a_null_handle(api):
    lib = api._lib()
    ptrs, planes = (C.c_void_p * 8)(), (api._DevPlaneC * 1)()
    for pre in ("mckpp_hip_", "mckpp_hip_multi_"):
        calls = {
            "fluxes_dev": lambda f: f(None, 1, ptrs, 0, 1.0, 1.0, None),
            "flux_ring_put_dev": lambda f: f(None, 0, ptrs, None),
            "fetch_dev": lambda f: f(None, 1, planes, None),
            "dev_fence": lambda f: f(None, None),
        }
        for name, call in calls.items():
            assert call(getattr(lib, pre + name)) < 0, pre + name
            assert (pre + name + ": null handle").encode() in lib.mckpp_hip_last_error(), lib.mckpp_hip_last_error()


class FakeDeviceArray:
    """What the Python layer sees of an array in device memory: __cuda_array_interface__ (version 2 keys)"""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=0x7000000):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 2}


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_any_library_call(api, cls, monkeypatch):
    import torch

    calls = []

    class Stub:
        """a library whose entry points all succeed"""

        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 0
            return entry

    monkeypatch.setattr(api, "_lib", lambda: Stub())
    npts, nzp1 = 12, 41
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    dev = FakeDeviceArray
    good = [dev((npts,), ptr=0x7000000 + 0x1000 * m) for m in range(8)]
    refused = {
        "a numpy array": ([np.zeros(npts)] * 8, "a host array"),
        "one numpy array of (8, npts)": (np.zeros((8, npts)), "a host array"),
        "a torch tensor in host memory": ([torch.zeros(npts, dtype=torch.float64)] * 8, "a host array"),
        "seven fields": (good[:7], "7 fields"),
        "a wrong dtype": (good[:3] + [dev((npts,), "<f4")] + good[4:], r"fields\[3\]: element type <f4"),
        "a non-contiguous array": (good[:5] + [dev((npts,), strides=(16,))] + good[6:], r"fields\[5\]: not C-contiguous"),
        "a wrong size": (good[:7] + [dev((npts + 1,))], r"fields\[7\]: shape \(13,\), the call takes 12 elements"),
        "one array of (8, npts + 1)": (dev((8, npts + 1)), "the call takes 96 elements"),
    }
    for what, (fields, msg) in refused.items():
        with pytest.raises(ValueError, match=msg):
            h.fluxes_dev(1, fields)
        with pytest.raises(ValueError, match=msg):
            h.flux_ring_put_dev(0, fields)
        assert calls == [], what
    out3, out1 = dev((nzp1, npts)), dev((npts,))
    planes = {
        "a level range outside the axis": ([("T", out3, 1, nzp1)], r"levels 1 \.\. 41 of field T, whose axis has 41"),
        "a range of a two-dimensional field": ([("hmix", dev((2, npts)), 0, 2)], "of field hmix, whose axis has 1"),
        "no level": ([("T", out1, 0, 0)], "whose axis has 41"),
        "a negative first level": ([("T", out1, -1, 1)], "whose axis has 41"),
        "more levels than the axis, from the array": ([("u", dev((nzp1 + 1, npts)))], "whose axis has 41"),
        "a numpy array": ([("T", np.zeros(npts), 0, 1)], "a host array"),
        "an integer array": ([("T", dev((npts,), "<i8"), 0, 1)], "element type <i8"),
        "an array of another size": ([("T", dev((nzp1, npts)), 0, 2)], "the call takes 24 elements"),
        "a non-contiguous array": ([("T", dev((2, npts), strides=(8, 16)), 0, 2)], "not C-contiguous"),
        "an unknown field": ([("sst", out1, 0, 1)], "unknown output field"),
        "a second plane that is wrong": ([("T", out1, 0, 1), ("v", out1, 41, 1)], r"planes\[1\]"),
    }
    for what, (p, msg) in planes.items():
        with pytest.raises(ValueError, match=msg):
            h.fetch_dev(p)
        assert calls == [], what
    with pytest.raises(ValueError, match="stream"):
        h.dev_fence(stream="0")
    assert calls == []
    # well-formed calls reach the library: the addresses, the plane table and the null stream as they should be
    h.fluxes_dev(3, good, l_rest=1, fence=True)
    h.flux_ring_put_dev(5, dev((8, npts), ptr=0x9000000))
    h.fetch_dev([("T", out1, 0, 1), ("S", dev((nzp1, npts), "<f4", ptr=0xa000000)), ("hmix", out1)], land_value=-2.0)
    h.fetch_dev([("u", out3, 0, nzp1)], fill_land=False)
    pre = h._pre
    assert [c[0] for c in calls] == [pre + n for n in ("fluxes_dev", "dev_fence", "flux_ring_put_dev", "fetch_dev", "fetch_dev")]
    a = calls[0][1]
    assert (a[1], a[3], a[4], a[5]) == (3, 1, 334000.0, 2.5e6) and a[6].value is None
    assert [a[2][m] for m in range(8)] == [0x7000000 + 0x1000 * m for m in range(8)]
    assert [calls[2][1][2][m] for m in range(8)] == [0x9000000 + 8 * npts * m for m in range(8)]
    n, tab = calls[3][1][1], calls[3][1][2]
    got = [(tab[k].field, tab[k].lev0, tab[k].nlev, tab[k].dtype, tab[k].fill_land, tab[k].land_value, tab[k].out)
           for k in range(n)]
    assert got == [(api.OUT["T"], 0, 1, api.EXP_F64, 1, -2.0, 0x7000000), (api.OUT["S"], 0, nzp1, api.EXP_F32, 1, -2.0, 0xa000000),
                   (api.OUT["hmix"], 0, 1, api.EXP_F64, 1, -2.0, 0x7000000)]
    assert calls[4][1][2][0].fill_land == 0 and calls[4][1][2][0].nlev == nzp1
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_device_array_bindings(built, tmp_path):
    """A program that uses the eight new interfaces and the plane type compiles and links against the layer."""
    src = tmp_path / "uses_dev.F90"
    src.write_text("""program uses_dev
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_dev_plane_c, MCKPP_OUT_T, MCKPP_EXP_F64, &
    mckpp_hip_fluxes_dev, mckpp_hip_flux_ring_put_dev, mckpp_hip_fetch_dev, mckpp_hip_dev_fence, &
    mckpp_hip_multi_fluxes_dev, mckpp_hip_multi_flux_ring_put_dev, mckpp_hip_multi_fetch_dev, mckpp_hip_multi_dev_fence
  implicit none
  type(c_ptr) :: fields(8)
  type(mckpp_dev_plane_c) :: planes(1)
  integer(c_int) :: rc
  fields = c_null_ptr
  planes(1) = mckpp_dev_plane_c(MCKPP_OUT_T, 0, 1, MCKPP_EXP_F64, 1, 1.0e20_c_double, c_null_ptr)
  if (command_argument_count() > 0) then
    rc = mckpp_hip_fluxes_dev(c_null_ptr, 1_c_int, fields, 0_c_int, 334000.0_c_double, 2.5e6_c_double, c_null_ptr)
    rc = mckpp_hip_flux_ring_put_dev(c_null_ptr, 0_c_int, fields, c_null_ptr)
    rc = mckpp_hip_fetch_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_dev_fence(c_null_ptr, c_null_ptr)
    rc = mckpp_hip_multi_fluxes_dev(c_null_ptr, 1_c_int, fields, 0_c_int, 334000.0_c_double, 2.5e6_c_double, c_null_ptr)
    rc = mckpp_hip_multi_flux_ring_put_dev(c_null_ptr, 0_c_int, fields, c_null_ptr)
    rc = mckpp_hip_multi_fetch_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_multi_dev_fence(c_null_ptr, c_null_ptr)
  end if
end program uses_dev
""")
    exe = tmp_path / "uses_dev"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip", "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
