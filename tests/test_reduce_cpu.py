"""CPU side of the records reduced over levels and points (include/mckpp_hip_reduce.h): the library exports what the
sixth header declares, api._SIGNATURES_REDUCE states those functions type by type, the plane struct has the C layout,
each multi twin is marked once, the entry points refuse a null handle by their own name, mckpp_host_reduce_tree is the
tree of tests/reduce_ref.py - an order that the test can tell from another -, the Python methods refuse a malformed call
before the library is reached, and the Fortran layer builds with the new interfaces.

(mckpp_hip_reduce_weights' own refusals need a context, which needs a device: they are in tests/test_reduce_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as cm
import reduce_ref as rr
from harness import api, bound_as, null_ctx, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip_reduce.h")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("reduce_weights", "records_reduce_dev", "records_reduce_host")
NAMES = sorted([pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED] + ["mckpp_host_reduce_tree"])
FIELDS = ["sched", "field", "op", "lev0", "nlev", "axis_op", "domain_op", "weighted", "rec", "land_value", "out"]


def test_library_exports_every_function_of_the_reduce_header(api):
    protos = prototypes(HEADER)
    assert sorted(protos) == NAMES
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_reduce.h but not exported"
    assert '#include "mckpp_hip_device_records.h"' in open(HEADER).read()


def test_reduce_signatures_match_the_reduce_header(api):
    protos = prototypes(HEADER)
    table = api._signatures_reduce()
    assert sorted(table) == sorted(protos)
    lib = api._lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert bound_as(ret, restype, returned=True), name
        assert len(argtypes) == len(params), f"{name} takes {len(params)} parameters, {len(argtypes)} bound"
        for i, (p, t) in enumerate(zip(params, argtypes)):
            assert bound_as(p, t), f"{name}: parameter {i} is {p}, bound as {t}"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), f"{name}: _bind left another signature"
    # every handle function has its twin, which is the single form after the handle, and is stated once in the table
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in TWINNED:
        one, multi = "mckpp_hip_" + n, "mckpp_hip_multi_" + n
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % one, src), f"{one} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % multi, src), f"{multi} takes no multi handle"
        assert protos[one][0] == protos[multi][0] and protos[one][1][1:] == protos[multi][1][1:]
        assert api._SIGNATURES_REDUCE[one][2] and multi not in api._SIGNATURES_REDUCE
    assert not api._SIGNATURES_REDUCE["mckpp_host_reduce_tree"][2]
    # no function of this header is in another table
    others = {**api._signatures(), **api._signatures_device(), **api._signatures_zoom(), **api._signatures_records(),
              **api._signatures_put()}
    assert not set(table) & set(others)


def test_reduce_plane_struct_layout_matches_the_header(api, tmp_path):
    assert [f[0] for f in api._ReducePlaneC._fields_] == FIELDS
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(mckpp_reduce_plane_c));']
    body += [f'printf("{f} %zu\\n", offsetof(mckpp_reduce_plane_c, {f}));' for f in FIELDS]
    body += ['printf("%d %d %d %d %d %d %d\\n", MCKPP_RED_NONE, MCKPP_RED_SUM, MCKPP_RED_AVERAGE, MCKPP_RED_MIN, MCKPP_RED_MAX, '
             'MCKPP_RED_W_LEVELS, MCKPP_RED_W_POINTS);', "return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.check_call(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    assert int(out[0]) == C.sizeof(api._ReducePlaneC)
    seen = []
    for line in out[1:1 + len(FIELDS)]:
        name, off = line.split()
        assert getattr(api._ReducePlaneC, name).offset == int(off), name
        seen.append(name)
    assert seen == FIELDS
    assert [int(v) for v in out[1 + len(FIELDS)].split()] == [api.RED_NONE, api.RED_SUM, api.RED_AVERAGE, api.RED_MIN,
                                                              api.RED_MAX, api.RED_W_LEVELS, api.RED_W_POINTS]
    assert (rr.NONE, rr.SUM, rr.AVERAGE, rr.MIN, rr.MAX) == (api.RED_NONE, api.RED_SUM, api.RED_AVERAGE, api.RED_MIN, api.RED_MAX)


def test_entry_points_refuse_a_null_handle_by_their_own_name(api):
    """the sweep of tests/test_entry_cpu.py over the sixth table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_reduce().items():
        if res is not C.c_int or not argtypes or argtypes[0] is not api._H:
            continue
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == [n for n in NAMES if n != "mckpp_host_reduce_tree"]
    planes = (api._ReducePlaneC * 1)()
    for name in swept:
        if "records" in name:   # ... and with a table
            assert getattr(lib, name)(None, 1, planes, *([None] if name.endswith("_dev") else [])) == -1
            assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name


def _mixed(n, seed):
    """n values of mixed sign and of magnitudes over twelve decades"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)


def test_host_reduce_tree_is_the_stated_order(api):
    differs = []
    for n in (0, 1, 2, 3, 255, 256, 257, 1000):
        t = _mixed(n, 100 + n)
        keep = t.copy()
        got = api.host_reduce_tree(t)
        assert np.array_equal(rr.bits(t), rr.bits(keep)), "the terms were changed"
        assert rr.bits(got) == rr.bits(rr.tree(t)), n
        assert rr.bits(rr.staged(t, 64)) == rr.bits(rr.tree(t)), (n, "the staged decomposition with M = 64")
        differs.append(rr.bits(rr.left_to_right(t)) != rr.bits(rr.tree(t)))
    assert rr.bits(api.host_reduce_tree(np.zeros(0))) == rr.bits(0.0)   # +0.0
    assert rr.bits(api.host_reduce_tree(np.array([-0.0]))) == rr.bits(-0.0)   # one term: itself, no padding
    assert any(differs), "the data cannot tell the tree from the left-to-right sum"
    lib = api._lib()
    assert rr.bits(lib.mckpp_host_reduce_tree(None, 5)) == rr.bits(0.0)
    t = _mixed(1000, 7)
    for m in (1, 2, 8, 256, 1024, 4096):
        assert rr.bits(rr.staged(t, m)) == rr.bits(rr.tree(t)), m


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_the_library(api, cls):
    """on an object without a device context whatever reaches the library fails there with "null handle": a malformed
    plane must be a ValueError before that, a well-formed call must get there"""
    h = null_ctx(api, getattr(api, cls))
    npts, nzp1 = 12, 41
    h._npts, h._nzp1 = npts, nzp1
    every = api.WIN_MEAN | api.WIN_MIN | api.WIN_MAX | api.WIN_LAST
    unzoomed = api._Kept({api.OUT["T"]: api.WIN_MIN | api.WIN_LAST, api.OUT["hmix"]: every})
    zoomed = api._Kept({api.OUT["T"]: every})
    zoomed.zoom = (5, 12)
    h._wsched = {0: unzoomed, 2: zoomed}
    dev = FakeDeviceArray
    one, pts, levs, z5, z12 = dev((1,)), dev((npts,)), dev((nzp1,)), dev((5,)), dev((12,))
    bad = {
        "a plane of six": ([(0, 1, "T", 1, one, "sum")], r"planes\[0\] is \(sched, rec, field, op, out, axis_op, domain_op"),
        "a plane of nine": ([(0, 1, "T", 1, one, "sum", "sum", 0, 0)], r"planes\[0\] is \(sched"),
        "both none": ([(0, 1, "T", 1, one, "none", 0)], r"planes\[0\]: axis_op and domain_op are both none"),
        "an unknown reduction": ([(0, 1, "T", 1, one, "mean", "sum")], r"planes\[0\]: reduction 'mean'"),
        "a reduction out of range": ([(0, 1, "T", 1, one, 5, "sum")], r"planes\[0\]: reduction 5"),
        "an unknown weight bit": ([(0, 1, "T", 1, one, "sum", "sum", 4)], r"planes\[0\]: weighted 4"),
        "a field that is not in the schedule": ([(0, 1, "S", 1, one, "sum", "sum")], r"planes\[0\]: field S is not in output schedule 0"),
        "an op the schedule does not keep": ([(0, 1, "T", api.OP_MEAN, one, "sum", "sum")], r"keeps no op 0 of field T"),
        "a negative record": ([(0, -1, "T", 1, one, "sum", "sum")], r"planes\[0\]: record -1"),
        "a level range outside the axis": ([(0, 1, "T", 1, one, "sum", "sum", 0, 1, nzp1)], r"levels 1 \.\. 41 of field T"),
        "a range outside a zoom's levels": ([(2, 1, "T", 1, one, "sum", "sum", 0, 0, 13)], "output schedule 2 keeps 12"),
        "a scalar's array of a profile's size": ([(0, 1, "T", 1, levs, "sum", "sum")], "the call takes 1 elements"),
        "a profile's array of the point axis' size": ([(0, 1, "T", 1, pts, "none", "max")], f"the call takes {nzp1} elements"),
        "an axis-only array sized to the grid for a zoom": ([(2, 1, "T", 1, pts, "min", "none")], "the call takes 5 elements"),
        "a numpy array": ([(0, 1, "T", 1, np.zeros(1), "sum", "sum")], "a host array"),
        "a float array": ([(0, 1, "T", 1, dev((1,), "<f4"), "sum", "sum")], "element type <f4"),
        "a second plane that is wrong": ([(0, 1, "T", 1, one, "sum", "sum"), (0, 1, "T", 1, one, 0, 0)], r"planes\[1\]"),
        "65 planes": ([(0, 1, "T", 1, one, "sum", "sum")] * 65, "65 planes, at most 64"),
    }
    for what, (planes, msg) in bad.items():
        with pytest.raises(ValueError, match=msg):
            h.records_reduce_dev(planes)
    with pytest.raises(ValueError, match="a host array|numpy arrays"):
        h.records_reduce_host([(0, 1, "T", 1, one, "sum", "sum")])
    with pytest.raises(ValueError, match="the call takes 5 elements"):
        h.records_reduce_host([(2, 1, "T", 1, np.zeros(6), "sum", "none")])
    with pytest.raises(ValueError, match="element type <f4"):
        h.records_reduce_host([(2, 1, "T", 1, np.zeros(5, dtype=np.float32), "sum", "none")])
    with pytest.raises(ValueError, match="point_w has shape"):
        h.reduce_weights(point_w=np.ones(npts + 1))
    with pytest.raises(ValueError, match="iface_w has shape"):
        h.reduce_weights(iface_w=np.ones((nzp1, 1)))
    good = [[(0, 1, "T", 1, one, "sum", "average")], [(0, 7, "T", api.OP_LAST, levs, api.RED_NONE, api.RED_MAX, 0)],
            [(2, 1, "T", 2, z5, "average", "none", api.RED_W_LEVELS), (2, 1, "T", 0, z12, "none", "sum", api.RED_W_POINTS)],
            [(0, 1, "hmix", 3, pts, "sum", "none", 0, 0, 1)] * 64]
    for planes in good:
        with pytest.raises(api.MckppHipError, match=r"records_reduce_dev: null handle"):
            h.records_reduce_dev(planes)
    with pytest.raises(api.MckppHipError, match=r"records_reduce_host: null handle"):
        h.records_reduce_host([(2, 1, "T", 1, np.zeros(5), "sum", "none"), (0, 1, "hmix", 0, np.zeros(1), "none", "min")])
    with pytest.raises(api.MckppHipError, match=r"reduce_weights: null handle"):
        h.reduce_weights(np.ones(npts), np.ones(nzp1))


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
    a, b = FakeDeviceArray((2,), ptr=0x7000000), FakeDeviceArray((5,), ptr=0x8000000)
    h.records_reduce_dev([(3, 6, "T", api.OP_LAST, a, "none", "average", api.RED_W_POINTS, 10, 2),
                          (3, 2, "hmix", api.OP_MAX, b, "max", "none")], land_value=-2.0)
    out = np.zeros(1)
    h.records_reduce_host([(3, 0, "T", api.OP_MEAN, out, "sum", "sum", 3)])
    assert [c[0] for c in calls] == ["mckpp_hip_records_reduce_dev", "mckpp_hip_records_reduce_host"]
    n, tab, stream = calls[0][1][1:]
    got = [tuple(getattr(tab[k], f) for f in FIELDS) for k in range(n)]
    assert got == [(3, api.OUT["T"], 3, 10, 2, 0, 2, 2, 6, -2.0, 0x7000000),
                   (3, api.OUT["hmix"], 2, 0, 1, 4, 0, 0, 2, -2.0, 0x8000000)]
    assert stream.value is None
    t = calls[1][1][2][0]
    assert (t.lev0, t.nlev, t.axis_op, t.domain_op, t.weighted, t.rec, t.land_value, t.out) == (0, 12, 1, 1, 3, 0, 1e20, out.ctypes.data)
    assert h._dev_held[-2:] == [a, b] and h._held == {}
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_reduce_bindings(built, tmp_path):
    """A program that uses the new interfaces and the plane type compiles and links against the layer, and the host
    helper gives the tree's sum through it."""
    src = tmp_path / "uses_reduce.F90"
    src.write_text("""program uses_reduce
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_reduce_plane_c, MCKPP_OUT_T, MCKPP_RED_NONE, MCKPP_RED_AVERAGE, MCKPP_RED_W_POINTS, &
    mckpp_hip_reduce_weights, mckpp_hip_records_reduce_dev, mckpp_hip_records_reduce_host, mckpp_host_reduce_tree, &
    mckpp_hip_multi_reduce_weights, mckpp_hip_multi_records_reduce_dev, mckpp_hip_multi_records_reduce_host
  implicit none
  type(mckpp_reduce_plane_c) :: planes(1)
  real(c_double) :: t(3)
  integer(c_int) :: rc
  planes(1) = mckpp_reduce_plane_c(0, MCKPP_OUT_T, 0, 0, 1, MCKPP_RED_NONE, MCKPP_RED_AVERAGE, MCKPP_RED_W_POINTS, &
                                   5_c_int64_t, 1.0e20_c_double, c_null_ptr)
  if (planes(1)%rec /= 5 .or. planes(1)%domain_op /= 2) error stop 1
  t = [1.0_c_double, 2.0_c_double, 4.0_c_double]
  if (mckpp_host_reduce_tree(t, 3_c_int64_t) /= 7.0_c_double) error stop 2
  if (command_argument_count() > 0) then
    rc = mckpp_hip_reduce_weights(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    rc = mckpp_hip_records_reduce_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_records_reduce_host(c_null_ptr, 1_c_int32_t, planes)
    rc = mckpp_hip_multi_reduce_weights(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    rc = mckpp_hip_multi_records_reduce_dev(c_null_ptr, 1_c_int32_t, planes, c_null_ptr)
    rc = mckpp_hip_multi_records_reduce_host(c_null_ptr, 1_c_int32_t, planes)
  end if
end program uses_reduce
""")
    exe = tmp_path / "uses_reduce"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
