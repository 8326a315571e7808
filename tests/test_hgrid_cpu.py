"""CPU side of the caller's horizontal grids (include/mckpp_hip_hgrid.h): the library exports what the header declares
and nothing else of those names, api._SIGNATURES_HGRID states those functions type by type, the two structs have the C
layout, both handles have the methods and every entry point refuses a null handle by its own name, the Python methods
refuse a malformed call before the library is reached, the Fortran layer builds with the new types and interfaces - and
the three host functions, the part of the feature that needs no GPU: mckpp_host_hgrid_check's refusals name table, row
and entry, mckpp_host_hgrid_apply is tests/hgrid_ref.py's restatement of the header bit for bit, and
mckpp_host_hgrid_slices puts every entry at the address the header states; from the library and from a stand-alone
program built under the address and undefined-behaviour sanitizers."""
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
from harness import api, bound_as, prototypes  # noqa: F401
from test_device_arrays_cpu import FakeDeviceArray

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip_hgrid.h")
CSRC = os.path.join(ROOT, "mckpp_f90_amd", "csrc")
FDIR = os.path.join(ROOT, "mckpp_f90_amd", "fortran")
FC = "/opt/rocm/bin/amdflang"
TWINNED = ("hgrid_define", "hgrid_info", "hgrid_fluxes_dev", "hgrid_flux_ring_put_dev", "hgrid_fetch_dev")
NAMES = sorted(pre + n for pre in ("mckpp_hip_", "mckpp_hip_multi_") for n in TWINNED)
HOST_NAMES = ["mckpp_host_hgrid_apply", "mckpp_host_hgrid_check", "mckpp_host_hgrid_slices"]
STRUCTS = {
    "mckpp_hgrid_table_c": ("_HgridTableC", ["ptr", "idx", "w"]),
    "mckpp_hgrid_plane_c": ("_HgridPlaneC", ["field", "lev0", "nlev", "dtype", "grid", "norm", "fill_land", "land_value", "out"]),
}
TAGS = ("every_step_nz40", "sweep_nd3")      # the cases tests/test_hgrid_gpu.py runs on


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _tables():
    """(what, table, nrows, nsrc, ocean mask over the source or None): the tables of the GPU tests, both directions"""
    for tag in TAGS:
        case = lc.CASES[tag]
        npts, ocean = case.ncol, lc.ocean(case)
        for g, n in enumerate(hr.grids(npts)):
            yield f"{tag} grid {g} in", hr.general_in(npts, n, ocean, 7 + g), npts, n, None
            yield f"{tag} grid {g} out", hr.general_out(n, npts, ocean, 17 + g), n, npts, ocean


# ---------------------------------------------------------------------------
# header, table, structs, handles
# ---------------------------------------------------------------------------
def test_library_exports_exactly_the_functions_of_the_hgrid_header(api):
    protos = prototypes(HEADER)
    assert sorted(protos) == sorted(NAMES + HOST_NAMES)
    lib = api._lib()
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in mckpp_hip_hgrid.h but not exported"
    assert '#include "mckpp_hip_device.h"' in open(HEADER).read()
    so = os.path.join(ROOT, "mckpp_f90_amd", "libmckpp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_(?:multi_)?hgrid_[a-z_0-9]+)\b", syms)))
    assert exported == sorted(NAMES + HOST_NAMES)


def test_hgrid_signatures_match_the_hgrid_header(api):
    protos = prototypes(HEADER)
    table = api._signatures_hgrid()
    assert sorted(table) == sorted(protos)
    lib = api._lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        if name == "mckpp_host_hgrid_slices":
            assert ret == "int64_t" and restype is C.c_int64
        else:
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
        assert api._SIGNATURES_HGRID[one][2] and multi not in api._SIGNATURES_HGRID
    for n in HOST_NAMES:
        assert not api._SIGNATURES_HGRID[n][2]
    # no function of this header in another table
    others = [api._signatures(), api._signatures_device(), api._signatures_zoom(), api._signatures_records(),
              api._signatures_put(), api._signatures_reduce(), api._signatures_vaxis()]
    assert not any(set(table) & set(o) for o in others)
    # the constants of the header are the Python layer's
    for name, value in re.findall(r"\b(MCKPP_HGRID_NORM_[A-Z]+)\s*=\s*(\d+)", src):
        assert getattr(api, name[len("MCKPP_"):]) == int(value), name
    full = open(HEADER).read()
    assert re.search(r"#define\s+MCKPP_HGRIDS\s+4\b", full) and api.HGRIDS == 4
    assert re.search(r"#define\s+MCKPP_HGRID_PLANES_MAX\s+64\b", full)


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
    for n in ("host_hgrid_check", "host_hgrid_apply", "host_hgrid_slices"):
        assert callable(getattr(api, n))


def test_every_entry_point_refuses_a_null_handle_by_its_own_name(api):
    """the sweep of tests/test_entry_cpu.py over this table"""
    from test_entry_cpu import null_for

    lib = api._lib()
    swept = []
    for name, (res, argtypes) in api._signatures_hgrid().items():
        if name in HOST_NAMES:
            continue
        assert res is C.c_int and argtypes[0] is api._H, name
        lib.mckpp_hip_step(None, 0, -1)   # whatever the call leaves is its own
        assert getattr(lib, name)(None, *[null_for(t) for t in argtypes[1:]]) == -1, name
        assert lib.mckpp_hip_last_error() == (name + ": null handle").encode(), name
        swept.append(name)
    assert sorted(swept) == NAMES


# ---------------------------------------------------------------------------
# the host functions, without a GPU
# ---------------------------------------------------------------------------
def test_the_tables_reach_what_they_are_built_for():
    for tag in TAGS:
        case = lc.CASES[tag]
        npts, ocean = case.ncol, lc.ocean(case)
        small, big = hr.grids(npts)
        assert small == 37 < 64 and big % 64 and 1.25 * npts < big < 1.4 * npts
        for g, n in enumerate((small, big)):
            tin, tout = hr.general_in(npts, n, ocean, 7 + g), hr.general_out(n, npts, ocean, 17 + g)
            lin, lout = np.diff(tin[0]), np.diff(tout[0])
            assert set(lin) <= set(hr.LENGTHS) and set(lout) <= set(hr.LENGTHS)
            assert (lin[ocean != 0] > 0).all(), "an ocean point with an empty in row"
            if npts > 64:
                assert set(lin) == set(hr.LENGTHS) and set(lout) == set(hr.LENGTHS)
            assert lin[1] == 70 and lin[:8].max() == 70 and sorted(lin[:8])[-2] <= 4      # 70 next to short rows, one slice
            assert lout[1] == 70 and sorted(lout[:8])[-2] <= 4
            assert (tin[2] < 0).any() and (tout[2] < 0).any()                            # negative weights
            assert any(len(set(tin[1][tin[0][r]:tin[0][r + 1]])) < lin[r] for r in range(npts))   # repeated indices
            kinds = hr.row_kinds(tout, ocean)
            assert lout[0] == 0 and kinds[2] == 1 and kinds[3] == 2 and kinds[4] == 2 and kinds[5] == 3
            x = np.linspace(1.0, 2.0, npts)
            none, used = (hr.apply(tout, x, n, ocean, norm) for norm in hr.NORMS)
            assert none[2] == hr.LAND and used[2] == hr.LAND
            assert none[3] != used[3] and hr.LAND not in (none[3], used[3])              # some land: NONE differs from USED
            assert none[4] != hr.LAND and used[4] == hr.LAND                             # the used weights sum to 0.0
            assert (kinds == 2).sum() >= 2 and (kinds == 1).sum() >= 1


def test_host_hgrid_check_names_table_row_and_entry(api):
    good = hr.csr([[(0, 1.0), (2, -0.5)], [], [(1, 0.25), (1, 0.25)]])
    assert api.host_hgrid_check("in", good, 3, 3) is None
    ptr, idx, w = good

    def changed(**kw):
        t = dict(ptr=ptr.copy(), idx=idx.copy(), w=w.copy())
        for k, (at, v) in kw.items():
            t[k][at] = v
        return t["ptr"], t["idx"], t["w"]

    bad = {
        "ptr[0] != 0": (changed(ptr=(0, 1)), r"table out: row 0: ptr\[0\]=1"),
        "ptr decreases": (changed(ptr=(2, 1)), r"table out: row 1: ptr decreases"),
        "an index past the end": (changed(idx=(3, 3)), r"table out: row 2: entry 3: index 3 is outside 0\.\.2"),
        "a negative index": (changed(idx=(0, -1)), r"table out: row 0: entry 0: index -1"),
        "a NaN weight": (changed(w=(1, float("nan"))), r"table out: row 0: entry 1: the weight is not finite"),
        "an infinite weight": (changed(w=(2, float("inf"))), r"table out: row 2: entry 2: the weight is not finite"),
    }
    for what, (t, msg) in bad.items():
        got = api.host_hgrid_check("out", t, 3, 3)
        assert got is not None and re.search(msg, got), (what, got)
    assert api.host_hgrid_check("in", good, 3, 2) is not None      # the same table over fewer source points


def test_host_hgrid_apply_is_the_restatement(api):
    n = 0
    for what, table, nrows, nsrc, ocean in _tables():
        rng = np.random.default_rng(n)
        x = rng.uniform(-30.0, 30.0, nsrc)
        x[::7] = -0.0
        if ocean is None:
            assert np.array_equal(_bits(api.host_hgrid_apply(table, x, nrows)), _bits(hr.apply(table, x, nrows))), what
        else:
            held = rng.uniform(-1.0, 1.0, nrows)
            for norm in hr.NORMS:
                for fill in (True, False):
                    got = api.host_hgrid_apply(table, x, nrows, used=ocean, norm=norm, fill=fill, land_value=hr.LAND, out=held)
                    want = hr.apply(table, x, nrows, ocean, norm, fill, hr.LAND, held)
                    assert np.array_equal(_bits(got), _bits(want)), (what, norm, fill)
            none, used = (hr.apply(table, x, nrows, ocean, norm) for norm in hr.NORMS)
            assert (none != used).any()
        n += 1
    assert n == 8
    # a lone -0.0 survives: the first term is an assignment
    lone = hr.csr([[(0, 1.0)], [(0, 1.0), (1, 1.0)]])
    got = api.host_hgrid_apply(lone, [-0.0, -0.0], 2)
    assert np.signbit(got[0]) and np.signbit(got[1]) and np.signbit(hr.apply(lone, [-0.0, -0.0], 2)).all()
    with pytest.raises(ValueError):
        api.host_hgrid_apply(lone, [0.0, 0.0], 2, norm=2)


def _check_slices(what, table, nrows, rows, keep, off, ln, idx, w):
    ptr, tidx, tw = table
    listed = np.arange(nrows) if rows is None else np.asarray(rows)
    nslices = (len(listed) + 63) // 64
    assert len(off) == nslices + 1 and off[0] == 0 and len(ln) == len(listed), what
    seen = np.zeros(len(idx), dtype=bool)
    for s in range(nslices):
        width = 0
        for j in range(64 * s, min(64 * s + 64, len(listed))):
            r = listed[j]
            ent = [e for e in range(ptr[r], ptr[r + 1]) if keep is None or keep[tidx[e]]]
            assert ln[j] == len(ent), (what, j)
            for k, e in enumerate(ent):                       # order kept, dropped entries gone
                at = off[s] + 64 * k + j % 64
                assert idx[at] == tidx[e] and _bits(w[at]) == _bits(tw[e]), (what, j, k)
                seen[at] = True
            width = max(width, len(ent))
        assert off[s + 1] - off[s] == 64 * width, (what, s)     # a slice is as wide as its longest row
    assert len(idx) == len(w) == off[-1]
    assert (idx[~seen] == 0).all() and (w[~seen] == 0.0).all(), what


def test_host_hgrid_slices_puts_every_entry_at_the_stated_address(api):
    for what, table, nrows, nsrc, ocean in _tables():
        _check_slices(what, table, nrows, None, None, *api.host_hgrid_slices(table, nrows))
        if ocean is not None:    # the out direction: the entries of non-resident points dropped
            got = api.host_hgrid_slices(table, nrows, keep=ocean)
            _check_slices(what + ", land dropped", table, nrows, None, ocean, *got)
            assert got[1][2] == 0 and got[1][3] == 3
        else:                    # the in direction: the rows of the resident columns, in column order
            rows = np.nonzero(lc.ocean(lc.CASES[what.split()[0]]))[0]
            _check_slices(what + ", resident rows", table, nrows, rows, None, *api.host_hgrid_slices(table, nrows, rows=rows))
    # 150 listed rows, no multiple of 64: three slices, the last of 22 rows
    case = lc.CASES["sweep_nd3"]
    table = hr.general_in(case.ncol, 37, lc.ocean(case), 3)
    rows = np.random.default_rng(5).permutation(case.ncol)[:150]
    off, ln, idx, w = api.host_hgrid_slices(table, case.ncol, rows=rows)
    assert len(off) == 4 and len(ln) == 150
    _check_slices("150 rows", table, case.ncol, rows, None, off, ln, idx, w)
    # no row, and rows that are all empty
    off, ln, idx, w = api.host_hgrid_slices(hr.csr([[], []]), 2)
    assert list(off) == [0, 0] and list(ln) == [0, 0] and len(idx) == 0
    off, ln, idx, w = api.host_hgrid_slices(hr.csr([[(0, 1.0)]]), 1, rows=[])
    assert list(off) == [0] and len(ln) == 0


def test_the_host_functions_on_their_own_under_the_sanitizers(tmp_path):
    """tests/hgrid_table_main.cpp with mckpp_hgrid_table.cpp, built with -fsanitize=address,undefined and run as it is,
    on the same tables; every array of the program is a heap block of exactly its length"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hgrid_table")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", os.path.join(ROOT, "tests", "hgrid_table_main.cpp"),
                           os.path.join(CSRC, "mckpp_hgrid_table.cpp"), "-o", exe])
    cases, lines = [], []
    for what, table, nrows, nsrc, ocean in _tables():
        rng = np.random.default_rng(len(cases))
        x = rng.uniform(-30.0, 30.0, nsrc)
        mask = np.ones(nsrc, dtype=np.int64) if ocean is None else ocean
        rows = rng.permutation(nrows)[:min(nrows, 150)]
        norm, fill = (-1, 1) if ocean is None else (len(cases) % 2, len(cases) // 2 % 2)
        cases.append((what, table, nrows, nsrc, ocean, x, mask, rows, norm, fill))
    bad = hr.csr([[(0, 1.0)], [(5, 1.0)]])
    cases.append(("an index out of range", bad, 2, 3, None, np.zeros(3), np.ones(3, dtype=np.int64), np.arange(2), -1, 1))
    for what, (ptr, idx, w), nrows, nsrc, ocean, x, mask, rows, norm, fill in cases:
        lines.append(f"{nrows} {nsrc} {len(idx)} {len(rows)} {norm} {fill}")
        lines.append(" ".join(str(int(v)) for v in ptr))
        lines.append(" ".join(str(int(v)) for v in idx))
        lines.append(" ".join(float(v).hex() for v in w))
        lines.append(" ".join(float(v).hex() for v in x))
        lines.append(" ".join(str(int(v)) for v in mask))
        lines.append(" ".join(str(int(v)) for v in rows))
        lines.append(float(hr.LAND).hex())
    (tmp_path / "tables.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(tmp_path / "tables.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(r.stdout.split("\n"))
    for what, table, nrows, nsrc, ocean, x, mask, rows, norm, fill in cases[:-1]:
        assert next(out) == "check 0", what
        assert next(out) == "apply"
        got = np.array([float.fromhex(next(out)) for _ in range(nrows)])
        want = hr.apply(table, x, nrows) if norm < 0 else \
            hr.apply(table, x, nrows, mask, hr.NORMS[norm], bool(fill), hr.LAND, np.full(nrows, -7.0))
        assert np.array_equal(_bits(got), _bits(want)), what
        padded = int(next(out).split()[1])
        off = np.array(next(out).split(), dtype=np.int64)
        ln = np.array(next(out).split(), dtype=np.int64)
        idx = np.array(next(out).split(), dtype=np.int64)
        w = np.array([float.fromhex(v) for v in next(out).split()])
        assert padded == off[-1]
        _check_slices(what, table, nrows, rows, mask, off, ln, idx, w)
    assert next(out) == "check -1"
    assert "table t: row 1: entry 1: index 5 is outside 0..2" in next(out)


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


@pytest.mark.parametrize("cls", ["MckppHip", "MckppHipMulti"])
def test_python_argument_checks_come_before_any_library_call(api, cls, monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(api, "_lib", lambda: stub)
    npts, nzp1, n = 12, 41, 5
    h = getattr(api, cls).__new__(getattr(api, cls))
    h._h, h._held, h._npts, h._nzp1 = C.c_void_p(0x1000), {}, npts, nzp1
    pre = h._pre
    tin = hr.csr([[(p % n, 1.0)] for p in range(npts)])
    tout = hr.csr([[(j, 0.5), (j + 1, 0.5)] for j in range(n)])

    class Csr:      # what scipy.sparse.csr_matrix shows
        indptr, indices, data = tout

    bad_define = {
        "a grid number past the last": ((4, n, tin, tout), "grid 4"),
        "a bool": ((True, n, tin, tout), "grid True"),
        "a negative n": ((0, -1, tin, tout), "n=-1"),
        "a pair": ((0, n, tin[:2], tout), r"table_in: a table is a \(ptr, idx, w\) triple"),
        "the tables swapped": ((0, n, tout, tin), f"table_in: ptr has shape \\({n + 1},\\); the table has {npts} rows"),
        "idx and w of two lengths": ((0, n, (tin[0], tin[1], tin[2][:-1]), None), "table_in: idx has shape"),
        "ptr past the entries": ((0, n, None, (tout[0], tout[1][:4], tout[2][:4])), "table_out: ptr names entry 9"),
    }
    for what, (args, msg) in bad_define.items():
        with pytest.raises(ValueError, match=msg):
            h.hgrid_define(*args)
        assert stub.calls == [], what
    h.hgrid_define(0, n, tin, tout)
    h.hgrid_define(1, n, None, Csr)
    h.hgrid_define(2, 7, hr.csr([[(0, 1.0)]] * npts))
    h.hgrid_define(2, 0)
    assert [c[0] for c in stub.calls] == [pre + "hgrid_define"] * 4 and h._hgrids() == {0: n, 1: n}
    assert [c[1][1:3] for c in stub.calls] == [(0, n), (1, n), (2, 7), (2, 0)]
    assert stub.calls[1][1][3] is None and stub.calls[1][1][4] is not None and stub.calls[3][1][3:] == (None, None)
    t = stub.calls[0][1][4]._obj
    assert [t.ptr[j] for j in range(n + 1)] == list(tout[0]) and t.idx[9] == 5 and t.w[9] == 0.5
    del stub.calls[:]
    dev = FakeDeviceArray
    f8, one, t3, f32 = dev((8, n)), dev((n,)), dev((3, n), ptr=0x9000000), dev((1, n), "<f4", ptr=0x8000000)
    bad_in = {
        "a numpy array": ((0, 1, np.zeros((8, n))), "a host array"),
        "arrays of the model's size": ((0, 1, dev((8, npts))), f"the call takes {8 * n} elements"),
        "seven fields": ((0, 1, [one] * 7), "7 fields"),
        "an undefined grid": ((3, 1, f8), "grid 3 is not defined"),
        "a dropped grid": ((2, 1, f8), "grid 2 is not defined"),
    }
    for what, (args, msg) in bad_in.items():
        for call in (h.hgrid_fluxes_dev, h.hgrid_flux_ring_put_dev):
            with pytest.raises(ValueError, match=msg):
                call(*args)
            assert stub.calls == [], what
    bad_out = {
        "a numpy array": ([("T", 0, np.zeros((1, n)))], {}, "a host array"),
        "an undefined grid": ([("T", 0, t3), ("T", 3, t3)], {}, r"planes\[1\]: grid 3 is not defined"),
        "an unknown field": ([("sst", 0, t3)], {}, r"planes\[0\]: unknown output field"),
        "levels past the axis": ([("T", 0, t3, 40, 3)], {}, r"planes\[0\]: levels 40 \.\. 42 of field T"),
        "two levels of hmix": ([("hmix", 0, dev((2, n)))], {}, "field hmix, whose axis has 1"),
        "an array of the model's size": ([("T", 0, dev((3, npts)), 0, 3)], {}, f"the call takes {3 * n} elements"),
        "an unknown norm": ([("T", 0, t3)], dict(norm="area"), "norm 'area'"),
        "a plane of two": ([("T", t3)], {}, r"planes\[0\] is \(field, grid, out\)"),
        "65 planes": ([("T", 0, t3)] * 65, {}, "65 planes, at most 64"),
    }
    for what, (planes, kw, msg) in bad_out.items():
        with pytest.raises(ValueError, match=msg):
            h.hgrid_fetch_dev(planes, **kw)
        assert stub.calls == [], what
    # well-formed calls reach the library with the right tables
    F64, F32, O = api.EXP_F64, api.EXP_F32, api.OUT
    h.hgrid_fluxes_dev(0, 5, f8, l_rest=1, fence=False)
    h.hgrid_flux_ring_put_dev(1, 2, [one] * 8, fence=True)
    h.hgrid_fetch_dev([("T", 0, t3), ("hmix", 1, f32), ("S", 1, t3, 38, 3)], norm="used", land_value=-1.0)
    h.hgrid_fetch_dev([("T", 0, f32, 0, 1)], fill_land=False)
    h.hgrid_info(1)
    names = ["hgrid_fluxes_dev", "hgrid_flux_ring_put_dev", "dev_fence", "hgrid_fetch_dev", "hgrid_fetch_dev", "hgrid_info"]
    assert [c[0] for c in stub.calls] == [pre + x for x in names]
    a = stub.calls[0][1]
    assert a[1:3] == (0, 5) and [a[3][m] for m in range(8)] == [0x7000000 + 8 * n * m for m in range(8)] and a[4:7] == (1, 334000.0, 2.5e6)
    b = stub.calls[1][1]
    assert b[1:3] == (1, 2) and [b[3][m] for m in range(8)] == [0x7000000] * 8
    fields = STRUCTS["mckpp_hgrid_plane_c"][1]
    tab = stub.calls[3][1]
    assert [tuple(getattr(tab[2][k], f) for f in fields) for k in range(tab[1])] == [
        (O["T"], 0, 3, F64, 0, 1, 1, -1.0, 0x9000000), (O["hmix"], 0, 1, F32, 1, 1, 1, -1.0, 0x8000000),
        (O["S"], 38, 3, F64, 1, 1, 1, -1.0, 0x9000000)]
    tab = stub.calls[4][1]
    assert tuple(getattr(tab[2][0], f) for f in fields) == (O["T"], 0, 1, F32, 0, 0, 0, 1e20, 0x8000000)
    h._h = C.c_void_p()   # (nothing to finalize)


def test_fortran_layer_builds_with_the_hgrid_bindings(built, tmp_path):
    """A program that uses the two types, the constants and every interface compiles and links against the layer, and
    what it gets from the host functions is the header's arithmetic and layout."""
    src = tmp_path / "uses_hgrid.F90"
    src.write_text("""program uses_hgrid
  use iso_c_binding
  use mckpp_hip_binding, only: mckpp_hgrid_table_c, mckpp_hgrid_plane_c, MCKPP_OUT_T, MCKPP_EXP_F32, MCKPP_HGRIDS, &
    MCKPP_HGRID_PLANES_MAX, MCKPP_HGRID_NORM_NONE, MCKPP_HGRID_NORM_USED, mckpp_host_hgrid_check, mckpp_host_hgrid_apply, &
    mckpp_host_hgrid_slices, mckpp_hip_hgrid_define, mckpp_hip_hgrid_info, mckpp_hip_hgrid_fluxes_dev, &
    mckpp_hip_hgrid_flux_ring_put_dev, mckpp_hip_hgrid_fetch_dev, mckpp_hip_multi_hgrid_define, mckpp_hip_multi_hgrid_info, &
    mckpp_hip_multi_hgrid_fluxes_dev, mckpp_hip_multi_hgrid_flux_ring_put_dev, mckpp_hip_multi_hgrid_fetch_dev
  implicit none
  type(mckpp_hgrid_table_c), target :: t
  type(mckpp_hgrid_plane_c) :: planes(1)
  integer(c_int64_t), target :: ptr(3), info(6), off(2)
  integer(c_int32_t), target :: idx(3), len(2)
  real(c_double), target :: w(3), x(2), out(2)
  character(kind=c_char) :: msg(128)
  type(c_ptr) :: fields(8)
  integer(c_int) :: rc
  integer(c_int64_t) :: padded
  ptr = [0_c_int64_t, 2_c_int64_t, 3_c_int64_t]
  idx = [0, 1, 1]
  w = [0.5_c_double, 0.25_c_double, -1.0_c_double]
  x = [2.0_c_double, 4.0_c_double]
  t = mckpp_hgrid_table_c(c_loc(ptr), c_loc(idx), c_loc(w))
  planes(1) = mckpp_hgrid_plane_c(MCKPP_OUT_T, 0, 1, MCKPP_EXP_F32, 2, MCKPP_HGRID_NORM_USED, 1, 1.0e20_c_double, c_null_ptr)
  if (planes(1)%grid /= 2 .or. planes(1)%norm /= 1 .or. MCKPP_HGRIDS /= 4 .or. MCKPP_HGRID_PLANES_MAX /= 64) error stop 1
  if (mckpp_host_hgrid_check("in" // c_null_char, 2_c_int64_t, 2_c_int64_t, t, msg, 128_c_int64_t) /= 0) error stop 2
  if (mckpp_host_hgrid_check("in" // c_null_char, 2_c_int64_t, 1_c_int64_t, t, msg, 128_c_int64_t) /= -1) error stop 3
  rc = mckpp_host_hgrid_apply(2_c_int64_t, t, x, c_null_ptr, MCKPP_HGRID_NORM_NONE, 1, 0.0_c_double, out)
  if (rc /= 0 .or. out(1) /= 2.0_c_double .or. out(2) /= -4.0_c_double) error stop 4
  padded = mckpp_host_hgrid_slices(2_c_int64_t, c_null_ptr, t, c_null_ptr, off, len, c_null_ptr, c_null_ptr)
  if (padded /= 128 .or. off(2) /= 128 .or. any(len /= [2, 1])) error stop 5
  fields = c_null_ptr
  if (command_argument_count() > 0) then
    rc = mckpp_hip_hgrid_define(c_null_ptr, 0, 2_c_int64_t, c_loc(t), c_null_ptr)
    rc = mckpp_hip_hgrid_info(c_null_ptr, 0, info)
    rc = mckpp_hip_hgrid_fluxes_dev(c_null_ptr, 0, 1, fields, 0, 334000.0_c_double, 2.5e6_c_double, c_null_ptr)
    rc = mckpp_hip_hgrid_flux_ring_put_dev(c_null_ptr, 0, 0, fields, c_null_ptr)
    rc = mckpp_hip_hgrid_fetch_dev(c_null_ptr, 1, planes, c_null_ptr)
    rc = mckpp_hip_multi_hgrid_define(c_null_ptr, 0, 2_c_int64_t, c_loc(t), c_null_ptr)
    rc = mckpp_hip_multi_hgrid_info(c_null_ptr, 0, info)
    rc = mckpp_hip_multi_hgrid_fluxes_dev(c_null_ptr, 0, 1, fields, 0, 334000.0_c_double, 2.5e6_c_double, c_null_ptr)
    rc = mckpp_hip_multi_hgrid_flux_ring_put_dev(c_null_ptr, 0, 0, fields, c_null_ptr)
    rc = mckpp_hip_multi_hgrid_fetch_dev(c_null_ptr, 1, planes, c_null_ptr)
  end if
end program uses_hgrid
""")
    exe = tmp_path / "uses_hgrid"
    bdir = os.path.join(FDIR, "build")
    r = subprocess.run([FC, "-cpp", "-I" + bdir, str(src), os.path.join(bdir, "libmckpp_f90.a"),
                        "-L" + os.path.join(ROOT, "mckpp_f90_amd"), "-lmckpp_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "mckpp_f90_amd"), "-o", str(exe)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert exe.exists()
    assert subprocess.run([str(exe)]).returncode == 0
