"""CPU tests of the drop-in boundary: the library loads, exports every symbol
declared in include/mckpp_hip.h, the ctypes mirror of the structs matches the
C layout, host helpers agree with the oracle, and compute entry points fail
loudly (no CPU fallback) when no gfx950 device is present."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import common as cm
from harness import bound_as, prototypes
from oracle import orc

ROOT = cm.ROOT
HEADER = os.path.join(ROOT, "include", "mckpp_hip.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mckpp_h(?:ip|ost)_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(built):
    import mckpp_f90_amd as mk

    lib = mk.load_library()
    names = _declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mckpp_hip.h but not exported"


def test_ctypes_signatures_match_the_header(built):
    """Every function of include/mckpp_hip.h is in api.py's signature table with the header's parameter count, each
    parameter and the return type bound as a ctypes type of the header type's class, and the loaded library carries
    exactly that; every mckpp_hip_multi_X is its mckpp_hip_X after the handle, which is what the table's twin mark
    relies on."""
    from mckpp_f90_amd import api

    protos = prototypes(HEADER)
    assert sorted(protos) == _declared_functions() and len(protos) == 114
    table = api._signatures()
    assert sorted(table) == sorted(protos)
    lib = api._lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert bound_as(ret, restype, returned=True), f"{name} returns {ret}, bound as {restype}"
        assert len(argtypes) == len(params), f"{name} takes {len(params)} parameters, {len(argtypes)} bound"
        for i, (p, t) in enumerate(zip(params, argtypes)):
            assert bound_as(p, t), f"{name}: parameter {i} is {p}, bound as {t}"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), f"{name}: _bind left another signature"
    # the twins: the same return type and the same parameters after the handle; init, which takes no handle, is the
    # only pair that differs, and every other pair is stated once in the table
    pairs = {n: "mckpp_hip_multi_" + n[len("mckpp_hip_"):] for n in protos if not n.startswith("mckpp_hip_multi_")}
    pairs = {n: m for n, m in pairs.items() if m in protos}
    assert len(pairs) == 46
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n, m in pairs.items():
        if n == "mckpp_hip_init":
            assert protos[n] != protos[m] and not api._SIGNATURES[n][2] and m in api._SIGNATURES
            continue
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_handle\s" % n, src), f"{n} takes no handle"
        assert re.search(r"\b%s\s*\(\s*mckpp_hip_multi_handle\s" % m, src), f"{m} takes no multi handle"
        assert protos[n][0] == protos[m][0] and protos[n][1][1:] == protos[m][1][1:], f"{m} is not {n} after the handle"
        assert api._SIGNATURES[n][2] and m not in api._SIGNATURES, f"{n} / {m}: one entry with the twin mark"
    assert sum(1 for s in api._SIGNATURES.values() if s[2]) == len(pairs) - 1


SINGLE_ONLY = {"vmix_pass", "vmix_only", "solver_mode", "last_kernel_ms", "last_launch_count", "kernel_residency",
               "kernel_name", "eos_batch", "exp_batch", "div_batch"}
MULTI_ONLY = {"gather"}


def test_both_handles_have_the_same_methods():
    """What one context can be asked, several GPUs behind one handle can be asked too, and the other way round, apart
    from the two lists above: a method added to one class alone fails here."""
    from mckpp_f90_amd import api

    def public(cls):
        return {n for n in dir(cls) if not n.startswith("_")
                and (callable(getattr(cls, n)) or isinstance(getattr(cls, n), property))}

    one, multi = public(api.MckppHip), public(api.MckppHipMulti)
    assert one - multi == SINGLE_ONLY
    assert multi - one == MULTI_ONLY
    assert {"upload", "step", "status", "ncolumns", "fluxes", "bottomtemp", "update_ancillaries", "load_restart",
            "window_schedule", "flux_ring_put", "close"} <= one & multi


def test_driver_context_dies_with_its_constants(built, monkeypatch):
    """The context that mckpp_initialize_ocean_model parks on its kpp_const_fields is finalized when the constants go,
    by reference counting alone: no cycle through the context keeps it (and the arrays it holds pinned) for the
    cyclic collector."""
    import gc
    import weakref

    import mckpp_f90_amd as mk
    from mckpp_f90_amd import api

    calls = []

    class Stub:
        """a library whose entry points all succeed"""

        def __getattr__(self, name):
            def entry(*args):
                calls.append(name)
                if name == "mckpp_hip_init":
                    args[-1]._obj.value = 0x1000   # (a handle: close() finalizes no null one)
                return 0
            return entry

    kc, k3 = cm.make_hip_case(4, 10)
    stub = Stub()
    gc.collect()
    gc.disable()
    try:
        monkeypatch.setattr(api, "_lib", lambda: stub)
        ctx = mk.mckpp_initialize_ocean_model(k3, kc, download=False)
        assert calls == ["mckpp_hip_init", "mckpp_hip_upload", "mckpp_hip_init_ocean"]
        alive = weakref.ref(ctx)
        del kc, k3, ctx
        assert alive() is None, "the driver's context outlives its kpp_const_fields"
        assert calls.count("mckpp_hip_finalize") == 1
    finally:
        gc.enable()


def test_struct_layout_matches_header(built, tmp_path):
    """sizeof/offsetof from a C compile of the header vs the ctypes mirror in api.py."""
    from mckpp_f90_amd import api

    csrc = tmp_path / "layout.c"
    fields_c = [f[0] for f in api._ConstC._fields_]
    fields_s = [f[0] for f in api._StateC._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu %zu\\n", sizeof(mckpp_const_c), sizeof(mckpp_state_ptrs_c));']
    for f in fields_c:
        body.append(f'printf("c {f} %zu\\n", offsetof(mckpp_const_c, {f}));')
    for f in fields_s:
        body.append(f'printf("s {f} %zu\\n", offsetof(mckpp_state_ptrs_c, {f}));')
    body.append("return 0;}")
    csrc.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(csrc), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    sz = out[0].split()
    assert int(sz[0]) == C.sizeof(api._ConstC) and int(sz[1]) == C.sizeof(api._StateC)
    for line in out[1:]:
        if not line:
            continue
        which, name, off = line.split()
        cls = api._ConstC if which == "c" else api._StateC
        assert getattr(cls, name).offset == int(off), (which, name)


def test_host_lookup_and_tri_match_oracle(built):
    import mckpp_f90_amd as mk

    nz = 60
    kc = mk.KppConstFields(nz)
    mk.mckpp_physics_lookup(kc)
    oc = orc.Const(nz)
    # Fortran wmt(0:891,0:49) == oracle [j, i] view transposed
    assert np.array_equal(np.asarray(kc.wmt).T, oc.wmt)
    assert np.array_equal(np.asarray(kc.wst).T, oc.wst)
    assert np.array_equal(kc.tri[0:nz + 1, 0, 0], oc.tri0[0:nz + 1])
    assert np.array_equal(kc.tri[0:nz + 1, 1, 0], oc.tri1[0:nz + 1])
    assert np.array_equal(kc.zm, oc.zm[1:nz + 2]) and np.array_equal(kc.dm, oc.dm[0:nz + 1])


def test_no_cpu_fallback(built):
    """Without a HIP device every compute entry point must fail with an error, never compute."""
    import torch

    import mckpp_f90_amd as mk

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    kc = mk.KppConstFields(40)
    mk.mckpp_physics_lookup(kc)
    with pytest.raises(mk.MckppHipError):
        mk.MckppHip(kc)
    k3 = mk.Kpp3dFields(4, kc)
    with pytest.raises(mk.MckppHipError):
        mk.mckpp_physics_driver(k3, kc, 1)


def test_missing_library_fails_loudly(built, tmp_path, monkeypatch):
    import mckpp_f90_amd as mk

    monkeypatch.setattr(mk, "_lib", None)
    monkeypatch.setattr(mk, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mk.load_library()


def test_product_does_not_touch_oracle():
    """The package and the C sources never import, include or link the oracle."""
    pkg = os.path.join(ROOT, "mckpp_f90_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".h", ".F90", ".f90", "Makefile")):
                txt = open(os.path.join(dirpath, fn), errors="ignore").read()
                assert "liboracle" not in txt and "mckpp_oracle" not in txt and "from oracle" not in txt \
                    and "import oracle" not in txt, os.path.join(dirpath, fn)


def test_synthetic_generators_are_sliceable():
    a = cm.synth.columns(30, 12)
    idx = np.arange(1, 30, 3)
    b = cm.synth.columns(len(idx), 12, index=idx, ntotal=30)
    for k in ("T", "S", "U", "f", "Sref"):
        assert np.array_equal(a[k][idx], b[k])
    assert np.array_equal(cm.synth.forcing(30)[idx], cm.synth.forcing(len(idx), index=idx))


def test_shard_mask_logic(built):
    """mckpp_host_shard_mask (the column-to-device map of mckpp_hip_multi_upload): the j-th run_physics
    point goes to shard j mod ndev - shards are disjoint, cover the ocean, differ by at most one column."""
    import mckpp_f90_amd as mk

    rng = np.random.default_rng(3)
    for npts, ndev in [(1, 1), (17, 3), (1000, 8), (1000, 7), (5, 8)]:
        rp = (rng.uniform(size=npts) > 0.35).astype(np.int32)
        total = np.zeros(npts, dtype=np.int32)
        counts = []
        ocean = np.flatnonzero(rp)
        for d in range(ndev):
            m, n = mk.host_shard_mask(rp, ndev, d)
            assert n == int(m.sum())
            assert np.array_equal(np.flatnonzero(m), ocean[d::ndev])      # round-robin in ipt order
            total += m
            counts.append(n)
        assert np.array_equal(total, rp) and max(counts) - min(counts) <= 1
    with pytest.raises(mk.MckppHipError):
        mk.host_shard_mask(np.ones(4, dtype=np.int32), 2, 2)


def test_hip_resources_have_one_owner():
    """The runtime creates and destroys no device block, pinned block, event or stream by hand: every such call is in
    the owners of mckpp_own.h, so no path of the runtime can forget a release."""
    csrc = os.path.join(ROOT, "mckpp_f90_amd", "csrc")
    runtime = open(os.path.join(csrc, "mckpp_runtime.cpp")).read()
    own = open(os.path.join(csrc, "mckpp_own.h")).read()
    for call in ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipMalloc(", "hipHostMalloc(",
                 "hipEventCreate", "hipStreamCreate"):
        assert call not in runtime, f"{call} in mckpp_runtime.cpp: use the owners of mckpp_own.h"
        assert call in own, call
