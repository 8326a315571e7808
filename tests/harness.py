"""What the test files share and pytest has a part in: fixtures, and helpers that assert.  Each file imports what it
uses by name (`from harness import mk  # noqa: F401`): an imported module-scoped fixture is instantiated once per
importing module, an imported autouse fixture applies to the importing module alone.  Builders of inputs that need no
pytest are in tests/common.py and the *_cases modules - bench.py, smoke() and the tools import those."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import common as cm
import ref_loop_cases as lc
import ref_step_cases as rc


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mk(built):
    import torch   # before the library: both bring a HIP runtime, the process must end up with one

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no HIP device visible)")
    import mckpp_f90_amd as m

    m.load_library()
    return m


@pytest.fixture(scope="module")
def api(built):
    import mckpp_f90_amd as mk

    mk.load_library()
    return mk.api


@pytest.fixture(scope="module")
def step_golden(built):
    """tests/golden/ref_step.npz; a file that has one record imports it `as golden`"""
    return rc.Golden()


@pytest.fixture(scope="module")
def loop_golden(built):
    """tests/golden/ref_loop.npz; a file that has one record imports it `as golden`"""
    return lc.Golden()


def cleared(env):
    """An autouse fixture that takes the variables of `env` out of the environment for every test of the module that
    binds it (`_clean_env = harness.cleared(ENV)`).  Which variables a file clears is that file's own statement: the
    suite is also run whole under MCKPP_SOLVER_MODE=1, which most files follow on purpose."""
    @pytest.fixture(autouse=True)
    def _clean_env(monkeypatch):
        for k in env:
            monkeypatch.delenv(k, raising=False)

    return _clean_env


# ---------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------
def null_ctx(api, cls):
    """A wrapper object without a device context: whatever reaches the library fails there with "null handle"."""
    h = cls.__new__(cls)
    h._h = C.c_void_p()
    h._held = {}
    return h


def initialised(mk, kc, k3, shards=0):
    """A context (shards > 0: an MckppHipMulti of that many shards on device 0) with k3 uploaded and initialised"""
    h = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    return h


def resident(mk, case, shards=0):
    """(context, KppConstFields, Kpp3dFields): the raw columns of a ref_loop case uploaded and initialised on the device"""
    kc, k3 = lc.hip_raw(case)
    return initialised(mk, kc, k3, shards), kc, k3


def force_bench(h, k3):
    """the bench forcing, constant, into k3 and onto the device"""
    cm.set_forcing_3d(k3, cm.synth.forcing(k3.npts, "bench"))
    h.set_forcing(k3.sflux)


def flux_args(case):
    return dict(l_rest=case.l_rest, flsn=lc.FLSN, el=lc.EL)


def shape(kc, npts, name):
    from mckpp_f90_amd import api

    two_d = name == "hmix" or api.OUT[name] >= api.OUT["fcorr"]   # (the 2-D fields: hmix, fcorr .. dampv_flag)
    return (npts,) if two_d else (npts, kc.nzp1)


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def assert_loop_step(golden, tag, nt, k3, kc, what):
    """the downloaded k3 of a ref_loop case after step nt against the recorded reference (tests/golden/ref_loop.npz)"""
    case = lc.CASES[tag]
    values = golden.values(tag, "pexp") if nt == case.nsteps else None
    bad = lc.mismatches(case, lc.LOOP_FIELDS, golden.sha(tag, "pexp")[nt - 1], lc.hip_get(k3, kc, case.nz), values)
    assert not bad, f"{tag} step {nt}, {what}: differs from the recorded reference: {bad}"


def loop_state(h, k3, kc, nz, names=lc.LOOP_FIELDS):
    """the named fields after a download, with the status words and the pass counts"""
    h.download(k3)
    get = lc.hip_get(k3, kc, nz)
    st, nf, npass = h.status()
    d = {n: np.array(get(n)) for n in names}
    d["status"], d["npasses"] = np.array(st), np.array(npass)
    return d


def assert_same(got, want, active, what):
    for n in want:
        assert np.array_equal(got[n][active], want[n][active], equal_nan=True), (what, n)


def differing(k3, ob, nz, active, fields=rc.STEP_FIELDS):
    return {k: v for k, v in cm.compare(k3, ob, nz, fields, active).items() if v[2] != 0}


def assert_equal_to_oracle(ctx, k3, ob, nz, active, what):
    ctx.download(k3)
    st, nf, npass = ctx.status()
    assert np.array_equal(st[active], ob["status"][active]), f"{what}: status words"
    assert np.array_equal(npass[active], ob["npasses"][active]), f"{what}: pass counts"
    bad = differing(k3, ob, nz, active)
    assert not bad, f"{what}: fields differing from the oracle (max_abs, max_rel, n_values): {bad}"


def is_the_oracles(h, k3, ob, nz, active, tag, fields=rc.STEP_FIELDS):
    h.download(k3)
    st, nf, npass = h.status()
    assert np.array_equal(st[active], ob["status"][active]), tag
    assert np.array_equal(npass[active], ob["npasses"][active]), tag
    bad = {k: v for k, v in cm.compare(k3, ob, nz, fields, active).items() if v[2] != 0}
    assert not bad, f"{tag}: fields differing from the oracle (max_abs, max_rel, n_values): {bad}"


# ---------------------------------------------------------------------------
# the Fortran driver
# ---------------------------------------------------------------------------
def drive(tmp_path, name, kc, k3, sf, nsteps, flags, shards):
    """kpp_driver on a case file written from kc, k3 and the forcing sf; the path of its output file"""
    from test_fortran_host import DRIVER, _write_case

    case, out = tmp_path / f"{name}.case", tmp_path / f"{name}.out"
    _write_case(case, kc, k3, sf, nsteps, 0, flags=flags, shards=shards)
    r = subprocess.run([DRIVER, str(case), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    return out


# ---------------------------------------------------------------------------
# the C headers against the ctypes tables
# ---------------------------------------------------------------------------
HANDLES = ("mckpp_hip_handle", "mckpp_hip_multi_handle")


def ctype(decl):
    """The type of a parameter declaration or a return type as a header writes it, without the parameter's name:
    "ptr" for any pointer, array parameter or handle, else the type's one word."""
    words = decl.replace("*", " * ").replace("[", " [ ").split()
    if "*" in words or "[" in words or words[0] in HANDLES:
        return "const char *" if words[:3] == ["const", "char", "*"] else "ptr"
    return [w for w in words if w != "const"][0]


def prototypes(header):
    """name -> (return type, [parameter types]) of every function `header` itself declares, types as ctype gives them."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"\{[^{}]*\}", "", src.replace('extern "C" {', ""))   # bodies of structs and enums
    out = {}
    for stmt in src.split(";"):
        m = re.fullmatch(r"\s*(.*?)\b(mckpp_h(?:ip|ost)_[a-z_0-9]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m:
            ret, name, params = m.groups()
            assert name not in out, name
            out[name] = (ctype(ret), [] if params.strip() == "void" else [ctype(p) for p in params.split(",")])
    return out


def bound_as(header_type, t, returned=False):
    """Is the ctypes type `t` what the header's type is bound as?"""
    if header_type == "const char *":
        return t is C.c_char_p if returned else bound_as("ptr", t)
    if header_type == "ptr":
        return isinstance(t, type) and (issubclass(t, C._Pointer) or t in (C.c_void_p, C.c_char_p)) \
            and C.sizeof(t) == C.sizeof(C.c_void_p)
    if header_type == "void":
        return returned and t is None
    if header_type in ("int", "int32_t"):
        return t in (C.c_int, C.c_int32) and C.sizeof(t) == 4
    return t is {"double": C.c_double, "int64_t": C.c_int64, "uint32_t": C.c_uint32}[header_type]
