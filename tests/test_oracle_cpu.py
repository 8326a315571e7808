"""CPU tests of the oracle: pinned to the reference's own check values, to
golden vectors produced by the compiled reference, and (when oracle/_ref is
present) to the compiled reference itself on a million points."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import common as cm
from oracle import orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731


def _abk(fn, S, T, P, kappa=1.0):
    a, b, k, s0, s = (C.c_double(v) for v in (1.0, 1.0, kappa, 0.0, 0.0))
    fn(S, T, P, C.byref(a), C.byref(b), C.byref(k), C.byref(s0), C.byref(s))
    return a.value, b.value, k.value, s0.value, s.value


def test_reference_check_values():
    """Check values printed in the reference's comments:
    src/mckpp_physics_state_equations.F90:24-25 (CPSW) and :105-111 (alpha, beta, kappa)."""
    L = orc.lib()
    assert abs(L.orc_cpsw(40.0, 40.0, 10000.0) - 3849.500) < 1e-3
    a, b, k, _, _ = _abk(L.orc_abk80, 35.0, 15.0, 0.0)
    assert abs(a / 2.14136e-4 - 1) < 5e-6 and abs(b / 7.51638e-4 - 1) < 5e-6 and abs(k / 4.32576e-5 - 1) < 5e-6
    a, b, k, _, _ = _abk(L.orc_abk80, 40.0, 0.0, 10000.0)
    assert abs(a / 2.69822e-4 - 1) < 5e-6 and abs(b / 6.88317e-4 - 1) < 5e-6 and abs(k / 3.55271e-5 - 1) < 5e-6


def test_eos_golden_bitexact():
    g = np.load(os.path.join(GOLD, "eos_ref.npz"))
    n = len(g["s"])
    L = orc.lib()
    out = [np.zeros(n) for _ in range(5)]
    L.orc_abk80_batch(n, dp(g["s"]), dp(g["t"]), dp(g["p"]), *[dp(o) for o in out[:4]])
    L.orc_cpsw_batch(n, dp(g["s"]), dp(g["t"]), dp(g["p"]), dp(out[4]))
    for o, nm in zip(out, ("alpha", "beta", "sig0", "sig", "cp")):
        assert np.array_equal(o.view(np.int64), g[nm].view(np.int64)), nm


def test_z121_golden_bitexact():
    g = np.load(os.path.join(GOLD, "z121_ref.npz"))
    L = orc.lib()
    for km, vin, vout, wout in zip(g["km"], g["vin"], g["vout"], g["wout"]):
        v = vin[: km + 2].copy()
        w = np.full(km + 2, 7.0)
        L.orc_z121(int(km) + 1, 0.0, 0.8, dp(v), dp(w))
        assert np.array_equal(v.view(np.int64), vout[: km + 2].view(np.int64))
        assert np.array_equal(w, wout[: km + 2])


def _golden_module():
    sys.path.insert(0, GOLD)
    import make_golden as mg
    return mg


def _ref_checks():
    """What the compiled reference returned for the two tests below (tests/golden/eos_ref_checks.json, written by
    tests/golden/make_golden.py), and the compiled reference itself where __graft_entry__.build() made oracle/_ref."""
    with open(os.path.join(GOLD, "eos_ref_checks.json")) as f:
        checks = json.load(f)
    return checks, (orc.ref() if os.path.exists(orc.REFLIB) else None)


def test_eos_vs_compiled_reference_1e6(built):
    mg = _golden_module()
    checks, R = _ref_checks()
    L = orc.lib()
    pts = mg.eos_points_1e6()
    assert mg.digest(np.stack(pts)) == checks["eos_1e6"]["inputs_sha256"], "the seeded 1e6 points are not the recorded ones"
    o = mg.eos_batch(L, "orc", *pts)
    for name in mg.EOS_NAMES:
        assert mg.digest(o[name]) == checks["eos_1e6"]["sha256"][name], name
    if R is not None:
        r = mg.eos_batch(R, "ref", *pts)
        for name in mg.EOS_NAMES:
            assert np.array_equal(o[name].view(np.int64), r[name].view(np.int64)), name


def test_abk80_flag_paths_vs_compiled_reference(built):
    """P = 0 short-cuts and the kappa-only / alpha-only entry paths of mckpp_abk80."""
    mg = _golden_module()
    checks, R = _ref_checks()
    L = orc.lib()
    mine = mg.abk80_paths(L.orc_abk80)
    refs = [[[float.fromhex(v) for v in r] for r in checks["abk80_paths"]]]
    if R is not None:
        refs.append(mg.abk80_paths(R.ref_abk80))
    entries = [(S, T, P, a0, b0, k0) for S, T, P in mg.ABK80_POINTS for a0, b0, k0 in mg.ABK80_FLAGS]
    for ref in refs:
        assert len(ref) == len(entries)
        for e, got, want in zip(entries, mine, ref):
            assert tuple(got) == tuple(want), (e, got, want)


def test_portable_exp_accuracy():
    L = orc.lib()
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-80, 10, 20000), [0.0, -80.0, 1e-300, -1e-300, 700.0, -740.0]])
    y = np.array([L.orc_exp_portable(float(v)) for v in x])
    ref = np.exp(x)
    ulp = np.spacing(ref)
    assert np.all(np.abs(y - ref) <= 1.0 * ulp)
    assert L.orc_exp_portable(0.0) == 1.0


def test_lookup_table_properties():
    """wmt/wst (src/mckpp_physics_lookup_mod.F90:42-64): last row (zehat=0) is the neutral
    value vonk*ustar; unstable entries exceed it; continuity across the zeta switch."""
    oc = orc.Const(40)
    wm, ws = oc.wmt, oc.wst          # [j, i]
    du = 0.04 / 49
    usta = du * np.arange(50)
    assert np.allclose(wm[:, 891], 0.4 * usta, rtol=1e-13, atol=0)
    assert np.all(wm[1:, :891] >= wm[1:, 891:892] * (1 - 1e-12))
    assert np.all(np.isfinite(wm)) and np.all(np.isfinite(ws)) and np.all(wm >= 0) and np.all(ws >= 0)


def test_tridiagonal_solver_residual():
    """tridcof + tridmat (src/mckpp_physics_solvers.F90:14-44, 112-161) solve A y = rhs."""
    L = orc.lib()
    nz = 60
    oc = orc.Const(nz)
    rng = np.random.default_rng(5)
    n = nz + 4
    diff = np.zeros(n); diff[1:nz + 1] = rng.uniform(1e-5, 5e-2, nz)
    cu, cc, cl, rhs, yo, yn, gam = (np.zeros(n) for _ in range(7))
    L.orc_tridcof(oc.ptr, dp(diff), nz, dp(cu), dp(cc), dp(cl))
    rhs[1:nz + 1] = rng.normal(size=nz)
    yo[nz + 1] = 3.25
    assert L.orc_tridmat(dp(cu), dp(cc), dp(cl), dp(rhs), dp(yo), nz, dp(yn), dp(gam)) == 0
    assert cu[1] == 0.0 and cl[nz] == 0.0 and yn[nz + 1] == 3.25
    res = cc[1:nz + 1] * yn[1:nz + 1]
    res[1:] += cu[2:nz + 1] * yn[1:nz]
    res[:-1] += cl[1:nz] * yn[2:nz + 1]
    assert np.max(np.abs(res - rhs[1:nz + 1])) < 1e-12
    # zero pivot is reported, not fatal
    cc0 = cc.copy(); cc0[1] = 1.0; cl0 = cl.copy(); cu0 = cu.copy()
    cc0[2] = cu0[2] * (cl0[1] / cc0[1])
    assert L.orc_tridmat(dp(cu0), dp(cc0), dp(cl0), dp(rhs), dp(yo), nz, dp(yn), dp(gam)) == 1


@pytest.mark.parametrize("nz,ncol", [(40, 64), (60, 96)])
def test_step_invariants(nz, ncol):
    """Heat and salt budgets of the implicit step, convergence bookkeeping, persistence contract."""
    oc, ob = cm.make_oracle(ncol, nz, exp_mode=0)
    f0 = ob["f"].copy()
    hm = oc.hm
    for nt in (1, 2):
        before = ob.copy()
        orc.physics_driver(oc, ob, nt)
        assert np.array_equal(ob["f"], f0)                       # f is not written back
        assert np.all(ob["npasses"] >= 6)                        # 3 compulsory + >=3 converged passes
        assert np.all(ob["reset_flag"] == 0)
        assert np.array_equal(ob["old"], before["newi"]) and np.array_equal(ob["newi"], 1 - ob["old"])
        for c in range(ncol):
            new = int(ob["newi"][c])
            assert np.array_equal(ob[f"Ts{new}"][c], ob["T"][c])
            assert ob["hmixd"][c, new] == ob["hmix"][c]
            assert 2 <= ob["kmix"][c] <= nz
        # heat budget: sum h (Tn-To) = dto*(-wX(0,1) + wXNT(nz) - wXNT(0)) + bottom diffusive flux
        dT = ((ob["T"][:, 1:nz + 1] - before["T"][:, 1:nz + 1]) * hm[1:nz + 1]).sum(axis=1)
        bot = hm[nz] * oc.tri1[nz] * ob["dift"][:, nz] * (before["T"][:, nz + 1] - ob["T"][:, nz])
        src = oc.c.dto * (-ob["wX1"][:, 0] + ob["wXNT1"][:, nz] - ob["wXNT1"][:, 0]) + bot
        assert np.max(np.abs(dT - src)) < 1e-9 * max(1.0, np.max(np.abs(src)))
        dS = ((ob["S"][:, 1:nz + 1] - before["S"][:, 1:nz + 1]) * hm[1:nz + 1]).sum(axis=1)
        botS = hm[nz] * oc.tri1[nz] * ob["difs"][:, nz] * (before["S"][:, nz + 1] - ob["S"][:, nz])
        srcS = oc.c.dto * (-ob["wX2"][:, 0]) + botS
        assert np.max(np.abs(dS - srcS)) < 1e-9 * max(1e-3, np.max(np.abs(srcS)))
        assert np.array_equal(ob["T"][:, nz + 1], before["T"][:, nz + 1])   # yn(nz+1) = yo(nz+1)


def test_threads_do_not_change_results():
    oc, a = cm.make_oracle(200, 40, exp_mode=1, nthreads=1)
    _, b = cm.make_oracle(200, 40, exp_mode=1, nthreads=4)
    orc.physics_driver(oc, a, 1, nthreads=1)
    orc.physics_driver(oc, b, 1, nthreads=4)
    for k in ("U", "V", "T", "S", "hmix", "kmix", "difm", "ghat"):
        assert np.array_equal(a[k], b[k]), k


def test_instability_trap_and_reset():
    """ocnstep_mod.F90:200-236 + overrides.F90:72-78: absurd currents trip the trap,
    f is perturbed for the retries only, U falls back to U_init after ten failures."""
    oc, ob = cm.make_oracle(8, 40, exp_mode=1)
    ob["U"][:, 1:5] = 50.0              # the old profile itself is absurd: |U| >= 10 after every try
    orc.physics_driver(oc, ob, 1)
    st = ob["status"]
    assert np.all(st & orc.ST_RETRIED) and np.all(st & orc.ST_FAILED)
    assert np.all(ob["reset_flag"] == 0)             # overrides.F90:121-123
    assert np.array_equal(ob["U"], ob["U_init"])
    assert np.all(ob["npasses"] >= 11 * 6)


def test_exp_mode_only_changes_last_bits():
    oc0, a = cm.make_oracle(128, 60, exp_mode=0)
    oc1, b = cm.make_oracle(128, 60, exp_mode=1)
    for nt in (1, 2, 3):
        orc.physics_driver(oc0, a, nt)
        orc.physics_driver(oc1, b, nt)
    same_path = a["npasses"] == b["npasses"]
    assert same_path.mean() > 0.9
    for k in ("T", "S", "U", "V"):
        d = np.abs(a[k][same_path] - b[k][same_path])
        assert d.max() < 1e-10, (k, d.max())


@pytest.mark.parametrize("nz", [1, 2, 3, 5, 40, 61])
def test_two_ended_elimination_solves_the_same_system(nz):
    """orc_tridmat_2e (solver mode 1: levels 1..nz/2 eliminated downward as tridmat does, nz..nz/2+1 upward, a 2x2
    system in the middle) against tridmat in the reference's order (solvers.F90:112-161): the same system, the
    same solution to rounding, its upper levels - where a perturbation from the meeting point has decayed - to the
    bit; a zero pivot met on the way up is reported like one met on the way down."""
    L = orc.lib()
    oc = orc.Const(max(nz, 2))
    rng = np.random.default_rng(nz)
    n = nz + 4
    diff = np.zeros(n); diff[1:nz + 1] = rng.uniform(1e-5, 5e-2, nz)
    cu, cc, cl, rhs, yo, y0, y1, g0, g1 = (np.zeros(n) for _ in range(9))
    if nz >= 2:
        L.orc_tridcof(oc.ptr, dp(diff), nz, dp(cu), dp(cc), dp(cl))
    else:
        cc[1] = 1.5
    rhs[1:nz + 1] = 10.0 + rng.normal(size=nz)
    yo[nz + 1] = 3.25
    assert L.orc_tridmat(dp(cu), dp(cc), dp(cl), dp(rhs), dp(yo), nz, dp(y0), dp(g0)) == 0
    assert L.orc_tridmat_2e(dp(cu), dp(cc), dp(cl), dp(rhs), dp(yo), nz, dp(y1), dp(g1)) == 0
    assert y1[nz + 1] == 3.25
    res = cc[1:nz + 1] * y1[1:nz + 1]
    res[1:] += cu[2:nz + 1] * y1[1:nz]
    res[:-1] += cl[1:nz] * y1[2:nz + 1]
    assert np.max(np.abs(res - rhs[1:nz + 1])) < 1e-12
    assert np.max(np.abs(y1[1:nz + 1] - y0[1:nz + 1])) < 1e-13 * np.abs(y0[1:nz + 1]).max()
    if nz == 1:
        assert y1[1] == y0[1]
    if nz >= 40:   # the meeting point's rounding has decayed long before the top of the column
        assert np.array_equal(y1[1:6], y0[1:6])
        # a pivot that vanishes in the upward elimination: cc(i) = 0 with cl(i) = 0
        i = nz - 6
        cc2, cl2 = cc.copy(), cl.copy()
        cc2[i] = 0.0; cl2[i] = 0.0
        assert L.orc_tridmat_2e(dp(cu), dp(cc2), dp(cl2), dp(rhs), dp(yo), nz, dp(y1), dp(g1)) == 1
        cc2 = cc.copy(); cc2[nz] = 0.0        # its first pivot
        assert L.orc_tridmat_2e(dp(cu), dp(cc2), dp(cl), dp(rhs), dp(yo), nz, dp(y1), dp(g1)) == 1


def test_two_ended_elimination_flags_a_singular_middle_system():
    """The 2x2 system where the two eliminations of orc_tridmat_2e meet has a pivot of its own, 1 - gam(m+1) g(m+1):
    when it vanishes the solver reports it like any zero pivot of tridmat (solvers.F90:140-151: the status bit, 1e-12 in
    its place) instead of returning Inf / NaN unflagged - the device's solver mode 1 does the same."""
    L = orc.lib()
    n = 8
    for nz in (2, 3, 6):
        cu, cc, cl, rhs, yo, y1, g1 = (np.zeros(n + nz) for _ in range(7))
        cc[1:nz + 1] = 1.0
        m = nz // 2
        cl[m] = 1.0; cu[m + 1] = 1.0          # levels m, m+1: [[1, 1], [1, 1]], decoupled from the rest
        rhs[1:nz + 1] = 2.0
        assert L.orc_tridmat_2e(dp(cu), dp(cc), dp(cl), dp(rhs), dp(yo), nz, dp(y1), dp(g1)) == 1
        assert np.isfinite(y1[1:nz + 1]).all()
        cl[m] = 0.5                            # regular again: no flag
        assert L.orc_tridmat_2e(dp(cu), dp(cc), dp(cl), dp(rhs), dp(yo), nz, dp(y1), dp(g1)) == 0


def test_solver_mode_and_pow_lowering_only_change_last_bits():
    """The oracle's two switches beside exp_mode: solver_mode=1 (two-ended elimination) and half_pow_mode=1 (wst built
    with pow(x, .5), as a compiler without amdflang's square-root rewrite of x**(1./2.) lowers lookup_mod.F90:60-62).
    Both are rounding-level variants: a few steps on the bench columns agree to 1e-12 (the tables over every shape and
    up to 1000 steps: profiles/r04/parity_tolerance.json)."""
    a = orc.Const(60)
    b = orc.Const(60, half_pow_mode=1)
    assert np.array_equal(a.wmt, b.wmt)
    d = a.wst != b.wst
    assert 0 < d.sum() < 200, d.sum()      # (27 entries with this libm, 28 with flang's)
    assert np.max(np.abs(a.wst[d] - b.wst[d]) / np.abs(a.wst[d])) < 5e-16
    oc0, r0 = cm.make_oracle(128, 60, exp_mode=1, solver_mode=0)
    oc1, r1 = cm.make_oracle(128, 60, exp_mode=1, solver_mode=1)
    oc2, r2 = cm.make_oracle(128, 60, exp_mode=1, solver_mode=0, half_pow_mode=1)
    for nt in (1, 2, 3):
        for oc, r in ((oc0, r0), (oc1, r1), (oc2, r2)):
            orc.physics_driver(oc, r, nt)
    for r in (r1, r2):
        assert np.array_equal(r["npasses"], r0["npasses"]) and np.array_equal(r["kmix"], r0["kmix"])
        m = cm.tolerance_metrics(cm.oracle_state(r, 60), cm.oracle_state(r0, 60))
        assert m["off_path_columns"] == 0
        assert all(v["max"] < 1e-12 for v in m["same_path"].values()), m["same_path"]
    assert not np.array_equal(r1["T"], r0["T"])     # (it IS another order of operations)


def test_fluxes_assembly():
    """mckpp_fluxes restatement: defaults of the no-flux-file branch (fluxes_mod.F90:41-49) reproduce
    synth.forcing("baseline"); calm points get taux=1e-10; wXNT follows swdk_opt."""
    n, nz = 5, 40
    oc, ob = cm.make_oracle(n, nz, exp_mode=0)
    one = np.ones(n)
    orc.fluxes(oc, ob, 1, 0.01 * one, 0 * one, 200 * one, 0 * one, -150 * one, 0 * one, 6e-5 * one, 0 * one)
    assert np.array_equal(ob["sflux"], cm.synth.forcing(n, "baseline"))
    w = ob["wXNT1"][:, 0:nz + 1]
    assert np.all(w[:, 0] < 0) and np.all(np.diff(np.abs(w), axis=1) < 0)       # decays with depth
    assert np.allclose(w[:, 0], -200.0 / (ob["rho"][:, 0] * ob["cp"][:, 0]), rtol=1e-15)
    orc.fluxes(oc, ob, 2, 0 * one, 0 * one, 200 * one, 0 * one, -150 * one, 0 * one, 6e-5 * one, 0 * one)
    assert np.all(ob["sflux"][:, 0] == 1e-10)


def test_bottomtemp_override():
    """overrides.F90:12-24: the increment, its heat-flux equivalent and the overwritten bottom point."""
    from oracle import orc

    ncol, nz = 9, 40
    oc, ob = cm.make_oracle(ncol, nz, exp_mode=0)
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    orc.physics_driver(oc, ob, 1)
    t_old = ob["T"][:, nz + 1].copy()
    rho, cp = ob["rho"][:, nz + 1].copy(), ob["cp"][:, nz + 1].copy()
    bt = t_old + np.linspace(-0.5, 0.5, ncol)
    orc.bottomtemp(oc, ob, bt)
    assert np.array_equal(ob["T"][:, nz + 1], bt)
    assert np.array_equal(ob["tinc_fcorr"][:, nz + 1], bt - t_old)
    assert np.array_equal(ob["ocnTcorr"][:, nz + 1], (bt - t_old) * rho * cp / 3600.0)
    assert np.all(ob["tinc_fcorr"][:, 1:nz + 1] == 0)


def _conv_check(x, p3, p4, ph, pt, pq, lit):
    L = orc.lib()
    n = len(x)
    o = [np.zeros(n) for _ in range(5)]
    L.orc_conv_probe(n, dp(x), *[dp(a) for a in o])
    for name, mine, want in zip(("x**3", "x**4", "x**(1./2.)", "x**(1./3.)", "x**(1./4.)"), o, (p3, p4, ph, pt, pq)):
        bad = mine.view(np.int64) != want.view(np.int64)
        assert not bad.any(), f"{name}: the oracle's C lowering differs from amdflang's on {int(bad.sum())} of {n} values"
    ol = np.zeros(11)
    L.orc_conv_literals(dp(ol))
    assert np.array_equal(ol.view(np.int64), lit[:11].view(np.int64)), "unkinded literals are not full doubles"
    assert lit[11] == 8.0     # KIND of default REAL under -fdefault-real-8


def test_compiler_conventions_golden():
    """The Fortran constructs the oracle lowers by hand - integer powers, **(1./2.), **(1./3.), **(1./4.),
    unkinded literals - against what amdflang produced for them (tests/golden/conv_probe.npz, made by
    tests/golden/make_conv_golden.py from oracle/conv_probe.F90).  Found with this probe: **(1./2.) is a
    square root, which differs from libm's pow(x, .5) in 28 entries of the wst table."""
    g = np.load(os.path.join(GOLD, "conv_probe.npz"))
    _conv_check(np.ascontiguousarray(g["x"]), g["p3"], g["p4"], g["ph"], g["pt"], g["pq"], g["literals"])
    x = g["x"]
    assert np.array_equal(g["ph"], np.sqrt(x)) and np.array_equal(g["p4"], ((x * x) * x) * x)
    assert not np.array_equal(g["p4"], (x * x) * (x * x))      # the association matters


def test_compiler_conventions_live():
    """Same check against a fresh amdflang build of the probe, where the compiler is installed."""
    P = orc.conv_probe()
    if P is None:
        pytest.skip("amdflang not installed here")
    rng = np.random.default_rng(5)
    x = np.ascontiguousarray(np.concatenate([rng.uniform(0, 20, 50000), 10 ** rng.uniform(-15, 5, 50000)]))
    n = len(x)
    o = [np.zeros(n) for _ in range(5)]
    P.conv_probe_powers(n, dp(x), *[dp(a) for a in o])
    lit = np.zeros(12)
    P.conv_probe_literals(dp(lit))
    _conv_check(x, *o, lit)


def _conv2_compare(want, got):
    """amdflang's results (`want`) against the oracle's C lowering (`got`): bit for bit, integers equal."""
    assert set(want) == set(got)
    for name in sorted(want):
        w, g = np.asarray(want[name]), np.asarray(got[name])
        if w.dtype.kind == "i":
            bad = w != g
        else:
            bad = np.ascontiguousarray(w).view(np.int64) != np.ascontiguousarray(g).view(np.int64)
        assert not bad.any(), (f"{name}: the oracle's C lowering differs from amdflang's on {int(bad.sum())} of {bad.size} values, "
                               f"first at index {int(np.flatnonzero(bad)[0])}")


def _conv2_module():
    sys.path.insert(0, GOLD)
    import make_conv_golden2 as g2
    return g2


def test_compiler_conventions_intrinsics_golden():
    """EXP (>= 1e4 arguments in [-80, 0] and the model's own -dm(k)/a1, -hbl/a2 of every BASELINE grid and Jerlov type),
    SQRT, ABS, x**2, swfrac / swdk as the reference writes them (swfrac_mod.F90:74-77, fluxes_mod.F90:134-135),
    SIGN(a, b) incl. SIGN(0.5, +-0.0) and SIGN(0.5, x + epsln) near zero (bldepth_mod.F90:123,196,201), MAX / MIN /
    AMAX1 / AMIN1 with 2-4 arguments incl. equal and signed-zero operands, ifix / int / float (blmix_mod.F90:68,
    wscale_mod.F90:65-77): what amdflang returned for them under the reference's flags
    (tests/golden/conv_probe_intrinsics.npz, made by tests/golden/make_conv_golden2.py from oracle/conv_probe.F90: the
    inputs and a SHA-256 digest of each output array) against the oracle's lowering - exp(), sqrt(), fabs(), copysign,
    a > b ? a : b left to right, (int) - bit for bit.  exp_mode = 0 of the oracle is therefore amdflang's EXP, not an
    assumption about it."""
    g2 = _conv2_module()
    z = np.load(os.path.join(GOLD, "conv_probe_intrinsics.npz"))
    inp = {k[3:]: np.ascontiguousarray(z[k]) for k in z.files if k.startswith("in_")}
    want = {k[7:]: str(z[k]) for k in z.files if k.startswith("sha256_")}
    assert (inp["x"] <= 0).sum() >= 10000 and len(inp["z"]) > 3000
    got = g2.run_oracle(inp)
    assert set(want) == set(got)
    bad = sorted(name for name in want if g2.digest(got[name]) != want[name])
    assert not bad, f"the oracle's C lowering differs from amdflang's bit for bit in {bad}"
    # what the probe says about the lowering itself (`got` is amdflang's result, bit for bit)
    assert np.array_equal(got["sign_half"][np.signbit(inp["b"])], np.zeros(int(np.signbit(inp["b"]).sum())))   # SIGN(0.5, -0.0) = -0.5
    assert np.array_equal(got["amax1"].view(np.int64), got["max"].view(np.int64))
    assert np.array_equal(got["amin1"].view(np.int64), got["min"].view(np.int64))


def test_compiler_conventions_intrinsics_live():
    """The same against a fresh amdflang build of the probe on other random arguments, where the compiler is installed."""
    P = orc.conv_probe()
    if P is None or not hasattr(P, "conv_probe_unary"):
        pytest.skip("amdflang not installed here")
    g2 = _conv2_module()
    inp = g2.inputs(seed=7, n=20000)
    _conv2_compare(g2.run_probe(P, inp), g2.run_oracle(inp))
