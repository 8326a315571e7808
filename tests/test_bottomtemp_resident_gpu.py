"""The L_VARY_BOTTOM_TEMP override from a resident field (mckpp_hip_set_bottomtemp): every column-step of a step launch
ends with mckpp_physics_overrides_bottomtemp (src/mckpp_physics_overrides.F90:12-24), as the reference's driver ends every
step with it (src/mckpp_physics_driver_mod.F90:67-71), so a run with the switch on is one launch like any other.

What is expected never comes from the code under test: it is the compiled reference's record (tests/golden/ref_step.npz,
case `bottom_temp`) or the CPU oracle stepped one step at a time with orc.bottomtemp after every step (portable-exp mode).
Every case holds every field of STEP_FIELDS, the status words and the pass counts to equality, over the columns that are
stepped."""
import functools

import numpy as np
import pytest

import common as cm
import ref_step_cases as rc
from harness import cleared, force_bench, initialised, is_the_oracles, mk  # noqa: F401
from harness import step_golden as golden  # noqa: F401

pytestmark = pytest.mark.gpu

ENV = ("MCKPP_MULTISTEP", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT", "MCKPP_XCC_DROP", "MCKPP_PS_FIXED_L", "MCKPP_L3_CAP")
_clean_env = cleared(ENV)


# ---------------------------------------------------------------------------
# the cases: the same set-up on both sides
# ---------------------------------------------------------------------------
def _no_freeze(ncol, nzp1, ob):
    T = ob["T"][:, 1:nzp1 + 1].copy()
    T[::3, :] = -2.2   # below -1.8 at every level, the bottom one too
    return {"T": T}


PRE = {None: None, "fcorr_withz": rc._fcorr_withz, "relax_ocnt": rc._relax_ocnt_sal, "no_freeze": _no_freeze,
       "isotherm": rc._freeze_isotherm, "ldd": rc._salt_fingers, "tjump_clim": rc._tjump_clim}


def _both(ncol, nz, grid="uniform", land_every=0, pre=None, solver_mode=None, **switches):
    """Oracle const + batch and the HIP side's constants + fields of one case, before initialisation."""
    oc, ob, kc, k3 = cm.make_both(ncol, nz, grid, land_every, solver_mode, **switches)
    if PRE[pre]:
        rc.apply_both(ob, k3, nz + 1, PRE[pre](ncol, nz + 1, ob))
    return oc, ob, kc, k3


def _bt(ob, nz, seed=0):
    """a bottom temperature around half a kelvin below the deepest level of the start, different on every column"""
    n = ob["T"].shape[0]
    return np.asarray(ob["T"][:, nz + 1]) - 0.5 + 0.25 * np.sin(np.arange(n) + seed)


@functools.lru_cache(maxsize=None)
def _oracle(ncol, nz, nsteps, change_at=0, **case):
    """The oracle's run of a case, one step at a time with orc.bottomtemp after every step, once per case: the batch
    after the last step, the status words of every step, the bottom temperature(s), the active points.  The field
    changes to a second one before step `change_at` (0: never).  Shared and left unchanged."""
    from oracle import orc

    oc, ob, kc, k3 = _both(ncol, nz, **case)
    active = np.nonzero(k3.run_physics)[0]
    orc.init_ocean(oc, ob, 0)
    bts = [_bt(ob, nz), _bt(ob, nz, seed=5) + 0.3]
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    status = []
    ob.reset_flags = []   # (reset_flag after every step: the reach condition of the isotherm case)
    for nt in range(1, nsteps + 1):
        bt = bts[1] if change_at and nt >= change_at else bts[0]
        orc.physics_driver(oc, ob, nt)
        orc.bottomtemp(oc, ob, bt)
        status.append(np.array(ob["status"]))
        ob.reset_flags.append(np.array(ob["reset_flag"]))
    return ob, status, bts, active


def _hip(mk, ncol, nz, shards=0, **case):
    """The HIP side of the same case, initialised and forced, ready to step."""
    oc, ob, kc, k3 = _both(ncol, nz, **case)
    h = initialised(mk, kc, k3, shards)
    if case.get("solver_mode") is not None:
        h.set_solver_mode(case["solver_mode"])
    force_bench(h, k3)
    return h, kc, k3


def _fields(k3, nz):
    return {n: np.array(rc.hip_get(k3, nz)(n)) for n in rc.STEP_FIELDS}


# ---------------------------------------------------------------------------
# 1. pinned to the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("launches", ["one", "two"])
def test_pinned_to_the_compiled_reference(mk, golden, launches):
    """Golden case `bottom_temp` (24 columns, 40 levels, 2 steps, constant forcing), started as rc.run_hip starts it,
    then set_bottomtemp and the two steps as one launch or as two: the digests of the portable-exp reference build."""
    tag = "bottom_temp"
    case = rc.CASES[tag]
    oc, ob, pre, post = rc.oracle_start(case, exp_mode=1)
    assert np.array_equal(rc.input_digest(ob), golden.input_sha(tag, "pexp")), "not the recorded starting state"
    kc, k3 = cm.make_hip_case(case.ncol, case.nz, grid=case.grid, dto=case.dto, land_every=case.land_every)
    rc.apply_hip(k3, pre)
    ctx = mk.MckppHip(kc)
    ctx.set_solver_mode(0)
    ctx.upload(k3)
    ctx.init_ocean(0)
    ctx.download(k3)
    act = rc.active_columns(case)
    init = cm.compare(k3, ob, case.nz, rc.STEP_FIELDS, act)
    assert not {k: v for k, v in init.items() if v[2]}, f"HIP starting state differs from the oracle's: {init}"
    bt = rc.bottom_temp(case, ob)
    cm.set_forcing_3d(k3, rc.forcing(case, 1))
    ctx.set_forcing(k3.sflux)
    ctx.set_bottomtemp(bt)
    digests, values = golden.digests(tag, "pexp"), golden.values(tag)
    steps = list(rc.run_oracle(case, oc, ob)) if launches == "one" else None   # (status words: the oracle's)
    if launches == "one":
        ctx.step(1, case.nsteps)
        assert ctx.last_launch_count() == 1
        ctx.download(k3)
        bad = rc.mismatches(case, digests, values, case.nsteps, rc.hip_get(k3, case.nz))
        assert not bad, f"one launch, after step {case.nsteps}: {bad}"
        st, nf, npass = ctx.status()
        assert steps == [1, 2] and np.array_equal(st[act], ob["status"][act]) and np.array_equal(npass[act], ob["npasses"][act])
    else:
        for nt, _ in zip(range(1, case.nsteps + 1), rc.run_oracle(case, oc, ob)):
            ctx.step(nt, 1)
            ctx.download(k3)
            bad = rc.mismatches(case, digests, values, nt, rc.hip_get(k3, case.nz))
            assert not bad, f"a launch per step, after step {nt}: {bad}"
            st, nf, npass = ctx.status()
            assert np.array_equal(st[act], ob["status"][act]) and np.array_equal(npass[act], ob["npasses"][act])
    assert np.array_equal(k3.X[act, case.nz, 0], bt[act])
    ctx.close()


# ---------------------------------------------------------------------------
# 2. one launch = the oracle with the override after every step = a launch per step with ctx.bottomtemp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nz,grid,solver_mode", [(40, "uniform", 0), (40, "uniform", 1), (69, "stretched", 0)])
def test_one_launch_equals_the_oracle_and_the_host_override(mk, nz, grid, solver_mode):
    ncol, nsteps = 77, 6
    case = dict(grid=grid, land_every=6, solver_mode=solver_mode)
    ob, status, bts, active = _oracle(ncol, nz, nsteps, **case)
    bt = bts[0]
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    assert h.kernel_name == "k_column_ps"   # default physics: the correction rows come with set_bottomtemp
    h.set_bottomtemp(bt)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, ob, nz, active, f"one launch nz={nz} mode={solver_mode}")
    assert np.array_equal(k3.X[active, nz, 0], bt[active])
    land = np.nonzero(k3.run_physics == 0)[0]
    assert len(land) and np.all(k3.tinc_fcorr[land] == 0)
    one = _fields(k3, nz)
    h.close()
    # ocnTcorr(nzp1) is not zero in the step that first meets the field.  (Only then: ocnint leaves the bottom level as it
    # is, so from the second step on the override finds T(nzp1) = b already and its increment is zero - in the reference
    # too.  That is why this is asserted after a launch of one step, not after the six.)
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    h.set_bottomtemp(bt)
    h.step(1, 1)
    h.download(k3)
    assert np.all(k3.ocnTcorr[active, nz] != 0) and np.all(k3.tinc_fcorr[active, nz] != 0)
    assert np.all(one["ocnTcorr"][active, nz] == 0)
    h.close()
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    for nt in range(1, nsteps + 1):
        h.step(nt, 1)
        h.bottomtemp(bt)
    is_the_oracles(h, k3, ob, nz, active, f"launch per step + host override nz={nz} mode={solver_mode}")
    per_step = _fields(k3, nz)
    for n in rc.STEP_FIELDS:
        assert np.array_equal(one[n][active], per_step[n][active], equal_nan=True), n
    h.close()


# ---------------------------------------------------------------------------
# 3. the optional-physics kernel
# ---------------------------------------------------------------------------
OPTIONAL = {
    "fcorr_withz": dict(pre="fcorr_withz", L_FCORR_WITHZ=1),
    "relax_ocnt": dict(pre="relax_ocnt", L_RELAX_OCNT=1),
    "no_freeze": dict(pre="no_freeze", L_NO_FREEZE=1),
    "no_isotherm": dict(pre="isotherm", L_NO_ISOTHERM=1, clim_present=1, iso_bot=20, iso_thresh=0.002),
    "ldd": dict(pre="ldd", LDD=1),
}


@pytest.mark.parametrize("variant", list(OPTIONAL))
def test_optional_physics_kernels(mk, variant):
    """The override replaces tinc_fcorr(nzp1) and ocnTcorr(nzp1) that ocnint's corrections and the no-freeze clamp wrote
    in the same step, and follows check_profile's resets of T."""
    ncol, nz, nsteps = 70, 40, 4
    case = OPTIONAL[variant]
    ob, status, bts, active = _oracle(ncol, nz, nsteps, **case)
    if variant == "no_freeze":   # reach: the clamp fired on the columns that start below -1.8 at every level
        assert np.all(ob["freeze_flag"][::3] > 0) and np.all(ob["T"][::3, nz + 1] == bts[0][::3])
    if variant == "no_isotherm":
        assert any(np.any(r < 0) for r in ob.reset_flags)   # reach: an isotherm reset (of every level, the bottom one too)
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    assert h.kernel_name == "k_column_ps<EXT>"
    h.set_bottomtemp(bts[0])
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, ob, nz, active, variant)
    assert np.array_equal(k3.X[:, nz, 0], bts[0])
    h.close()


# ---------------------------------------------------------------------------
# 4. a retried step and a climatology reset
# ---------------------------------------------------------------------------
def test_a_retried_step_and_a_climatology_reset(mk):
    """Every third column starts with the 12 K temperature step of ref_step_cases: its steps are retried ten times and
    check_profile resets T and S to the climatology - the bottom level too - before the override replaces that level."""
    ncol, nz, nsteps = 60, 40, 3
    case = dict(pre="tjump_clim", clim_present=1)
    ob, status, bts, active = _oracle(ncol, nz, nsteps, **case)
    assert any(np.any(s & 4) for s in status[:-1])   # reach: a retried column-step in a step that is not the last
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    h.set_bottomtemp(bts[0])
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, ob, nz, active, "tjump + climatology")
    assert np.array_equal(k3.X[:, nz, 0], bts[0])
    h.close()


# ---------------------------------------------------------------------------
# 5. who does the work
# ---------------------------------------------------------------------------
FORMS = {
    "fewer_columns_than_slots": (64, 40, 20, {}),
    "launch_per_step": (77, 40, 6, {"MCKPP_MULTISTEP": "0"}),
    "stragglers_at_once": (77, 40, 6, {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}),
    "xcc_drop_0x55": (77, 40, 6, {"MCKPP_XCC_DROP": "0x55"}),
    "xcc_drop_0xfe": (77, 40, 6, {"MCKPP_XCC_DROP": "0xfe"}),
    "literal_levels_at_60": (77, 60, 6, {}),
    "general_kernel_at_60": (77, 60, 6, {"MCKPP_PS_FIXED_L": "0"}),
    "l3_cap_3": (77, 40, 6, {"MCKPP_L3_CAP": "3"}),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_forms(mk, monkeypatch, form):
    """Fewer columns than slots over twenty steps (every later ticket is drawn before its column is ready: the column
    goes on in its slot), every column past its first pass a straggler (the workgroups go into views, in which the item
    that finishes a column is not the one that ran its L1), XCDs that start without a queue, the general kernel against
    the literal-level one, and the scan's second round on every pass."""
    ncol, nz, nsteps, env = FORMS[form]
    ob, status, bts, active = _oracle(ncol, nz, nsteps, land_every=6)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, kc, k3 = _hip(mk, ncol, nz, land_every=6)
    h.set_bottomtemp(bts[0])
    h.step(1, nsteps)
    assert h.last_launch_count() == (nsteps if form == "launch_per_step" else 1)
    is_the_oracles(h, k3, ob, nz, active, form)
    assert np.array_equal(k3.X[active, nz, 0], bts[0][active])
    h.close()


# ---------------------------------------------------------------------------
# 6. a new field between launches; cancelling
# ---------------------------------------------------------------------------
def test_a_new_field_between_launches_and_none(mk):
    """set_bottomtemp(bt1), step(1, 3), set_bottomtemp(bt2), step(4, 3): the oracle with the same change.  Then
    set_bottomtemp(None) and one more step: the oracle's plain step from that state."""
    from oracle import orc

    ncol, nz = 77, 40
    oc, ob, kc, k3 = _both(ncol, nz, land_every=6)
    active = np.nonzero(k3.run_physics)[0]
    orc.init_ocean(oc, ob, 0)
    bts = [_bt(ob, nz), _bt(ob, nz, seed=5) + 0.3]
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    for nt in range(1, 7):
        orc.physics_driver(oc, ob, nt)
        orc.bottomtemp(oc, ob, bts[1] if nt >= 4 else bts[0])
    h, kc, k3 = _hip(mk, ncol, nz, land_every=6)
    h.set_bottomtemp(bts[0])
    h.step(1, 3)
    h.set_bottomtemp(bts[1])
    h.step(4, 3)
    is_the_oracles(h, k3, ob, nz, active, "bt1 for steps 1-3, bt2 for steps 4-6")
    assert np.array_equal(k3.X[active, nz, 0], bts[1][active])
    h.set_bottomtemp(None)
    h.step(7, 1)
    orc.physics_driver(oc, ob, 7)
    h.download(k3)
    st, nf, npass = h.status()
    assert np.array_equal(st[active], ob["status"][active]) and np.array_equal(npass[active], ob["npasses"][active])
    # (a plain default-physics step leaves the correction rows alone, the oracle's ocnint rewrites them: not compared)
    plain = [n for n in rc.STEP_FIELDS if n not in ("tinc_fcorr", "ocnTcorr")]
    bad = {k: v for k, v in cm.compare(k3, ob, nz, plain, active).items() if v[2] != 0}
    assert not bad, f"after set_bottomtemp(None): {bad}"
    h.bottomtemp(bts[0])   # ... and the host's override is allowed again
    h.close()


# ---------------------------------------------------------------------------
# 7. beside the schedules, in one forced run
# ---------------------------------------------------------------------------
def test_beside_window_restart_and_log_schedules(mk, tmp_path):
    """run_forced of 8 steps from a flux series, with a resident bottom temperature, a window schedule of period 2 on T,
    tinc_fcorr and fcorr_z, a restart schedule of period 2 and a step log: the window records are window_accumulate's
    after each step + bottomtemp of a launch-per-step run, the snapshot files are save_restart's of that run stopped
    there byte for byte, the log's records are the oracle's."""
    from oracle import orc

    A = mk.api
    ncol, nz, nsteps, ndtocn, min_passes = 77, 40, 8, 2, 6
    rng = np.random.default_rng(23)
    series = np.empty((nsteps // ndtocn, 8, ncol))
    for r in range(series.shape[0]):
        series[r] = [rng.uniform(-0.2, 0.3, ncol), rng.uniform(-0.1, 0.1, ncol), 300.0 * r * np.ones(ncol),
                     rng.uniform(-80, -20, ncol), rng.uniform(-300, 0, ncol), rng.uniform(-40, 10, ncol),
                     rng.uniform(0, 1e-4, ncol), np.zeros(ncol)]
    oc, ob, kc, k3 = _both(ncol, nz, land_every=6)
    active = np.nonzero(k3.run_physics)[0]
    orc.init_ocean(oc, ob, 0)
    bt = _bt(ob, nz)
    want = []
    for nt in range(1, nsteps + 1):
        if (nt - 1) % ndtocn == 0:
            orc.fluxes(oc, ob, nt, **dict(zip(cm.synth.FLUX_NAMES, series[(nt - 1) // ndtocn])))
        orc.physics_driver(oc, ob, nt)
        orc.bottomtemp(oc, ob, bt)
        st, npass = ob["status"], ob["npasses"]
        want += [(nt, int(c), int(st[c]), int(npass[c])) for c in active if st[c] != 0 or npass[c] >= min_passes]
    assert any(e[2] == 0 for e in want) and any(e[0] < nsteps for e in want)   # pass-count events, in steps before the last
    names = ("T", "tinc_fcorr", "fcorr_z")
    ops = ((A.OP_MEAN, A.OP_MEAN), (A.OP_MAX, A.OP_MAX), (A.OP_LAST, A.OP_INSTANT))   # (of a record, of the per-step window)

    def start():
        _, _, kc, k3 = _both(ncol, nz, land_every=6)
        h = mk.MckppHip(kc)
        h.upload(k3)
        h.init_ocean(0)
        h.set_flux_series(0, series)
        return h, kc, k3

    # a launch per step with the host's override: windows accumulated by the host's calls, restart files at steps 2, 4, ..
    h, kc, k3 = start()
    h.window_select([A.OUT_FIELDS.index(n) for n in names])
    ref_rec, ref_files = {}, []
    for nt in range(1, nsteps + 1):
        if nt % 2 == 1:
            h.window_reset()
        h.run_forced(nt, 1, ndtocn)
        h.bottomtemp(bt)
        h.window_accumulate()
        if nt % 2 == 0:
            for n in names:
                for rop, pop in ops:
                    ref_rec[nt // 2 - 1, n, rop] = h.window_fetch(A.OUT_FIELDS.index(n), pop, np.full((ncol, kc.nzp1), -7.0, order="F")).copy()
            ref_files.append(tmp_path / f"ref{nt}")
            h.save_restart(ref_files[-1])
    h.close()

    # one launch with the resident field under the three schedules
    h, kc, k3 = start()
    h.set_bottomtemp(bt)
    h.window_schedule(0, 1, 2, nsteps // 2, names, A.WIN_MEAN | A.WIN_MAX | A.WIN_LAST)
    h.restart_schedule(1, 2, nsteps // 2)
    h.step_log(nsteps * ncol, min_passes)
    h.run_forced(1, nsteps, ndtocn)
    assert h.last_launch_count() == 1
    for (w, n, rop), ref in ref_rec.items():
        got = h.window_record_fetch(0, w, n, rop, np.full((ncol, kc.nzp1), -7.0, order="F"))
        assert np.array_equal(got, ref, equal_nan=True), (w, n, rop)
    # (the override's increment is in the records: not zero in the window of the step that first meets the field)
    assert np.all(ref_rec[0, "tinc_fcorr", A.OP_MEAN][active, nz] != 0) and np.all(ref_rec[0, "fcorr_z", A.OP_MEAN][active, nz] != 0)
    for s, ref in enumerate(ref_files):
        f = tmp_path / f"snap{s}"
        h.restart_snapshot_save(s, f)
        assert open(f, "rb").read() == open(ref, "rb").read(), f"snapshot {s}"
    nt_, pt, st, npass = h.step_log_fetch()
    assert list(zip(nt_.tolist(), pt.tolist(), st.tolist(), npass.tolist())) == want
    is_the_oracles(h, k3, ob, nz, active, "beside the schedules")
    h.close()


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals_and_upload_cancels(mk):
    from oracle import orc

    ncol, nz = 77, 40
    ob, status, bts, active = _oracle(ncol, nz, 6, land_every=6)
    h, kc, k3 = _hip(mk, ncol, nz, land_every=6)
    h.set_bottomtemp(bts[0])
    with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_bottomtemp: a bottom temperature is resident.*drop\s+this call"):
        h.bottomtemp(bts[0])
    before = _fields_of(h, k3, nz)
    h.set_diagnostics(0)
    for call in (lambda: h.step(1, 1), lambda: h.step(1, 3)):
        with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_step: a bottom temperature is resident.*diagnostics are switched off"):
            call()
    h.set_diagnostics(1)
    after = _fields_of(h, k3, nz)
    for n in rc.STEP_FIELDS:   # nothing was launched
        assert np.array_equal(before[n], after[n], equal_nan=True), n
    # after an upload nothing is resident: a step is a plain step
    h.upload(k3)
    h.set_forcing(k3.sflux)
    h.step(1, 1)
    oc, ob1, _, _ = _both(ncol, nz, land_every=6)
    orc.init_ocean(oc, ob1, 0)
    ob1["sflux"] = cm.synth.forcing(ncol, "bench")
    orc.physics_driver(oc, ob1, 1)
    h.download(k3)
    plain = [n for n in rc.STEP_FIELDS if n not in ("tinc_fcorr", "ocnTcorr")]
    bad = {k: v for k, v in cm.compare(k3, ob1, nz, plain, active).items() if v[2] != 0}
    assert not bad, f"a step after upload: {bad}"
    assert np.all(k3.X[active, nz, 0] != bts[0][active])
    h.bottomtemp(bts[0])   # not refused: nothing is resident
    h.close()


def _fields_of(h, k3, nz):
    h.download(k3)
    return _fields(k3, nz)


# ---------------------------------------------------------------------------
# 9. several shards
# ---------------------------------------------------------------------------
def test_three_shards_equal_the_single_context(mk):
    ncol, nz, nsteps = 77, 40, 6
    ob, status, bts, active = _oracle(ncol, nz, nsteps, land_every=6)
    h, kc, k3 = _hip(mk, ncol, nz, shards=3, land_every=6)
    h.set_bottomtemp(bts[0])
    h.step(1, nsteps)
    h.synchronize()
    is_the_oracles(h, k3, ob, nz, active, "3 shards")
    multi = _fields(k3, nz)
    h.set_bottomtemp(None)
    h.close()
    h, kc, k3 = _hip(mk, ncol, nz, land_every=6)
    h.set_bottomtemp(bts[0])
    h.step(1, nsteps)
    single = _fields_of(h, k3, nz)
    for n in rc.STEP_FIELDS:
        assert np.array_equal(multi[n][active], single[n][active], equal_nan=True), n
    h.close()
