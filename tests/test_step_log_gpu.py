"""The step log (mckpp_hip_step_log): with a log set, every MCKPP_MODE_STEP launch leaves a record {nt, point, status,
npasses} for each column-step that ends with a non-zero status word or with at least min_passes passes, so that the
flags and pass counts of the steps inside a launch of several steps are not lost.

The expected records always come from the CPU oracle run step by step (status and pass counts read after each step,
portable-exp mode), never from the library; every test also holds the end state, the status words and the pass counts of
the last step to the oracle's, bit for bit."""
import functools

import numpy as np
import pytest

import common as cm
from harness import cleared, force_bench, initialised, is_the_oracles, mk  # noqa: F401

pytestmark = pytest.mark.gpu

ALL_FIELDS = cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["hmixd0", "hmixd1"] + list(cm.DIAG_FIELDS.keys())
ENV = ("MCKPP_MULTISTEP", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT", "MCKPP_XCC_DROP", "MCKPP_PS_FIXED_L")
_clean_env = cleared(ENV)


# ---------------------------------------------------------------------------
# the cases: the same set-up on both sides
# ---------------------------------------------------------------------------
def _prep_none(k3, ob):
    pass


def _prep_relax_sst(k3, ob):
    r = np.full(k3.npts, 1.0 / (5 * 86400.0))
    r[::4] = 0.0
    k3.relax_sst[:] = r
    ob["relax_sst"] = r
    sst = np.asarray(k3.X[:, 0, 0]) + 1.5
    k3.SST0[:] = sst
    ob["SST0"] = sst


def _prep_ldd(k3, ob):
    nzp1 = k3.X.shape[1]
    S = np.asarray(k3.X[:, :, 1]).copy()
    S[::2] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
    k3.X[:, :, 1] = S
    ob.a["S"][:, 1:nzp1 + 1] = S


def _prep_trap(k3, ob):   # test_instability_trap_retry_and_reset: U = 50 in the top four levels of every 7th column
    bad = np.arange(0, k3.npts, 7)
    k3.U[bad, 0:4, 0] = 50.0
    ob["U"][bad, 1:5] = 50.0


PREP = {"none": _prep_none, "relax_sst": _prep_relax_sst, "ldd": _prep_ldd, "trap": _prep_trap}


def _both(ncol, nz, itermax=200, land_every=7, prep="none", prep_after_init=False, solver_mode=None, tri_nz=None, **switches):
    """Oracle const + batch and the HIP side's constants + fields of one case, before initialisation."""
    oc, ob, kc, k3 = cm.make_both(ncol, nz, "uniform", land_every, solver_mode, itermax, **switches)
    if tri_nz is not None:   # test_zero_pivot_on_device, last level: cc(nz) = 1 + (-1e4)(1e-4) + 0 = 0
        kc.tri[nz, 0, 0], kc.tri[nz, 1, 0] = 0.0, tri_nz
        oc.tri0[nz], oc.tri1[nz] = 0.0, tri_nz
    if not prep_after_init:
        PREP[prep](k3, ob)
    return oc, ob, kc, k3


def _events(ob, nt, active, min_passes):
    st, npass = ob["status"], ob["npasses"]
    return [(nt, int(c), int(st[c]), int(npass[c])) for c in active
            if st[c] != 0 or (min_passes > 0 and npass[c] >= min_passes)]


@functools.lru_cache(maxsize=None)
def _oracle(ncol, nz, nsteps, min_passes=0, **case):
    """The oracle's run of a case, step by step, once per case: (events of each step as lists of (nt, point, status,
    npasses) in point order, the batch after the last step, the active points).  Shared and left unchanged."""
    from oracle import orc

    case = dict(case)
    oc, ob, kc, k3 = _both(ncol, nz, **case)
    active = np.nonzero(k3.run_physics)[0]
    orc.init_ocean(oc, ob, 0)
    if case.get("prep_after_init"):
        PREP[case["prep"]](k3, ob)
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    per_step = []
    for nt in range(1, nsteps + 1):
        orc.physics_driver(oc, ob, nt)
        per_step.append(_events(ob, nt, active, min_passes))
    return per_step, ob, active


def _hip(mk, ncol, nz, shards=0, **case):
    """The HIP side of the same case, initialised and forced, ready to step."""
    case = dict(case)
    oc, ob, kc, k3 = _both(ncol, nz, **case)
    h = initialised(mk, kc, k3, shards)
    if case.get("prep_after_init"):
        h.download(k3)
        PREP[case["prep"]](k3, ob)
        h.upload(k3)
    if case.get("solver_mode") is not None:
        h.set_solver_mode(case["solver_mode"])
    force_bench(h, k3)
    return h, kc, k3


def _records(h):
    nt, pt, st, npass = h.step_log_fetch()
    assert all(a.dtype == np.int32 for a in (nt, pt, st, npass))
    return list(zip(nt.tolist(), pt.tolist(), st.tolist(), npass.tolist()))


def _flat(per_step):
    return [e for step in per_step for e in step]


def _status_or(events):
    return int(np.bitwise_or.reduce([e[2] for e in events] or [0]))


_end_state_is_the_oracles = functools.partial(is_the_oracles, fields=ALL_FIELDS)


CASE1 = dict(itermax=4)   # bench forcing from the analytic start, land_every = 7: point != resident column


# ---------------------------------------------------------------------------
# 1. flags of a step that is not the last one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nz,kernel", [(40, "general"), (60, "literal level count")])
def test_flags_of_steps_inside_a_launch(mk, nz, kernel):
    """itermax = 4, step(1, 3) as one launch: the fetched records are the oracle's list over the three steps, exactly
    and in order.  status() after the launch shows step 3 only - what the log is for."""
    from oracle import orc

    ncol = 120
    per_step, ob, active = _oracle(ncol, nz, 3, **CASE1)
    want = _flat(per_step)
    # reach: a flagged column-step before the last step, and an unflagged column-step
    assert sum(len(s) for s in per_step[:-1]) > 0 and len(want) < 3 * len(active)
    assert all(e[2] & orc.ST_LONG_ITER for e in want)
    assert len(active) < ncol and np.any(active != np.arange(len(active)))   # point != resident column
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(3 * ncol)
    assert h.step_logged == (3 * ncol, 0) and h.step_log_count() == (0, 0, 0)
    h.step(1, 3)
    assert h.last_launch_count() == 1
    assert h.step_log_count() == (len(want), len(want), _status_or(want))
    assert _records(h) == want
    assert _records(h) == want   # (fetch does not clear)
    _end_state_is_the_oracles(h, k3, ob, nz, active, f"nz={nz}")
    h.close()


# ---------------------------------------------------------------------------
# 2. pass-count events
# ---------------------------------------------------------------------------
def test_pass_count_events(mk):
    """itermax = 200, min_passes = 13, step(1, 4) in one launch: the records are the oracle's column-steps with at least
    13 passes or a status; with min_passes = 0 the same run logs nothing."""
    ncol, nz, nsteps = 200, 60, 4
    per_step, ob, active = _oracle(ncol, nz, nsteps, min_passes=13)
    want = _flat(per_step)
    # reach: a record with status 0, every record in a step that is not the last, fewer records than column-steps
    assert any(e[2] == 0 for e in want) and not per_step[-1] and 0 < len(want) < nsteps * len(active)
    assert all(e[3] >= 13 or e[2] != 0 for e in want)
    for min_passes, expect in ((13, want), (0, [e for e in want if e[2] != 0])):
        h, kc, k3 = _hip(mk, ncol, nz)
        h.step_log(nsteps * ncol, min_passes)
        h.step(1, nsteps)
        assert h.last_launch_count() == 1
        assert _records(h) == expect, min_passes
        assert h.step_log_count() == (len(expect), len(expect), _status_or(expect))
        _end_state_is_the_oracles(h, k3, ob, nz, active, f"min_passes={min_passes}")
        h.close()
    assert [e for e in want if e[2] != 0] == []   # (min_passes = 0 logged nothing)


# ---------------------------------------------------------------------------
# 3. the instability trap and its retries
# ---------------------------------------------------------------------------
def test_a_retried_column_step_is_one_record(mk):
    """U = 50 on every 7th column: step 1 of those columns is retried ten times and reset (bits 4 and 8).  One record per
    flagged column-step, status and passes accumulated over the tries as the oracle's are."""
    ncol, nz = 70, 40
    case = dict(land_every=0, prep="trap", prep_after_init=True)
    per_step, ob, active = _oracle(ncol, nz, 3, **case)
    want = _flat(per_step)
    bad = list(range(0, ncol, 7))
    assert [e[1] for e in per_step[0]] == bad and all(e[2] & 12 == 12 for e in per_step[0])
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    h.step_log(3 * ncol)
    h.step(1, 3)
    assert h.last_launch_count() == 1
    got = _records(h)
    assert len({(e[0], e[1]) for e in got}) == len(got)   # one record per column-step
    assert got == want
    _end_state_is_the_oracles(h, k3, ob, nz, active, "trap")
    h.close()


# ---------------------------------------------------------------------------
# 4. zero pivot
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver_mode", [0, 1])
def test_zero_pivot_inside_a_launch(mk, solver_mode):
    """tri(nz) crafted so that the last pivot of the momentum system vanishes, steps 1-2 in one launch: the records are
    the oracle's and the OR of the status words carries MCKPP_ST_ZERO_PIVOT."""
    from oracle import orc

    ncol, nz = 70, 60
    case = dict(land_every=0, tri_nz=-1.0e4, solver_mode=solver_mode)
    per_step, ob, active = _oracle(ncol, nz, 2, **case)
    want = _flat(per_step)
    assert any(e[2] & orc.ST_ZERO_PIVOT for e in per_step[0])   # reach: a zero pivot in the step that is not the last
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    h.step_log(2 * ncol)
    h.step(1, 2)
    assert h.last_launch_count() == 1
    assert _records(h) == want
    n_events, n_stored, status_or = h.step_log_count()
    assert (n_events, n_stored) == (len(want), len(want))
    assert status_or & orc.ST_ZERO_PIVOT and status_or == _status_or(want)
    _end_state_is_the_oracles(h, k3, ob, nz, active, f"zero pivot, solver mode {solver_mode}")
    h.close()


# ---------------------------------------------------------------------------
# 5. overflow
# ---------------------------------------------------------------------------
def test_overflow_keeps_the_count_and_the_or(mk):
    """Case 1 at 40 levels with room for 16 records: the count and the OR stay exact, the 16 stored records are distinct
    records of the oracle's list, and the run itself is untouched."""
    ncol, nz = 120, 40
    per_step, ob, active = _oracle(ncol, nz, 3, **CASE1)
    want = _flat(per_step)
    assert len(want) > 16
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(16)
    h.step(1, 3)
    assert h.step_log_count() == (len(want), 16, _status_or(want))
    got = _records(h)
    assert len(got) == 16 and len(set(got)) == 16 and set(got) <= set(want)
    assert got == sorted(got)
    _end_state_is_the_oracles(h, k3, ob, nz, active, "overflow")
    h.close()


# ---------------------------------------------------------------------------
# 6. across launches, clear, cancel
# ---------------------------------------------------------------------------
def test_the_log_spans_launches_until_it_is_cleared(mk):
    ncol, nz = 120, 40
    per_step, ob, active = _oracle(ncol, nz, 3, **CASE1)
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(3 * ncol)
    h.step(1, 2)
    h.step(3, 1)
    assert _records(h) == _flat(per_step)
    h.close()
    # cleared after the first launch: a further step logs only its own
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(3 * ncol)
    h.step(1, 2)
    assert _records(h) == _flat(per_step[:2])
    h.step_log_clear()
    assert h.step_log_count() == (0, 0, 0) and _records(h) == []
    h.step(3, 1)
    assert _records(h) == per_step[2]
    assert h.step_log_count() == (len(per_step[2]), len(per_step[2]), _status_or(per_step[2]))
    _end_state_is_the_oracles(h, k3, ob, nz, active, "across launches")
    # cancelled: count fails with a message; so does everything else that needs a log
    h.step_log(0)
    assert h.step_logged is None
    for call in (h.step_log_count, h.step_log_fetch, h.step_log_clear):
        with pytest.raises(mk.MckppHipError, match=r"no step log is set"):
            call()
    # upload cancels
    h.step_log(8)
    assert h.step_logged == (8, 0)
    h.upload(k3)
    assert h.step_logged is None
    with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_step_log_count: no step log is set"):
        h.step_log_count()
    with pytest.raises(mk.MckppHipError, match=r"capacity=-1"):
        mk.api._chk(mk.api._lib().mckpp_hip_step_log(h._h, -1, 0))
    with pytest.raises(mk.MckppHipError, match=r"min_passes=-2"):
        mk.api._chk(mk.api._lib().mckpp_hip_step_log(h._h, 4, -2))
    h.close()


# ---------------------------------------------------------------------------
# 7. launch forms that change who does the work
# ---------------------------------------------------------------------------
FORMS = {
    "launch_per_step": {"MCKPP_MULTISTEP": "0"},
    "stragglers_at_once": {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"},
    "xcc_drop_0x55": {"MCKPP_XCC_DROP": "0x55"},
    "xcc_drop_0xfe": {"MCKPP_XCC_DROP": "0xfe"},
    "general_kernel_at_60": {"MCKPP_PS_FIXED_L": "0"},
}


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_forms(mk, monkeypatch, form):
    """Case 1 at 60 levels with a launch per step, with every column past its first pass a straggler, with XCDs that
    start without a queue, and through the general kernel: the records are the oracle's in every form."""
    ncol, nz = 120, 60
    per_step, ob, active = _oracle(ncol, nz, 3, **CASE1)
    want = _flat(per_step)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(3 * ncol)
    h.step(1, 3)
    assert h.last_launch_count() == (3 if form == "launch_per_step" else 1)
    assert _records(h) == want
    assert h.step_log_count() == (len(want), len(want), _status_or(want))
    _end_state_is_the_oracles(h, k3, ob, nz, active, form)
    h.close()


def test_fewer_columns_than_slots_over_twenty_steps(mk):
    ncol, nz, nsteps = 64, 60, 20
    per_step, ob, active = _oracle(ncol, nz, nsteps, **CASE1)
    want = _flat(per_step)
    assert 0 < len(want) < nsteps * len(active)
    h, kc, k3 = _hip(mk, ncol, nz, **CASE1)
    h.step_log(nsteps * ncol)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    assert _records(h) == want
    _end_state_is_the_oracles(h, k3, ob, nz, active, "64 columns x 20 steps")
    h.close()


@pytest.mark.parametrize("variant", ["relax_sst", "ldd"])
def test_optional_physics_kernels_log_too(mk, variant):
    """The optional-physics build (SST relaxation on) and the double-diffusion build, case 1 at 60 levels."""
    ncol, nz = 120, 60
    case = dict(CASE1, prep=variant, **(dict(L_RELAX_SST=1) if variant == "relax_sst" else dict(LDD=1)))
    per_step, ob, active = _oracle(ncol, nz, 3, **case)
    want = _flat(per_step)
    assert 0 < len(want) < 3 * len(active)
    h, kc, k3 = _hip(mk, ncol, nz, **case)
    if variant == "relax_sst":
        assert h.kernel_name == "k_column_ps<EXT>"
    h.step_log(3 * ncol)
    h.step(1, 3)
    assert h.last_launch_count() == 1
    assert _records(h) == want
    _end_state_is_the_oracles(h, k3, ob, nz, active, variant)
    h.close()


# ---------------------------------------------------------------------------
# 8. beside the schedules
# ---------------------------------------------------------------------------
def test_the_log_beside_output_and_restart_schedules(mk, tmp_path):
    """run_forced of 6 steps from a flux series with an output schedule (period 2), a restart schedule (period 3) and the
    log together: window records and snapshot files are what they are without the log, the records are the oracle's."""
    from oracle import orc

    A = mk.api
    ncol, nz, nsteps, ndtocn = 120, 40, 6, 2
    rng = np.random.default_rng(11)
    series = np.empty((nsteps // ndtocn, 8, ncol))
    for r in range(series.shape[0]):
        series[r] = [rng.uniform(-0.2, 0.3, ncol), rng.uniform(-0.1, 0.1, ncol), 400.0 * r * np.ones(ncol),
                     rng.uniform(-80, -20, ncol), rng.uniform(-300, 0, ncol), rng.uniform(-40, 10, ncol),
                     rng.uniform(0, 1e-4, ncol), np.zeros(ncol)]
    oc, ob, kc, k3 = _both(ncol, nz, **CASE1)
    active = np.nonzero(k3.run_physics)[0]
    orc.init_ocean(oc, ob, 0)
    want = []
    for nt in range(1, nsteps + 1):
        if (nt - 1) % ndtocn == 0:
            orc.fluxes(oc, ob, nt, **dict(zip(cm.synth.FLUX_NAMES, series[(nt - 1) // ndtocn])))
        orc.physics_driver(oc, ob, nt)
        want += _events(ob, nt, active, 0)
    assert 0 < len(want) < nsteps * len(active) and any(e[0] < nsteps for e in want)

    def run(log):
        _, _, kc, k3 = _both(ncol, nz, **CASE1)
        h = mk.MckppHip(kc)
        h.upload(k3)
        h.init_ocean(0)
        h.set_flux_series(0, series)
        h.window_schedule(0, 1, 2, 3, ("T", "hmix"), A.WIN_MEAN | A.WIN_MAX)
        h.restart_schedule(1, 3, 2)
        if log:
            h.step_log(nsteps * ncol)
        h.run_forced(1, nsteps, ndtocn)
        assert h.last_launch_count() == 1
        rec = {}
        for w in range(3):
            for n in ("T", "hmix"):
                for op in (A.OP_MEAN, A.OP_MAX):
                    shape = (ncol,) if n == "hmix" else (ncol, kc.nzp1)
                    rec[w, n, op] = h.window_record_fetch(0, w, n, op, np.full(shape, -7.0, order="F")).copy()
        files = []
        for s in range(2):
            files.append(tmp_path / f"snap{s}_{int(log)}")
            h.restart_snapshot_save(s, files[-1])
        got = _records(h) if log else None
        if log:
            _end_state_is_the_oracles(h, k3, ob, nz, active, "beside the schedules")
        h.close()
        return rec, files, got

    rec0, files0, _ = run(False)
    rec1, files1, got = run(True)
    assert got == want
    assert rec0.keys() == rec1.keys()
    for key in rec0:
        assert np.array_equal(rec0[key], rec1[key], equal_nan=True), key
    for a, b in zip(files0, files1):
        assert open(a, "rb").read() == open(b, "rb").read()


# ---------------------------------------------------------------------------
# 9. several shards
# ---------------------------------------------------------------------------
def test_shards_report_the_callers_points(mk):
    """MckppHipMulti(kc, [0, 0, 0]), case 1 at 40 levels with land: the merged records name the caller's points - the
    list of the single context, the oracle's."""
    ncol, nz = 120, 40
    per_step, ob, active = _oracle(ncol, nz, 3, **CASE1)
    want = _flat(per_step)
    h, kc, k3 = _hip(mk, ncol, nz, shards=3, **CASE1)
    h.step_log(3 * ncol)
    h.step(1, 3)
    h.synchronize()
    assert h.step_log_count() == (len(want), len(want), _status_or(want))
    assert _records(h) == want
    _end_state_is_the_oracles(h, k3, ob, nz, active, "3 shards")
    h.step_log_clear()
    assert h.step_log_count() == (0, 0, 0)
    h.step_log(0)
    with pytest.raises(mk.MckppHipError, match=r"no step log is set"):
        h.step_log_count()
    h.close()
