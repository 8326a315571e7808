"""Ancillary record series (mckpp_hip_set_ancillary_series, mckpp_hip_ancillary_schedule): what mckpp_boundary_update
rewrites at the ndtupd* cadences (src/mckpp_boundary_update_mod.F90:24-124) and what mckpp_boundary_interpolate forms
from two records (src/mckpp_boundary_interpolate.F90:14-121), read by every column-step from immutable resident records
through the epoch of the step it is in - so a forced run under such updates is one launch.

What is expected never comes from the code under test.  It is the CPU oracle stepped one step at a time with the epoch's
field written into its state before the step, an interpolated field formed in numpy as nxt*wn + prv*wp
(tests/anc_cases.py); and the library's earlier way: launches cut at every epoch boundary with update_ancillaries /
set_bottomtemp between them.  Every case holds every field of STEP_FIELDS (those of tests/common.py, fcorr, tinc_fcorr,
ocnTcorr, sinc_fcorr and scorr among them), the status words and the pass counts to equality, over the columns that are
stepped."""
import numpy as np
import pytest

import anc_cases as ac
import common as cm
import ref_step_cases as rc
from harness import cleared, force_bench, initialised, is_the_oracles, mk  # noqa: F401
from mckpp_f90_amd import api as A

pytestmark = pytest.mark.gpu

ENV = ("MCKPP_MULTISTEP", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT", "MCKPP_XCC_DROP", "MCKPP_PS_FIXED_L", "MCKPP_L3_CAP")
NCOL, NZ, NSTEPS = 96, 40, 12
_clean_env = cleared(ENV)


# ---------------------------------------------------------------------------
# the HIP side
# ---------------------------------------------------------------------------
def _hip(mk, ncol, nz, shards=0, series=None, **case):
    """The HIP side of a case, initialised and forced (bench forcing, or a resident flux series), ready to step."""
    oc, ob, kc, k3, TS = ac.both(ncol, nz, **case)
    h = initialised(mk, kc, k3, shards)
    if case.get("solver_mode") is not None:
        h.set_solver_mode(case["solver_mode"])
    if series is None:
        force_bench(h, k3)
    else:
        h.set_flux_series(0, series)
    return h, kc, k3


def _as_series(name, recs):
    """[nrec, ncol(, nzp1)] -> the layout of set_ancillary_series: [nrec, npts] or [nrec, nzp1, npts]"""
    return np.ascontiguousarray(recs.transpose(0, 2, 1)) if ac.KINDS[name][2] else np.ascontiguousarray(recs)


def _schedule(h, sched, recs, origin=1):
    for n, (cad, ep) in sched.items():
        h.set_ancillary_series(ac.KINDS[n][0], 0, _as_series(n, recs[n]))
        h.ancillary_schedule(ac.KINDS[n][0], origin, cad, ep)


def _fields(h, k3, nz):
    h.download(k3)
    return {n: np.array(rc.hip_get(k3, nz)(n)) for n in rc.STEP_FIELDS}


def _same(a, b, active, tag):
    for n in rc.STEP_FIELDS:
        assert np.array_equal(a[n][active], b[n][active], equal_nan=True), (tag, n)


def _put_hip_field(h, k3, name, f):
    """the library's earlier way of changing a field between launches"""
    if name == "bottom_temp":
        h.set_bottomtemp(f)
    else:
        getattr(k3, ac.KINDS[name][1])[...] = f
        h.update_ancillaries(k3)


def _cut_launches(h, k3, sched, recs, nsteps, run=None):
    """Launches cut at every epoch boundary of any kind, with update_ancillaries / set_bottomtemp in between."""
    run = run or (lambda nt, n: h.step(nt, n))
    cuts = sorted({nt for cad, ep in sched.values() for nt in range(1, nsteps + 1, cad)} | {nsteps + 1})
    for a, b in zip(cuts[:-1], cuts[1:]):
        for n, (cad, ep) in sched.items():
            if (a - 1) % cad == 0:
                _put_hip_field(h, k3, n, ac.field_at(recs[n], cad, ep, a))
        run(a, b - a)


# ---------------------------------------------------------------------------
# 1. each kind alone, stepwise, cadence 3, one launch of 12 steps
# ---------------------------------------------------------------------------
ALONE = {
    "relax_sst": ("SST0", dict(L_RELAX_SST=1)),
    "relax_sst_calconly": ("SST0", dict(L_RELAX_SST=1, L_RELAX_CALCONLY=1)),
    "fcorr": ("fcorr_twod", dict(L_FCORR=1)),
    "fcorr_withz": ("fcorr_withz", dict(L_FCORR_WITHZ=1)),
    "sfcorr_withz": ("sfcorr_withz", dict(L_SFCORR_WITHZ=1)),
    "relax_ocnt": ("ocnT_clim", dict(L_RELAX_OCNT=1)),
    "relax_sal": ("sal_clim", dict(L_RELAX_SAL=1)),
    "bottom_temp": ("bottom_temp", dict()),
}


@pytest.mark.parametrize("case", list(ALONE))
def test_each_kind_alone_stepwise(mk, case):
    name, sw = ALONE[case]
    sched = {name: (3, ac.stepwise(3, NSTEPS))}
    assert ac.nrec_of(sched[name][1]) == 4
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), **sw)
    held = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), hold_record0=True, **sw)
    assert ac.differs_on(want.ob, held.ob, NZ, want.active).all()   # reach: the later records are read, on every ocean column
    h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
    _schedule(h, sched, want.recs)
    h.step(1, NSTEPS)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, want.ob, NZ, want.active, case)
    one = _fields(h, k3, NZ)
    h.close()
    h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
    _cut_launches(h, k3, sched, want.recs, NSTEPS)
    _same(one, _fields(h, k3, NZ), want.active, case + ": cut launches")
    h.close()


# ---------------------------------------------------------------------------
# 2. interpolated climatologies, cadence 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["interpolated", "mixed"])
@pytest.mark.parametrize("nz,grid,env", [(40, "uniform", {}), (69, "stretched", {}), (60, "uniform", {}),
                                          (60, "uniform", {"MCKPP_PS_FIXED_L": "0"})])
def test_interpolated_climatologies_every_step(mk, monkeypatch, table, nz, grid, env):
    """Every step has its own pair and weights: 0 and 1, and weights whose products are inexact; and interpolated and
    stepwise epochs in one table.  At 40 levels, 69 stretched levels, and 60 levels with the literal-level-count kernel
    and with the general one."""
    ep = getattr(ac, table)(NSTEPS)
    sched = {"ocnT_clim": (1, ep), "sal_clim": (1, ep[::-1] if table == "interpolated" else ep)}
    sw = dict(L_RELAX_OCNT=1, L_RELAX_SAL=1, grid=grid)
    want = ac.oracle_run(NCOL, nz, NSTEPS, ac.key(sched), **sw)
    held = ac.oracle_run(NCOL, nz, NSTEPS, ac.key(sched), hold_record0=True, **sw)
    assert ac.differs_on(want.ob, held.ob, nz, want.active).all()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, kc, k3 = _hip(mk, NCOL, nz, **sw)
    _schedule(h, sched, want.recs)
    h.step(1, NSTEPS)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, want.ob, nz, want.active, f"{table} nz={nz} {env}")
    h.close()


# ---------------------------------------------------------------------------
# 3. all seven kinds at once
# ---------------------------------------------------------------------------
# (L_RELAX_SST and L_FCORR exclude each other in ocnint (ocnint_mod.F90:97, :121), as do L_FCORR_WITHZ and either: SST0
# and fcorr_twod are scheduled and resident all the same, read or not, and the three-dimensional kinds are all read)
ALL7 = {"SST0": (1, ac.stepwise(1, NSTEPS)), "fcorr_twod": (2, ac.stepwise(2, NSTEPS)),
        "fcorr_withz": (3, ac.stepwise(3, NSTEPS)), "sfcorr_withz": (4, ac.stepwise(4, NSTEPS)),
        "ocnT_clim": (1, ac.interpolated(NSTEPS)), "sal_clim": (6, ((0, 1, 0.25, 0.75), 1)),
        "bottom_temp": (2, ac.stepwise(2, NSTEPS))}
ALL7_SW = dict(L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1, L_RELAX_OCNT=1, L_RELAX_SAL=1, L_RELAX_SST=1)


@pytest.mark.parametrize("solver_mode", [0, 1])
@pytest.mark.parametrize("shards", [0, 3])
def test_all_seven_kinds_different_cadences(mk, solver_mode, shards):
    sw = dict(ALL7_SW, solver_mode=solver_mode)
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(ALL7), **sw)
    h, kc, k3 = _hip(mk, NCOL, NZ, shards=shards, **sw)
    _schedule(h, ALL7, want.recs)
    h.step(1, NSTEPS)
    h.synchronize()
    is_the_oracles(h, k3, want.ob, NZ, want.active, f"all kinds, mode {solver_mode}, shards {shards}")
    h.close()


def test_sst0_and_fcorr_twod_beside_each_other_kinds(mk):
    """The two-dimensional kinds are read under their own switches (ocnint_mod.F90:97-125): each with the
    three-dimensional relaxations and the bottom temperature scheduled beside it."""
    for twod, sw2 in (("SST0", dict(L_RELAX_SST=1)), ("fcorr_twod", dict(L_FCORR=1))):
        sched = {twod: (2, ac.stepwise(2, NSTEPS)), "ocnT_clim": (1, ac.mixed(NSTEPS)), "sal_clim": (4, ac.stepwise(4, NSTEPS)),
                 "bottom_temp": (3, ac.stepwise(3, NSTEPS))}
        sw = dict(L_RELAX_OCNT=1, L_RELAX_SAL=1, **sw2)
        want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), **sw)
        only = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key({k: v for k, v in sched.items() if k != twod}), **sw)
        assert ac.differs_on(want.ob, only.ob, NZ, want.active).all()   # reach: the 2-D kind's later records are read
        h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
        _schedule(h, sched, want.recs)
        h.step(1, NSTEPS)
        is_the_oracles(h, k3, want.ob, NZ, want.active, twod)
        h.close()


# ---------------------------------------------------------------------------
# 4. columns at different epochs at the same time
# ---------------------------------------------------------------------------
FORMS = {
    "fewer_columns_than_slots": dict(),
    "forced_views": {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"},
    "xcc_drop_0x55": {"MCKPP_XCC_DROP": "0x55"},
    "xcc_drop_0xfe": {"MCKPP_XCC_DROP": "0xfe"},
}
AT_ONCE = {"ocnT_clim": (1, ac.interpolated(20)), "SST0": (1, ac.stepwise(1, 20)), "bottom_temp": (1, ac.stepwise(1, 20))}
AT_ONCE_SW = dict(L_RELAX_OCNT=1, L_RELAX_SST=1, land_every=0)


@pytest.mark.parametrize("form", list(FORMS))
def test_columns_at_different_epochs_at_once(mk, monkeypatch, form):
    """8 columns, 20 steps, cadence 1: fewer columns than slots, so later tickets are drawn before their columns are
    ready and columns run tens of steps apart; the same with every column a straggler (views), and with XCDs that start
    without a queue.  Each compared with a launch per step too."""
    ncol, nsteps = 8, 20
    want = ac.oracle_run(ncol, NZ, nsteps, ac.key(AT_ONCE), **AT_ONCE_SW)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    h, kc, k3 = _hip(mk, ncol, NZ, **AT_ONCE_SW)
    _schedule(h, AT_ONCE, want.recs)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, want.ob, NZ, want.active, form)
    one = _fields(h, k3, NZ)
    h.close()
    monkeypatch.setenv("MCKPP_MULTISTEP", "0")
    h, kc, k3 = _hip(mk, ncol, NZ, **AT_ONCE_SW)
    _schedule(h, AT_ONCE, want.recs)
    h.step(1, nsteps)
    assert h.last_launch_count() == nsteps
    _same(one, _fields(h, k3, NZ), want.active, form + ": a launch per step")
    h.close()


def test_flagged_steps_inside_the_launch_at_itermax_4(mk, monkeypatch):
    """itermax = 4: column-steps end flagged inside the launch; the step log's records are the oracle's."""
    ncol, nsteps = 8, 20
    sw = dict(AT_ONCE_SW, itermax=4)
    want = ac.oracle_run(ncol, NZ, nsteps, ac.key(AT_ONCE), **sw)
    log = [(nt + 1, int(c), int(want.status[nt][c]), int(want.npasses[nt][c])) for nt in range(nsteps) for c in want.active
           if want.status[nt][c] != 0]
    assert any(e[0] < nsteps for e in log)   # reach: flagged steps before the last
    h, kc, k3 = _hip(mk, ncol, NZ, **sw)
    _schedule(h, AT_ONCE, want.recs)
    h.step_log(nsteps * ncol)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    nt_, pt, st, npass = h.step_log_fetch()
    assert list(zip(nt_.tolist(), pt.tolist(), st.tolist(), npass.tolist())) == log
    is_the_oracles(h, k3, want.ob, NZ, want.active, "itermax 4")
    one = _fields(h, k3, NZ)
    h.close()
    monkeypatch.setenv("MCKPP_MULTISTEP", "0")
    h, kc, k3 = _hip(mk, ncol, NZ, **sw)
    _schedule(h, AT_ONCE, want.recs)
    h.step(1, nsteps)
    _same(one, _fields(h, k3, NZ), want.active, "itermax 4: a launch per step")
    h.close()


# ---------------------------------------------------------------------------
# 5. the resets read the step's own record
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k_column_ps", "k_column_ps<EXT>"])
def test_a_retried_step_resets_to_the_steps_own_climatology(mk, kernel):
    """ref_step_cases' temperature step on every third column: the step is retried and check_profile resets T and S to
    the climatology (overrides.F90:57-78) - of that step's epoch.  The first records carry the temperature step
    themselves, so steps of later epochs are reset too.  With clim_present alone it is the default-physics kernel, and
    reset_flag stays zero (overrides.F90:121-123): the reach condition is the retried steps and that nothing but the
    reset reads the climatology.  With L_NO_ISOTHERM beside it (and a threshold no column meets) reset_flag shows 999."""
    ncol, nsteps = 60, 6
    sched = {"ocnT_clim": (1, ac.stepwise(1, nsteps)), "sal_clim": (2, ac.stepwise(2, nsteps))}
    sw = dict(pre="tjump", clim_present=1)
    if kernel != "k_column_ps":
        sw.update(L_NO_ISOTHERM=1, iso_bot=20, iso_thresh=1e-12)
    want = ac.oracle_run(ncol, NZ, nsteps, ac.key(sched), **sw)
    held = ac.oracle_run(ncol, NZ, nsteps, ac.key(sched), hold_record0=True, **sw)
    assert all(np.any(want.status[nt][want.active] & 4) for nt in (1, 2, 3))   # reach: retried steps in epochs 1, 2, 3
    assert ac.differs_on(want.ob, held.ob, NZ, want.active).any()            # ... whose reset read a later record
    if kernel != "k_column_ps":
        assert all(np.any(want.reset_flags[nt][want.active] == 999.) for nt in (1, 2, 3))
        assert not any(np.any(r < 0) for r in want.reset_flags)
    h, kc, k3 = _hip(mk, ncol, NZ, **sw)
    assert h.kernel_name == kernel
    _schedule(h, sched, want.recs)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, want.ob, NZ, want.active, "tjump + scheduled climatology")
    h.close()


def test_an_isotherm_reset_reads_the_steps_own_climatology(mk):
    """L_NO_ISOTHERM (overrides.F90:102-120): an isothermal column is reset to the climatology of its step's epoch; the
    first records are isothermal there themselves, so the reset fires in later epochs too."""
    ncol, nsteps = 60, 6
    sched = {"ocnT_clim": (1, ac.stepwise(1, nsteps)), "sal_clim": (1, ac.stepwise(1, nsteps))}
    sw = dict(pre="isothermal", L_NO_ISOTHERM=1, clim_present=1, iso_bot=20, iso_thresh=0.002)
    want = ac.oracle_run(ncol, NZ, nsteps, ac.key(sched), **sw)
    assert all(np.any(want.reset_flags[nt][want.active] < 0) for nt in (1, 2, 3))   # reach: isotherm resets in epochs 1, 2, 3
    h, kc, k3 = _hip(mk, ncol, NZ, **sw)
    assert h.kernel_name == "k_column_ps<EXT>"
    _schedule(h, sched, want.recs)
    h.step(1, nsteps)
    assert h.last_launch_count() == 1
    is_the_oracles(h, k3, want.ob, NZ, want.active, "isotherm reset + scheduled climatology")
    h.close()


# ---------------------------------------------------------------------------
# 6. beside the other in-launch features
# ---------------------------------------------------------------------------
def test_beside_flux_series_windows_snapshots_and_log(mk, tmp_path):
    """run_forced of 12 steps from a flux series under schedules of ocnT_clim (interpolated every step), SST0 (every 3)
    and the bottom temperature (every 4), with a window schedule of period 2 on T, tinc_fcorr, fcorr_z and fcorr, a restart
    schedule of period 4 and a step log: records, snapshot files (byte for byte) and log equal those of the run with
    its launches cut at the epoch boundaries; the end state and the log are the oracle's."""
    ncol, nz, nsteps, ndtocn, min_passes = 77, NZ, NSTEPS, 2, 6
    sched = {"ocnT_clim": (1, ac.interpolated(nsteps)), "SST0": (3, ac.stepwise(3, nsteps)),
             "bottom_temp": (4, ac.stepwise(4, nsteps))}
    sw = dict(L_RELAX_OCNT=1, L_RELAX_SST=1)
    want = ac.oracle_run(ncol, nz, nsteps, ac.key(sched), series_key=23, ndtocn=ndtocn, **sw)
    log = [(nt + 1, int(c), int(want.status[nt][c]), int(want.npasses[nt][c])) for nt in range(nsteps) for c in want.active
           if want.status[nt][c] != 0 or want.npasses[nt][c] >= min_passes]
    assert any(e[0] < nsteps for e in log)
    names = ("T", "tinc_fcorr", "fcorr_z", "fcorr")
    ops = (A.OP_MEAN, A.OP_MAX, A.OP_LAST)

    def run(cut):
        h, kc, k3 = _hip(mk, ncol, nz, series=want.series, **sw)
        h.window_schedule(0, 1, 2, nsteps // 2, names, A.WIN_MEAN | A.WIN_MAX | A.WIN_LAST)
        h.restart_schedule(1, 4, nsteps // 4)
        h.step_log(nsteps * ncol, min_passes)
        if cut:
            _cut_launches(h, k3, sched, want.recs, nsteps, run=lambda nt, n: h.run_forced(nt, n, ndtocn))
        else:
            _schedule(h, sched, want.recs)
            h.run_forced(1, nsteps, ndtocn)
            assert h.last_launch_count() == 1
        rec = {}
        for w in range(nsteps // 2):
            for n in names:
                shape = (ncol,) if n == "fcorr" else (ncol, kc.nzp1)
                for op in ops:
                    rec[w, n, op] = h.window_record_fetch(0, w, n, op, np.full(shape, -7.0, order="F")).copy()
        files = []
        for s in range(nsteps // 4):
            files.append(tmp_path / f"snap{int(cut)}_{s}")
            h.restart_snapshot_save(s, files[-1])
        lg = h.step_log_fetch()
        if not cut:
            is_the_oracles(h, k3, want.ob, nz, want.active, "beside the schedules")
        h.close()
        return rec, [open(f, "rb").read() for f in files], list(zip(*[a.tolist() for a in lg]))

    rec1, files1, log1 = run(cut=False)
    rec2, files2, log2 = run(cut=True)
    assert log1 == log and log2 == log
    for k in rec2:
        assert np.array_equal(rec1[k], rec2[k], equal_nan=True), k
    assert files1 == files2


# ---------------------------------------------------------------------------
# 7. the same split differently
# ---------------------------------------------------------------------------
SPLIT = {"ocnT_clim": (2, ((0, 1, 0.75, 0.25), (0, 1, 0.25, 0.75), (1, 2, 0.6, 0.4), 2, (2, 3, 1.0 / 3.0, 1.0 - 1.0 / 3.0), 3)),
         "SST0": (3, ac.stepwise(3, NSTEPS)), "bottom_temp": (3, ac.stepwise(3, NSTEPS))}
SPLIT_SW = dict(L_RELAX_OCNT=1, L_RELAX_SST=1)


def test_five_plus_seven_steps_with_the_schedule_kept(mk):
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(SPLIT), **SPLIT_SW)
    h, kc, k3 = _hip(mk, NCOL, NZ, **SPLIT_SW)
    _schedule(h, SPLIT, want.recs)
    h.step(1, 5)
    h.step(6, 7)
    is_the_oracles(h, k3, want.ob, NZ, want.active, "5 + 7")
    h.close()


def test_series_replaced_between_launches_holding_the_later_records(mk):
    """Steps 1-6 with records 0.. resident, then each series replaced by one that starts at the first record steps 7-12
    need (rec0 > 0) and holds only the later ones."""
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(SPLIT), **SPLIT_SW)
    h, kc, k3 = _hip(mk, NCOL, NZ, **SPLIT_SW)
    _schedule(h, SPLIT, want.recs)
    h.step(1, 6)
    for n, (cad, ep) in SPLIT.items():
        later = [e for e in ep[6 // cad:]]
        rec0 = min(min(e[0], e[1]) if np.ndim(e) else e for e in later)
        assert rec0 > 0
        h.set_ancillary_series(ac.KINDS[n][0], rec0, _as_series(n, want.recs[n][rec0:]))
    with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_step: SST0: step 6 \(epoch 1\) needs record 1, resident are 2\.\.3"):
        h.step(6, 2)
    h.step(7, 6)
    is_the_oracles(h, k3, want.ob, NZ, want.active, "later records only")
    h.close()


# ---------------------------------------------------------------------------
# 8. refusals; cancelling; upload
# ---------------------------------------------------------------------------
def test_refusals_leave_the_state_unchanged(mk):
    sched = {"ocnT_clim": (3, ac.stepwise(3, NSTEPS)), "bottom_temp": (3, ac.stepwise(3, NSTEPS))}
    sw = dict(L_RELAX_OCNT=1)
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), **sw)
    K = {n: v[0] for n, v in ac.KINDS.items()}
    bt, clim = _as_series("bottom_temp", want.recs["bottom_temp"]), _as_series("ocnT_clim", want.recs["ocnT_clim"])
    h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
    before = _fields(h, k3, NZ)
    E = mk.MckppHipError
    # negative arguments, unknown kinds
    for call in (lambda: h.set_ancillary_series(K["ocnT_clim"], -1, clim), lambda: h.ancillary_schedule(7, 1, 3, (0, 1)),
                 lambda: h.ancillary_schedule(-1, 1, 3, (0, 1)), lambda: h.ancillary_schedule(K["ocnT_clim"], -1, 3, (0, 1)),
                 lambda: h.ancillary_schedule(K["ocnT_clim"], 1, 0, (0, 1)), lambda: h.ancillary_schedule(K["ocnT_clim"], 1, -3, (0, 1)),
                 lambda: h.ancillary_schedule(K["ocnT_clim"], 1, 3, (0, 1), epoch0=-1),
                 lambda: h.ancillary_schedule(K["ocnT_clim"], 1, 3, (0, -2)),
                 lambda: h.ancillary_schedule(K["ocnT_clim"], 1, 3, ((-1, 1, 0.5, 0.5),))):
        with pytest.raises(E, match=r"mckpp_hip_(set_ancillary_series|ancillary_schedule): "):
            call()
    lib = mk.load_library()
    assert lib.mckpp_hip_set_ancillary_series(h._h, K["ocnT_clim"], 0, -1, clim.ctypes.data_as(A._dp)) != 0
    assert lib.mckpp_hip_ancillary_schedule(h._h, K["ocnT_clim"], 1, 3, 0, -1, None) != 0
    for kind in (-1, 7):
        assert lib.mckpp_hip_set_ancillary_series(h._h, kind, 0, 2, clim.ctypes.data_as(A._dp)) != 0
    # interpolation on a 2-D kind (and on the other kinds the reference does not interpolate)
    for n in ("SST0", "fcorr_twod", "bottom_temp", "fcorr_withz", "sfcorr_withz"):
        with pytest.raises(E, match=r"is interpolated.*ocnT_clim and sal_clim only"):
            h.ancillary_schedule(K[n], 1, 3, ((0, 1, 0.5, 0.5),))
    # a record that is not resident; an epoch outside the table; a step before the origin
    h.ancillary_schedule(K["ocnT_clim"], 1, 3, sched["ocnT_clim"][1])
    with pytest.raises(E, match=r"mckpp_hip_step: ocnT_clim: step 1 \(epoch 0\) needs record 0, none is resident"):
        h.step(1, NSTEPS)
    h.set_ancillary_series(K["ocnT_clim"], 0, clim[:3])
    with pytest.raises(E, match=r"mckpp_hip_step: ocnT_clim: step 10 \(epoch 3\) needs record 3, resident are 0\.\.2"):
        h.step(1, NSTEPS)
    h.set_ancillary_series(K["ocnT_clim"], 0, clim)
    with pytest.raises(E, match=r"mckpp_hip_step: ocnT_clim: step 13 is in epoch 4, the table holds epochs 0\.\.3"):
        h.step(1, NSTEPS + 1)
    with pytest.raises(E, match=r"mckpp_hip_run_forced: ocnT_clim: step 13 is in epoch 4"):
        h.set_flux_series(0, ac.flux_series(NCOL, 13, 1))
        h.run_forced(13, 1, 1)
    h.ancillary_schedule(K["ocnT_clim"], 2, 3, sched["ocnT_clim"][1])
    with pytest.raises(E, match=r"mckpp_hip_step: ocnT_clim: step 1 lies before the schedule's origin 2"):
        h.step(1, 1)
    h.ancillary_schedule(K["ocnT_clim"], 1, 3, sched["ocnT_clim"][1])
    # the bottom temperature: exclusive with set_bottomtemp in either order, host override refused, diagnostics needed
    h.set_bottomtemp(want.recs["bottom_temp"][0])
    with pytest.raises(E, match=r"mckpp_hip_ancillary_schedule: a bottom temperature is resident.*mutually exclusive"):
        h.ancillary_schedule(K["bottom_temp"], 1, 3, sched["bottom_temp"][1])
    h.set_bottomtemp(None)
    h.set_ancillary_series(K["bottom_temp"], 0, bt)
    h.ancillary_schedule(K["bottom_temp"], 1, 3, sched["bottom_temp"][1])
    with pytest.raises(E, match=r"mckpp_hip_set_bottomtemp: the bottom temperature has a schedule.*mutually exclusive"):
        h.set_bottomtemp(want.recs["bottom_temp"][0])
    with pytest.raises(E, match=r"mckpp_hip_bottomtemp: the bottom temperature has a schedule"):
        h.bottomtemp(want.recs["bottom_temp"][0])
    h.set_diagnostics(0)
    for call in (lambda: h.step(1, 1), lambda: h.step(1, NSTEPS)):
        with pytest.raises(E, match=r"mckpp_hip_step: the bottom temperature has a schedule.*diagnostics are switched\s+off"):
            call()
    h.set_diagnostics(1)
    _same(before, _fields(h, k3, NZ), want.active, "nothing was launched")
    # ... and the good launch
    h.step(1, NSTEPS)
    is_the_oracles(h, k3, want.ob, NZ, want.active, "after the refusals")
    h.close()


def test_other_kinds_are_refused_on_a_default_physics_context(mk):
    sched = {"bottom_temp": (3, ac.stepwise(3, NSTEPS))}
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched))
    h, kc, k3 = _hip(mk, NCOL, NZ)
    assert h.kernel_name == "k_column_ps"
    for n, (kind, _, is3d) in ac.KINDS.items():
        if n == "bottom_temp":
            continue
        recs = np.zeros((2, NZ + 1, NCOL) if is3d else (2, NCOL))
        with pytest.raises(mk.MckppHipError, match=rf"mckpp_hip_set_ancillary_series: {n} on a context of the default physics.*L_RELAX_SST"):
            h.set_ancillary_series(kind, 0, recs)
        with pytest.raises(mk.MckppHipError, match=rf"mckpp_hip_ancillary_schedule: {n} on a context of the default physics"):
            h.ancillary_schedule(kind, 1, 3, (0, 1))
    _schedule(h, sched, want.recs)
    h.step(1, NSTEPS)
    is_the_oracles(h, k3, want.ob, NZ, want.active, "bottom temperature on the default physics")
    h.close()


def test_cancel_and_upload_return_to_the_plain_resident_field(mk):
    """nepochs = 0, and upload, cancel: the launches read what upload / update_ancillaries / nothing left resident - the
    oracle holding record 0 (the field the case starts with) throughout, without a bottom-temperature override."""
    sched = {"ocnT_clim": (3, ac.stepwise(3, NSTEPS)), "SST0": (3, ac.stepwise(3, NSTEPS))}
    sw = dict(L_RELAX_OCNT=1, L_RELAX_SST=1)
    want = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), **sw)
    held = ac.oracle_run(NCOL, NZ, NSTEPS, ac.key(sched), hold_record0=True, **sw)
    assert ac.differs_on(want.ob, held.ob, NZ, want.active).all()
    h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
    both = dict(sched, bottom_temp=(3, ac.stepwise(3, NSTEPS)))
    recs = dict(want.recs, bottom_temp=np.stack([ac.record("bottom_temp", r, *ac.both(NCOL, NZ, **sw)[4]) for r in range(4)]))
    _schedule(h, both, recs)
    for n in both:
        h.ancillary_schedule(ac.KINDS[n][0], 1, 3, None)
    h.step(1, NSTEPS)
    is_the_oracles(h, k3, held.ob, NZ, held.active, "cancelled by nepochs = 0")
    h.close()
    h, kc, k3 = _hip(mk, NCOL, NZ, **sw)
    _schedule(h, both, recs)
    _, _, _, k3, _ = ac.both(NCOL, NZ, **sw)
    h.upload(k3)
    h.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(NCOL, "bench"))
    h.set_forcing(k3.sflux)
    h.step(1, NSTEPS)
    is_the_oracles(h, k3, held.ob, NZ, held.active, "cancelled by upload")
    with pytest.raises(mk.MckppHipError, match=r"needs record 0, none is resident"):   # the records went with the schedules
        h.ancillary_schedule(ac.KINDS["SST0"][0], 1, 3, sched["SST0"][1])
        h.step(1, 1)
    h.close()
