"""The flux-record ring (mckpp_hip_flux_ring, _put, _records): forcing streamed into a ring of record slots on the device
while earlier launches run, read by the column kernel slot by slot.

The yardstick is tests/golden/ref_loop.npz, the compiled reference's own time loop (tests/ref_loop_cases.py); its
neighbouring records differ on every ocean column, so a record read from the wrong slot changes the digests.  Where a
form has no golden record (another solver mode, optional physics, a case made here) the run through the ring is held,
bit for bit, to set_flux_series plus one run_forced of the same records: every compared field, status words and pass
counts.

The loop of a run through the ring: put two records, run_forced over their steps, until the case ends.  With 3 slots
the second call holds records 2,3 in slots 2,0: a launch whose records wrap.  Which cases have such a launch follows
from their number of records n: a call starts at an even record r0, and wraps if r0 % 3 == 2 with a second record to
go - r0 = 2, n >= 4.  diurnal_nz60_nd3 and sweep_nd3 (8 records) do; deep_nz100_nd4 has 3 records, its second call
holds record 2 alone, and does not."""
import numpy as np
import pytest

import anc_cases as ac
import ref_loop_cases as lc
import ref_step_cases as rc
from harness import assert_loop_step, assert_same, cleared, flux_args, initialised, loop_state, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401

pytestmark = pytest.mark.gpu

ENV = ("MCKPP_MULTISTEP", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT", "MCKPP_XCC_DROP", "MCKPP_PS_FIXED_L", "MCKPP_SOLVER_MODE")
PER_CALL = 2
_clean_env = cleared(ENV)


def _assert_golden(golden, tag, nt, h, k3, kc, what):
    h.download(k3)
    assert_loop_step(golden, tag, nt, k3, kc, what)


def _through_the_ring(h, rec, nsteps, nd, nslots, run=None, after_call=None, **args):
    """Put PER_CALL records, run_forced over their steps, until step nsteps.  Returns how many of the calls held records
    whose slots wrap, from flux_ring_records() and the ring size."""
    run = run or (lambda nt0, n: h.run_forced(nt0, n, nd, **args))
    wraps = 0
    for r0 in range(0, len(rec), PER_CALL):
        count = min(PER_CALL, len(rec) - r0)
        for r in range(r0, r0 + count):
            h.flux_ring_put(r, rec[r])
        first, last = h.flux_ring_records()
        assert (first, last) == (max(0, r0 + count - nslots), r0 + count - 1)
        first_of_call = last - count + 1
        wraps += first_of_call % nslots + count > nslots
        nt0, nt1 = r0 * nd + 1, min((r0 + count) * nd, nsteps)
        run(nt0, nt1 - nt0 + 1)
        if after_call:
            after_call(nt1)
    return wraps


def _expect_wraps(n, nslots):
    return sum(r0 % nslots + min(PER_CALL, n - r0) > nslots for r0 in range(0, n, PER_CALL))


# ---------------------------------------------------------------------------
# 1. every golden case through rings of 2 and of 3 slots
# ---------------------------------------------------------------------------
# cases that reach a path of their own, named so that an edit of the case list cannot drop them silently: L_REST, the
# eight constants without a flux file, land columns
REACH = ("l_rest", "no_flux_file", "every_step_nz40", "namelist_nz69_nd2")


def test_the_cases_that_reach_a_path_are_in_the_list():
    for tag in REACH:
        assert tag in lc.CASES, tag
    assert lc.CASES["l_rest"].l_rest == 1 and not lc.CASES["no_flux_file"].flux_file
    assert lc.CASES["every_step_nz40"].land_every and lc.CASES["namelist_nz69_nd2"].land_every
    assert _expect_wraps(lc.nrec(lc.CASES["diurnal_nz60_nd3"]), 3) and _expect_wraps(lc.nrec(lc.CASES["sweep_nd3"]), 3)


@pytest.mark.parametrize("nslots", [2, 3])
@pytest.mark.parametrize("tag", list(lc.CASES))
def test_golden_cases_through_the_ring(mk, golden, tag, nslots):
    """The digest after the last step of every call, not only of the run; with 3 slots, launches whose records wrap."""
    case = lc.CASES[tag]
    h, kc, k3 = resident(mk, case)
    h.flux_ring(nslots)
    assert h.flux_ring_records() == (-1, -1)
    wraps = _through_the_ring(h, lc.flux_records(case), case.nsteps, case.ndtocn, nslots,
                              after_call=lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, f"ring of {nslots}"),
                              **flux_args(case))
    assert wraps == _expect_wraps(lc.nrec(case), nslots)
    if nslots == 2:
        assert wraps == 0
    if nslots == 3 and tag in ("diurnal_nz60_nd3", "sweep_nd3"):
        assert wraps >= 1, "no launch of the case holds records whose slots wrap"
    h.close()


# ---------------------------------------------------------------------------
# 2. ordering without host waits
# ---------------------------------------------------------------------------
def test_puts_and_launches_are_ordered_on_the_device(mk, golden):
    """sweep_nd3, ring of 2, no synchronize between the first put and the final download: every put follows the
    asynchronous run_forced before it at once - it overwrites a slot whose record the queued launch reads - and every
    launch follows the put of its own records at once.  The array handed to put is filled with NaN right after."""
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    rec = lc.flux_records(case)
    h, kc, k3 = resident(mk, case)
    h.flux_ring(2)
    buf = np.empty((8, case.ncol))
    for r0 in range(0, len(rec), 2):
        for r in (r0, r0 + 1):
            buf[...] = rec[r]
            h.flux_ring_put(r, buf)
            buf.fill(np.nan)
        h.run_forced(r0 * case.ndtocn + 1, 2 * case.ndtocn, case.ndtocn, **flux_args(case))
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "puts and launches back to back")
    h.close()


# ---------------------------------------------------------------------------
# 3. launch forms
# ---------------------------------------------------------------------------
def _series_run(mk, make, rec, nsteps, nd, nz, mode=None, **args):
    """set_flux_series of all records plus one run_forced"""
    h, kc, k3 = make()
    if mode is not None:
        h.set_solver_mode(mode)
    h.set_flux_series(0, rec)
    h.run_forced(1, nsteps, nd, **args)
    out = loop_state(h, k3, kc, nz)
    h.close()
    return out


GOLDEN_FORMS = {
    "launch_per_step": {"MCKPP_MULTISTEP": "0"},
    "general_kernel_at_60": {"MCKPP_PS_FIXED_L": "0"},
    "forced_views": {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"},
    "xcc_drop_0x55": {"MCKPP_XCC_DROP": "0x55"},
    "xcc_drop_0xfe": {"MCKPP_XCC_DROP": "0xfe"},
}


@pytest.mark.parametrize("form", list(GOLDEN_FORMS))
def test_launch_forms_against_the_golden_record(mk, golden, monkeypatch, form):
    """diurnal_nz60_nd3 (60 levels: the literal-level kernels by default), ring of 3: its second call wraps."""
    tag = "diurnal_nz60_nd3"
    case = lc.CASES[tag]
    for k, v in GOLDEN_FORMS[form].items():
        monkeypatch.setenv(k, v)
    h, kc, k3 = resident(mk, case)
    h.flux_ring(3)
    counts = []

    def run(nt0, n):
        h.run_forced(nt0, n, case.ndtocn, **flux_args(case))
        counts.append((n, h.last_launch_count()))

    wraps = _through_the_ring(h, lc.flux_records(case), case.nsteps, case.ndtocn, 3, run=run,
                              after_call=lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, form))
    assert wraps >= 1
    assert all(k == (n if form == "launch_per_step" else 1) for n, k in counts), counts
    h.close()


def test_one_step_per_call(mk):
    """run_forced(nt, 1, ...) in a loop - k_fluxes is handed the slot's pointer - against the series run."""
    case = lc.CASES["diurnal_nz60_nd3"]
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    want = _series_run(mk, lambda: resident(mk, case), rec, case.nsteps, case.ndtocn, case.nz, **args)
    h, kc, k3 = resident(mk, case)
    h.flux_ring(3)

    def run(nt0, n):
        for nt in range(nt0, nt0 + n):
            h.run_forced(nt, 1, case.ndtocn, **args)

    assert _through_the_ring(h, rec, case.nsteps, case.ndtocn, 3, run=run) >= 1
    assert_same(loop_state(h, k3, kc, case.nz), want, active, "a step per call")
    h.close()


def test_fewer_columns_than_slots(mk):
    """8 columns over 20 steps, records made as flux_records makes them."""
    case = lc.LoopCase(8, 40, 20, 3, seed=211, sun=True, land_every=5, calm_every=3)
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    assert len(rec) == 7
    want = _series_run(mk, lambda: resident(mk, case), rec, case.nsteps, case.ndtocn, case.nz, **args)
    h, kc, k3 = resident(mk, case)
    h.flux_ring(3)
    assert _through_the_ring(h, rec, case.nsteps, case.ndtocn, 3, **args) >= 1
    assert_same(loop_state(h, k3, kc, case.nz), want, active, "8 columns")
    h.close()


def test_double_diffusion_kernel(mk):
    case = lc.CASES["ldd_nz60"]
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    want = _series_run(mk, lambda: resident(mk, case), rec, case.nsteps, case.ndtocn, case.nz, **args)
    h, kc, k3 = resident(mk, case)
    assert h.kernel_name == "k_column_ps<EXT>"
    h.flux_ring(3)
    assert _through_the_ring(h, rec, case.nsteps, case.ndtocn, 3, **args) >= 1
    assert_same(loop_state(h, k3, kc, case.nz), want, active, "LDD")
    h.close()


def _relax_sst(mk, ncol=77, nz=40, **kw):
    oc, ob, kc, k3, TS = ac.both(ncol, nz, L_RELAX_SST=1, **kw)
    return initialised(mk, kc, k3), kc, k3


def test_optional_physics_kernel(mk):
    """L_RELAX_SST: the kernel build that carries the optional physics."""
    ncol, nz, nsteps, nd = 77, 40, 12, 2
    rec = ac.flux_series(ncol, nsteps // nd, 31)
    want = _series_run(mk, lambda: _relax_sst(mk), rec, nsteps, nd, nz)
    h, kc, k3 = _relax_sst(mk)
    assert h.kernel_name == "k_column_ps<EXT>"
    active = np.nonzero(k3.run_physics)[0]
    h.flux_ring(3)
    assert _through_the_ring(h, rec, nsteps, nd, 3) >= 1
    assert_same(loop_state(h, k3, kc, nz), want, active, "L_RELAX_SST")
    h.close()


def test_two_ended_solver(mk, monkeypatch):
    """MCKPP_SOLVER_MODE=1 has no golden record: the ring against that mode's own series run, bit for bit (no looser
    than any tolerance: the two runs do the same arithmetic on the same records)."""
    monkeypatch.setenv("MCKPP_SOLVER_MODE", "1")
    case = lc.CASES["diurnal_nz60_nd3"]
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    want = _series_run(mk, lambda: resident(mk, case), rec, case.nsteps, case.ndtocn, case.nz, **args)
    h, kc, k3 = resident(mk, case)
    assert h.solver_mode == 1
    h.flux_ring(3)
    assert _through_the_ring(h, rec, case.nsteps, case.ndtocn, 3, **args) >= 1
    assert_same(loop_state(h, k3, kc, case.nz), want, active, "solver mode 1")
    h.close()


# ---------------------------------------------------------------------------
# 4. beside the other in-launch features
# ---------------------------------------------------------------------------
def test_beside_windows_export_snapshots_log_and_ancillary_schedule(mk, tmp_path):
    """One chunked run through a ring of 3 under a window schedule on T and hmix (mean, max) with its export, a restart
    schedule, a step log (itermax = 4; flagged column-steps and those of at least 3 passes) and an ancillary schedule on SST0: records, exported planes, snapshot files and
    log equal those of the all-resident one-launch run, byte for byte."""
    A = mk.api
    ncol, nz, nsteps, nd = 77, 40, 12, 2
    rec = ac.flux_series(ncol, nsteps // nd, 37)
    sched = {"SST0": (3, ac.stepwise(3, nsteps))}
    names, ops = ("T", "hmix"), (A.OP_MEAN, A.OP_MAX)

    def run(ring):
        oc, ob, kc, k3, (T, S) = ac.both(ncol, nz, L_RELAX_SST=1, itermax=4)
        h = mk.MckppHip(kc)
        h.upload(k3)
        h.init_ocean(0)
        recs = ac.records_of(sched, T, S)
        h.set_ancillary_series(A.ANC_SST0, 0, np.ascontiguousarray(recs["SST0"]))
        h.ancillary_schedule(A.ANC_SST0, 1, sched["SST0"][0], sched["SST0"][1])
        h.window_schedule(0, 1, 2, nsteps // 2, names, A.WIN_MEAN | A.WIN_MAX)
        h.window_export(0, "f8", -3.0)
        h.restart_schedule(1, 4, nsteps // 4)
        h.step_log(nsteps * ncol, 3)
        if ring:
            h.flux_ring(3)
            assert _through_the_ring(h, rec, nsteps, nd, 3) >= 1
        else:
            h.set_flux_series(0, rec)
            h.run_forced(1, nsteps, nd)
            assert h.last_launch_count() == 1
        out, exp = {}, {}
        for w in range(nsteps // 2):
            for n in names:
                shape = (ncol,) if n == "hmix" else (ncol, kc.nzp1)
                for op in ops:
                    out[w, n, op] = h.window_record_fetch(0, w, n, op, np.full(shape, -7.0, order="F")).copy()
                    exp[w, n, op] = h.window_export_fetch(0, w, n, op, np.zeros(shape, order="F")).copy()
        files = []
        for s in range(nsteps // 4):
            files.append(tmp_path / f"snap{int(ring)}_{s}")
            h.restart_snapshot_save(s, files[-1])
        lg = h.step_log_fetch()
        end = loop_state(h, k3, kc, nz, rc.STEP_FIELDS)
        h.close()
        return out, exp, [open(f, "rb").read() for f in files], list(zip(*[a.tolist() for a in lg])), end

    want, got = run(ring=False), run(ring=True)
    assert len(want[3]) > 0 and any(e[0] < nsteps for e in want[3]), "itermax = 4 flags no column-step inside the run"
    for k in want[0]:
        assert np.array_equal(got[0][k].view(np.uint64), want[0][k].view(np.uint64)), ("record", k)
        assert np.array_equal(got[1][k].view(np.uint64), want[1][k].view(np.uint64)), ("exported plane", k)
    assert got[2] == want[2], "snapshot files"
    assert got[3] == want[3], "step log"
    assert_same(got[4], want[4], slice(None), "end state")


# ---------------------------------------------------------------------------
# 5. refusals, each followed by good calls that end in the golden state
# ---------------------------------------------------------------------------
def _raw_state(h, k3, kc, nz):
    d = loop_state(h, k3, kc, nz)
    return {n: v.copy() for n, v in d.items()}


def test_refusals_leave_everything_as_it_was(mk, golden):
    tag = "namelist_nz69_nd2"
    case = lc.CASES[tag]
    nd, args, E = case.ndtocn, flux_args(case), mk.MckppHipError
    rec = lc.flux_records(case)
    assert len(rec) == 4 and case.nsteps == 8
    kc, k3 = lc.hip_raw(case)
    h = mk.MckppHip(kc)
    with pytest.raises(E, match="mckpp_hip_flux_ring_put: upload the state"):       # a put before upload
        h.flux_ring_put(0, rec[0])
    with pytest.raises(E, match="mckpp_hip_flux_ring: upload the state first"):
        h.flux_ring(2)
    h.upload(k3)
    h.init_ocean(0)
    with pytest.raises(E, match="mckpp_hip_flux_ring_put: no flux ring is set"):    # a put without a ring
        h.flux_ring_put(0, rec[0])
    with pytest.raises(E, match="mckpp_hip_flux_ring_records: no flux ring is set"):
        h.flux_ring_records()
    with pytest.raises(E, match=r"mckpp_hip_flux_ring: nslots=-1"):
        h.flux_ring(-1)
    h.flux_ring(2)
    with pytest.raises(E, match=r"record -1, but the records arrive in order: the first one is any record >= 0"):
        h.flux_ring_put(-1, rec[0])
    h.flux_ring_put(0, rec[0])
    with pytest.raises(E, match=r"record 0, but the records arrive in order: the next one is record 1"):   # repeated
        h.flux_ring_put(0, rec[0])
    with pytest.raises(E, match=r"record 2, but the records arrive in order: the next one is record 1"):   # skipped
        h.flux_ring_put(2, rec[2])
    assert h.flux_ring_records() == (0, 0)
    h.flux_ring_put(1, rec[1])
    with pytest.raises(E, match="mckpp_hip_set_flux_series: a flux ring of 2 slots is set .* cancel the ring first"):
        h.set_flux_series(0, rec)
    # a record not yet put: nothing is launched
    before = _raw_state(h, k3, kc, case.nz)
    with pytest.raises(E, match=r"mckpp_hip_run_forced: steps 1\.\.6 need flux records 0\.\.2, the ring of 2 slots holds 0\.\.1"):
        h.run_forced(1, 3 * nd, nd, **args)
    assert_same(_raw_state(h, k3, kc, case.nz), before, slice(None), "after the refused launch (record not yet put)")
    h.run_forced(1, 2 * nd, nd, **args)
    _assert_golden(golden, tag, 2 * nd, h, k3, kc, "after the refusals")
    h.flux_ring_put(2, rec[2])
    h.flux_ring_put(3, rec[3])
    assert h.flux_ring_records() == (2, 3)
    # a record already overwritten
    before = _raw_state(h, k3, kc, case.nz)
    with pytest.raises(E, match=r"mckpp_hip_run_forced: steps 3\.\.6 need flux records 1\.\.2, the ring of 2 slots holds 2\.\.3"):
        h.run_forced(nd + 1, 2 * nd, nd, **args)
    assert_same(_raw_state(h, k3, kc, case.nz), before, slice(None), "after the refused launch (record overwritten)")
    h.run_forced(2 * nd + 1, 2 * nd, nd, **args)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "after all refusals")
    h.close()


# ---------------------------------------------------------------------------
# 6. cancel
# ---------------------------------------------------------------------------
def test_cancel_and_what_cancels(mk, golden, tmp_path):
    tag = "namelist_nz69_nd2"
    case = lc.CASES[tag]
    nd, args, E = case.ndtocn, flux_args(case), mk.MckppHipError
    rec = lc.flux_records(case)
    none = "no flux ring is set"

    # flux_ring(0), then set_flux_series works again
    h, kc, k3 = resident(mk, case)
    h.flux_ring(2)
    h.flux_ring_put(0, rec[0])
    h.flux_ring(0)
    with pytest.raises(E, match=none):
        h.flux_ring_records()
    h.set_flux_series(0, rec)
    # flux_ring(n) drops a resident series
    h.flux_ring(3)
    with pytest.raises(E, match=r"steps 1\.\.8 need flux records 0\.\.3, the ring of 3 slots holds -1\.\.-1"):
        h.run_forced(1, case.nsteps, nd, **args)
    h.flux_ring(0)
    with pytest.raises(E, match=r"need flux records 0\.\.3, resident are"):
        h.run_forced(1, case.nsteps, nd, **args)
    h.set_flux_series(0, rec)
    h.run_forced(1, case.nsteps, nd, **args)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "series after a cancelled ring")

    # upload with the same land mask keeps the ring, with another one cancels it
    kc, k3 = lc.hip_raw(case)
    h.upload(k3)
    h.flux_ring(2)
    h.flux_ring_put(0, rec[0])
    h.upload(k3)
    assert h.flux_ring_records() == (0, 0)
    kc2, other = lc.hip_raw(case)
    other.run_physics[:] = 1
    other.l_ocean[:] = 1
    other.run_physics[1::4] = 0
    other.l_ocean[1::4] = 0
    h.upload(other)
    with pytest.raises(E, match=none):
        h.flux_ring_records()

    # load_restart cancels it; the run from the loaded state through a new ring ends in the golden state
    h.upload(k3)
    h.init_ocean(0)
    path = tmp_path / "init.rst"
    h.save_restart(path)
    h.flux_ring(2)
    h.flux_ring_put(0, rec[0])
    h.load_restart(path, case.ncol)
    with pytest.raises(E, match=none):
        h.flux_ring_records()
    h.flux_ring(2)
    _through_the_ring(h, rec, case.nsteps, nd, 2, **args)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "a new ring after load_restart")
    h.close()


# ---------------------------------------------------------------------------
# 7. three shards on the one device
# ---------------------------------------------------------------------------
def test_three_shards(mk, golden):
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    h, kc, k3 = resident(mk, case, shards=3)
    h.flux_ring(3)
    assert h.flux_ring_records() == (-1, -1)
    wraps = _through_the_ring(h, lc.flux_records(case), case.nsteps, case.ndtocn, 3, **flux_args(case))
    assert wraps >= 1
    h.synchronize()
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "3 shards, ring of 3")
    h.close()
