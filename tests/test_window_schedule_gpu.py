"""Output windows accumulated inside the step launches (mckpp_hip_window_schedule): records written by the column
kernel after each column's step, so that a run with output can take many steps in one launch.  Every record must be,
bit for bit, what a second context run from the same start gives through the per-step API: window_select, window_reset
at the window's first step, window_accumulate after each of its steps, window_fetch after its last ("last": op 3, the
field as it stands then)."""
import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401
from harness import shape as _shape

pytestmark = pytest.mark.gpu

LAST_FIELDS = ("T", "S", "hmix")
RED_FIELDS = ("T", "S", "hmix", "difm", "wT", "rho", "Rig", "solar_in")


def _cut(kc, name, a):
    return a[:, :kc.nz] if name in ("Rig", "Shsq") else a   # level nzp1 of these is never written by the model


def _equal(kc, name, got, ref, ocean, tag):
    assert np.array_equal(_cut(kc, name, got)[ocean], _cut(kc, name, ref)[ocean]), (name, tag)
    assert np.all(got[~ocean] == -7.0), (name, tag, "land")


class PerStep:
    """The reference: a context that runs the same steps one launch at a time and reduces with the existing API.
    Schedule `red` (period pr, mean/min/max) through window_select/reset/accumulate/fetch; schedule `last` (period pl)
    through window_fetch op 3 at each window's last step."""

    def __init__(self, mk, ctx, kc, npts, origin, pl, pr, red=RED_FIELDS, last=LAST_FIELDS, ops=(0, 1, 2)):
        self.mk, self.ctx, self.kc, self.npts = mk, ctx, kc, npts
        self.origin, self.pl, self.pr, self.red, self.last, self.ops = origin, pl, pr, red, last, ops
        self.rec_last, self.rec_red = {}, {}
        ctx.window_select([mk.api.OUT[n] for n in red])

    def after_step(self, nt):
        A, q = self.mk.api, nt - self.origin
        if q < 0:
            return
        if q % self.pr == 0:
            self.ctx.window_reset()
        self.ctx.window_accumulate()
        if q % self.pr == self.pr - 1:
            rec = {}
            for n in self.red:
                for op in self.ops:
                    out = np.full(_shape(self.kc, self.npts, n), -7.0, order="F")
                    rec[n, op] = self.ctx.window_fetch(A.OUT[n], op, out).copy()
            self.rec_red[q // self.pr] = rec
        if q % self.pl == self.pl - 1:
            rec = {}
            for n in self.last:
                out = np.full(_shape(self.kc, self.npts, n), -7.0, order="F")
                rec[n] = self.ctx.window_fetch(A.OUT[n], A.OP_INSTANT, out).copy()
            self.rec_last[q // self.pl] = rec


def _schedule(mk, h, origin, pl, pr, nrec=8, red=RED_FIELDS, last=LAST_FIELDS):
    A = mk.api
    h.window_schedule(0, origin, pl, nrec, last, A.WIN_LAST)
    h.window_schedule(1, origin, pr, nrec, red, A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX)


def _check_records(mk, h, ref, kc, npts, ocean, tag=""):
    A = mk.api
    assert ref.rec_last and ref.rec_red
    for w, rec in ref.rec_last.items():
        for n in ref.last:
            out = np.full(_shape(kc, npts, n), -7.0, order="F")
            h.window_record_fetch(0, w, n, A.OP_LAST, out)
            _equal(kc, n, out, rec[n], ocean, (tag, "last", w))
    for w, rec in ref.rec_red.items():
        for n in ref.red:
            for op in ref.ops:
                out = np.full(_shape(kc, npts, n), -7.0, order="F")
                h.window_record_fetch(1, w, n, op, out)
                _equal(kc, n, out, rec[n, op], ocean, (tag, op, w))


def _state_equal(a, b):
    for n in ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "difm", "rho", "wX"):
        assert np.array_equal(np.asarray(getattr(a, n)), np.asarray(getattr(b, n)), equal_nan=True), n


def _forced_pair(mk, ncol, nz, grid, nsteps, origin=1, pl=3, pr=4, land_every=7):
    """The per-step reference and one run_forced of all steps under two schedules, from the same start."""
    res = []
    for one_launch in (False, True):
        kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, land_every=land_every)
        ctx = mk.MckppHip(kc)
        ctx.upload(k3)
        ctx.init_ocean(0)
        ctx.set_flux_series(0, cm.synth.flux_series(ncol, 1, nsteps, kc.dto))
        ocean = k3.run_physics != 0
        if one_launch:
            _schedule(mk, ctx, origin, pl, pr)
            ctx.run_forced(1, nsteps, 1)
        else:
            ref = PerStep(mk, ctx, kc, ncol, origin, pl, pr)
            for nt in range(1, nsteps + 1):
                ctx.run_forced(nt, 1, 1)
                ref.after_step(nt)
        ctx.download(k3)
        res.append((ctx, kc, k3, ocean))
    (c0, kc, k0, ocean), (c1, _, k1, _) = res
    _state_equal(k1, k0)
    _check_records(mk, c1, ref, kc, ncol, ocean)
    return c1, ref


@pytest.mark.parametrize("nz,grid,ncol", [(60, "uniform", 400), (69, "stretched", 300), (100, "uniform", 250)])
def test_records_of_one_forced_run_equal_the_per_step_windows(mk, nz, grid, ncol):
    """12 steps in ONE run_forced with two iodef-like schedules - T, S, hmix "last" every 3 steps; mean, min and max of
    T, S, hmix, difm, wT, rho, Rig and solar_in every 4 - against the per-step API, with land."""
    h, ref = _forced_pair(mk, ncol, nz, grid, 12)
    assert h.window_records(0) == (0, 3) and h.window_records(1) == (0, 2)


def test_records_start_mid_run_and_keep_their_ring(mk):
    """A schedule whose origin is step 3 of a run of 13 steps (steps 1, 2 outside every window), periods 2 and 5."""
    _forced_pair(mk, 300, 60, "uniform", 13, origin=3, pl=2, pr=5)


def test_optional_physics_records(mk):
    """An optional-physics context (L_FCORR_WITHZ, L_DAMP_CURR): tinc_fcorr and dampu_flag among the fields."""
    ncol, nz, nsteps = 260, 60, 8
    red = ("T", "tinc_fcorr", "dampu_flag", "wT")
    res = []
    for one_launch in (False, True):
        kc, k3 = cm.make_hip_case(ncol, nz, land_every=5)
        kc.L_FCORR_WITHZ = 1
        kc.L_DAMP_CURR = 1
        z = np.arange(kc.nzp1)[None, :]
        k3.fcorr_withz[:, :] = 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, ncol)[:, None]
        ctx = mk.MckppHip(kc)
        ctx.upload(k3)
        ctx.init_ocean(0)
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        ctx.set_forcing(k3.sflux)
        ocean = k3.run_physics != 0
        if one_launch:
            ctx.window_schedule(0, 1, 2, 4, ("T", "dampu_flag"), mk.api.WIN_LAST)
            ctx.window_schedule(1, 1, 4, 4, red, mk.api.WIN_MEAN | mk.api.WIN_MIN | mk.api.WIN_MAX)
            ctx.step(1, nsteps)
        else:
            ref = PerStep(mk, ctx, kc, ncol, 1, 2, 4, red=red, last=("T", "dampu_flag"))
            for nt in range(1, nsteps + 1):
                ctx.step(nt, 1)
                ref.after_step(nt)
        ctx.download(k3)
        res.append((ctx, k3))
    _state_equal(res[1][1], res[0][1])
    _check_records(mk, res[1][0], ref, kc, ncol, ocean)


@pytest.mark.parametrize("env", [{"MCKPP_MULTISTEP": "0"}, {"MCKPP_SOLVER_MODE": "1"}, {}])
def test_constant_forcing_step_launch_forms(mk, monkeypatch, env):
    """step(nt, nsteps) with constant forcing: one launch, a launch per step (MCKPP_MULTISTEP=0), and solver mode 1;
    the steps in two calls (1..5, 6..12) to show the schedule carries over from launch to launch."""
    ncol, nz, nsteps = 500, 60, 12
    for k in ("MCKPP_MULTISTEP", "MCKPP_SOLVER_MODE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = []
    for one_launch in (False, True):
        kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
        ctx = mk.MckppHip(kc)
        ctx.upload(k3)
        ctx.init_ocean(0)
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        ctx.set_forcing(k3.sflux)
        ocean = k3.run_physics != 0
        if one_launch:
            _schedule(mk, ctx, 1, 3, 4)
            ctx.step(1, 5)
            ctx.step(6, nsteps - 5)
        else:
            ref = PerStep(mk, ctx, kc, ncol, 1, 3, 4)
            for nt in range(1, nsteps + 1):
                ctx.step(nt, 1)
                ref.after_step(nt)
        ctx.download(k3)
        res.append((ctx, k3))
    _state_equal(res[1][1], res[0][1])
    _check_records(mk, res[1][0], ref, kc, ncol, ocean)


@pytest.mark.parametrize("ncol,nz,nsteps,env", [(64, 100, 12, {}), (300, 60, 10, {}), (64, 60, 12, {"MCKPP_PS": "15x8x2"}),
                                                 (5000, 100, 24, {"MCKPP_SOLO_LIMIT": "1000000"}),
                                                 (300, 60, 10, {"MCKPP_XCC_DROP": "0x55"})])
def test_lagging_columns_finish_their_windows_in_order(mk, monkeypatch, ncol, nz, nsteps, env):
    """Fewer columns than slots, the analytic start, many columns at itermax (the workload of
    test_columns_behind_the_queue_go_on_where_they_are): a column finishes window w while others are windows ahead, so
    a sample taken after the step is published would show here.  One launch of all steps under two schedules against
    a launch per step with the per-step API; each case once."""
    for k in ("MCKPP_PS", "MCKPP_XCC_DROP", "MCKPP_SOLVER_MODE", "MCKPP_SOLO_LIMIT", "MCKPP_MULTISTEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = []
    for one_launch in (False, True):
        kc, k3 = cm.make_hip_case(ncol, nz, land_every=9)
        ctx = mk.MckppHip(kc)
        ctx.upload(k3)
        ctx.init_ocean(0)
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        ctx.set_forcing(k3.sflux)
        ocean = k3.run_physics != 0
        if one_launch:
            _schedule(mk, ctx, 1, 3, 4, red=("T", "hmix", "difm", "Rig"))
            ctx.step(1, nsteps)
        else:
            ref = PerStep(mk, ctx, kc, ncol, 1, 3, 4, red=("T", "hmix", "difm", "Rig"))
            for nt in range(1, nsteps + 1):
                ctx.step(nt, 1)
                ref.after_step(nt)
        ctx.download(k3)
        res.append((ctx, k3))
    _state_equal(res[1][1], res[0][1])
    _check_records(mk, res[1][0], ref, kc, ncol, ocean)


def test_three_shards_equal_the_single_context(mk):
    """Three shards on device 0 behind the multi handle: the records gathered into 3-D order equal the single context's."""
    A = mk.api
    ncol, nz, nsteps = 701, 69, 8
    outs = []
    for shards in (0, 3):
        kc, k3 = cm.make_hip_case(ncol, nz, grid="stretched", land_every=6)
        h = mk.MckppHip(kc) if shards == 0 else mk.MckppHipMulti(kc, [0] * shards)
        h.upload(k3)
        h.init_ocean(0)
        h.set_flux_series(0, cm.synth.flux_series(ncol, 1, nsteps, kc.dto))
        _schedule(mk, h, 1, 2, 4, nrec=2)
        got = {}
        for nt0 in (1, 5):
            h.run_forced(nt0, 4, 1)
            fk, lc = h.window_records(1)
            assert lc == fk
            fk0, lc0 = h.window_records(0)
            for w in range(fk0, lc0 + 1):
                for n in LAST_FIELDS:
                    got[0, w, n] = h.window_record_fetch(0, w, n, A.OP_LAST, np.full(_shape(kc, ncol, n), -7.0, order="F")).copy()
            for n in RED_FIELDS:
                for op in (0, 1, 2):
                    got[1, lc, n, op] = h.window_record_fetch(1, lc, n, op, np.full(_shape(kc, ncol, n), -7.0, order="F")).copy()
            h.window_record_release(0, lc0)
            h.window_record_release(1, lc)
        h.close()   # (before the arrays it has pinned go)
        outs.append((got, k3.run_physics != 0, kc))
    (a, ocean, kc), (b, _, _) = outs
    assert a.keys() == b.keys() and len(a) == 2 * 2 * 3 + 2 * 8 * 3
    for key in a:
        n = key[2]
        _equal(kc, n, b[key], a[key], ocean, key)


def test_errors_leave_the_context_as_it_was(mk):
    """Incomplete and released records, a launch beyond the ring, steps that do not follow on, a diagnostic field with
    the diagnostics off, an unknown field or op, memory that cannot be had: an error with a message, never an abort;
    the refused launch leaves the device state unchanged."""
    A = mk.api
    ncol, nz = 200, 60
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=5)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
    ctx.set_forcing(k3.sflux)
    lib = mk.api._lib()
    out = np.full((ncol, kc.nzp1), -7.0, order="F")
    ctx.step(1, 1)   # step 1 before any schedule
    ctx.window_schedule(0, 1, 2, 2, ["T"], A.WIN_MEAN | A.WIN_LAST)
    ctx.step(2, 3)   # steps 2..4: record 0 (steps 1, 2) began before the schedule, record 1 complete
    with pytest.raises(mk.MckppHipError, match=r"record 0 of schedule 0 \(steps 1\.\.2\) is incomplete"):
        ctx.window_record_fetch(0, 0, "T", A.OP_MEAN, out)
    with pytest.raises(mk.MckppHipError, match=r"record 2 of schedule 0 \(steps 5\.\.6\) is incomplete"):
        ctx.window_record_fetch(0, 2, "T", A.OP_LAST, out)
    assert ctx.window_records(0) == (1, 1)
    ctx.window_record_fetch(0, 1, "T", A.OP_MEAN, out)
    # the ring holds records 1, 2: step 7 would write record 3
    ctx.download(k3)
    before = {n: np.array(getattr(k3, n), copy=True) for n in ("U", "X", "hmix", "Us", "Xs")}
    with pytest.raises(mk.MckppHipError, match=r"ring of 2 records"):
        ctx.step(5, 3)
    ctx.synchronize()
    ctx.download(k3)
    for n, v in before.items():
        assert np.array_equal(np.asarray(getattr(k3, n)), v), n
    with pytest.raises(mk.MckppHipError, match=r"follow on from one another"):
        ctx.step(6, 1)
    ctx.window_record_release(0, 1)
    with pytest.raises(mk.MckppHipError, match=r"record 1 of schedule 0 \(steps 3\.\.4\) has been released"):
        ctx.window_record_fetch(0, 1, "T", A.OP_LAST, out)
    with pytest.raises(mk.MckppHipError, match=r"not complete"):
        ctx.window_record_release(0, 2)
    ctx.step(5, 3)   # records 2 (steps 5, 6) complete, 3 under way
    assert ctx.window_records(0) == (2, 2)
    # a diagnostic field with the diagnostics off: at schedule time, and at the launch if they go off afterwards
    ctx.set_diagnostics(0)
    with pytest.raises(mk.MckppHipError, match=r"diagnostic"):
        ctx.window_schedule(1, 1, 2, 2, ["difm"], A.WIN_MAX)
    ctx.set_diagnostics(1)
    ctx.window_schedule(1, 8, 2, 2, ["difm"], A.WIN_MAX)
    ctx.set_diagnostics(0)
    with pytest.raises(mk.MckppHipError, match=r"diagnostic"):
        ctx.step(8, 1)
    ctx.set_diagnostics(1)
    ctx.window_schedule(1, 1, 1, 1, [], 0)   # cancel
    # unknown field / op and empty masks at the library itself (the wrappers refuse them before)
    f = np.array([99], dtype=np.int32)
    o = np.array([1], dtype=np.uint32)
    import ctypes as C
    assert lib.mckpp_hip_window_schedule(ctx._h, 1, 1, 2, 2, f.ctypes.data_as(C.POINTER(C.c_int32)),
                                         o.ctypes.data_as(C.POINTER(C.c_uint32)), 1) < 0
    assert b"unknown output field 99" in lib.mckpp_hip_last_error()
    f[0] = A.OUT["T"]
    o[0] = 0
    assert lib.mckpp_hip_window_schedule(ctx._h, 1, 1, 2, 2, f.ctypes.data_as(C.POINTER(C.c_int32)),
                                         o.ctypes.data_as(C.POINTER(C.c_uint32)), 1) < 0
    assert b"operations 0x0" in lib.mckpp_hip_last_error()
    assert lib.mckpp_hip_window_record_fetch(ctx._h, 0, 2, A.OUT["T"], 7, out.ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert b"op 7" in lib.mckpp_hip_last_error()
    assert lib.mckpp_hip_window_record_fetch(ctx._h, 0, 2, A.OUT["T"], A.OP_MAX, out.ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert b"keeps no op 2" in lib.mckpp_hip_last_error()
    assert lib.mckpp_hip_window_record_fetch(ctx._h, 0, 2, 99, 0, out.ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert b"field 99 is not in schedule 0" in lib.mckpp_hip_last_error()
    # device memory that cannot be had: the call fails, the schedule is not set, the process goes on
    with pytest.raises(mk.MckppHipError, match=r"cannot allocate"):
        ctx.window_schedule(1, 1, 1, 1 << 30, ["T", "S"], A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX | A.WIN_LAST)
    with pytest.raises(mk.MckppHipError, match=r"schedule 1 is not set"):
        ctx.window_records(1)
    ctx.step(8, 1)   # schedule 0 goes on: record 3 (steps 7, 8) complete
    ctx.window_record_fetch(0, 3, "T", A.OP_LAST, out)
    # upload cancels
    ctx.upload(k3)
    with pytest.raises(mk.MckppHipError, match=r"schedule 0 is not set"):
        ctx.window_records(0)
    ctx.close()


def test_cancelled_schedule_leaves_the_steps_as_never_scheduled(mk):
    """Schedule, cancel, then steps: the state is bit-identical to a context that was never scheduled."""
    ncol, nz, nsteps = 400, 60, 6
    res = []
    for sched in (False, True):
        kc, k3 = cm.make_hip_case(ncol, nz, land_every=7)
        ctx = mk.MckppHip(kc)
        ctx.upload(k3)
        ctx.init_ocean(0)
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        ctx.set_forcing(k3.sflux)
        if sched:
            _schedule(mk, ctx, 1, 2, 3)
            assert ctx.window_records(0) == (0, -1)
            ctx.window_schedule(0, 1, 1, 1, [], 0)
            ctx.window_schedule(1, 1, 1, 1, [], 0)
        ctx.step(1, nsteps)
        ctx.download(k3)
        res.append(k3)
    _state_equal(res[1], res[0])
    for n in ("difs", "dift", "ghat", "wU", "wXNT", "Rig", "Shsq", "buoy", "cp"):
        assert np.array_equal(np.asarray(getattr(res[1], n)), np.asarray(getattr(res[0], n)), equal_nan=True), n
