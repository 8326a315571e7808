"""The prognostic state set or incremented in place from device arrays (include/mckpp_hip_put.h: mckpp_hip_put_dev,
mckpp_hip_put_host and their multi_ twins; k_put_planes).

Yardsticks: tests/golden/ref_loop.npz where a put must change nothing (what fetch_dev delivered put back, an increment
of -0.0); otherwise the honest host edit - download, the arithmetic of the header in numpy (host_put below: one numpy
operation per rounded operation, numpy contracts nothing), upload - on a second context, whose state every later launch
must reproduce.  Every comparison is an equality of bits; no test has a tolerance.

The cases are the small ones of tests/ref_loop_cases.py, which between them reach every path of the kernel:
every_step_nz40 (40 points, every fourth land: one partial tile, land in the map, 41 levels), sweep_nd3 (2000 points
with land: more than 256 columns, tails in the 64- and the 256-column path) and deep_nz100_nd4 (101 levels: two level
tiles).  They run with L_SSref set, the library's default, where Ssurf stays SSref; the same cases with L_SSref = 0 reach
the other branch, Ssurf = X(1,2) + Sref."""
import dataclasses

import numpy as np
import pytest

import ref_loop_cases as lc
from harness import assert_same, flux_args, loop_state, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401
from test_device_arrays_gpu import FILL_BYTES, FILLS, _assert_golden, _bits, _dev, _intervals, _ring_run, _state
from test_device_records_gpu import _too_small
from test_restart_schedule_gpu import _same_bytes
from test_step_log_gpu import _records
from test_window_schedule_gpu import PerStep, _check_records, _schedule

pytestmark = pytest.mark.gpu

LAND = 1e20
CASES = ("every_step_nz40", "sweep_nd3", "deep_nz100_nd4")
STATE = ("u", "v", "T", "S_anom")
FIELD_AT = {"u": ("U", 0), "v": ("U", 1), "T": ("X", 0), "S_anom": ("X", 1), "S": ("X", 1)}   # the array and its slab
REF_OF = {"u": "uref", "v": "vref", "T": "Tref"}
AMPLITUDE = {"u": 1e-4, "v": 1e-4, "T": 1e-3, "S_anom": 1e-4, "S": 1e-4}   # small: the run stays on its path
WRITTEN = ["U", "V", "T", "S", "Us0", "Us1", "Vs0", "Vs1", "Ts0", "Ts1", "Ss0", "Ss1", "Tref", "uref", "vref", "Ssurf"]


def test_the_cases_reach_the_paths_of_the_kernel():
    ncol = {t: len(lc.active_columns(lc.CASES[t])) for t in CASES}
    assert ncol["every_step_nz40"] == 30 and lc.CASES["every_step_nz40"].nz + 1 == 41           # one partial tile, land
    assert ncol["sweep_nd3"] > 256 and ncol["sweep_nd3"] % 256 and ncol["sweep_nd3"] % 64       # tails in both paths
    assert ncol["sweep_nd3"] < lc.CASES["sweep_nd3"].ncol
    assert 64 < lc.CASES["deep_nz100_nd4"].nz + 1 <= 128                                        # two level tiles
    assert all(not lc.CASES[t].switches.get("L_SSref", 1) == 0 for t in CASES)                  # L_SSref as the library sets it


def _case(tag, ssref=1):
    """the case, or the same case with L_SSref = 0 (no golden record: compared with the host edit alone)"""
    case = lc.CASES[tag]
    return case if ssref else dataclasses.replace(case, switches={**case.switches, "L_SSref": 0})


# ---------------------------------------------------------------------------
# the arithmetic of include/mckpp_hip_put.h in numpy, on a downloaded state
# ---------------------------------------------------------------------------
def host_put(k3, kc, planes, op, time_levels=False, skip=None):
    """planes: (field, array (nlev, npts) of float64 or float32, lev0).  The widening, the one add or subtract, the
    skip, both time levels where flagged, and the reference of the field where level 1 was written."""
    ocean = k3.run_physics != 0
    for name, arr, lev0 in planes:
        v = np.asarray(arr).astype(np.float64).T          # widened exactly; (npts, nlev)
        a, l = FIELD_AT[name]
        lv = slice(lev0, lev0 + v.shape[1])
        prof, saved = getattr(k3, a), getattr(k3, a + "s")
        x = prof[:, lv, l].copy()
        keep = ~ocean[:, None] | ((v == skip) if skip is not None else np.zeros(v.shape, dtype=bool))
        if op == "add":
            new = x + v
        elif name == "S":
            new = v - k3.Sref[:, None]
        else:
            new = v.copy()
        new = np.where(keep, x, new)
        prof[:, lv, l] = new
        if time_levels:
            for t in (0, 1):
                xs = saved[:, lv, l, t].copy()
                saved[:, lv, l, t] = np.where(keep, xs, xs + v if op == "add" else new)
        if lev0 == 0:
            wrote = ~keep[:, 0]
            if name in REF_OF:
                getattr(k3, REF_OF[name])[wrote] = new[wrote, 0]
            elif not kc.L_SSref:
                k3.Ssurf[wrote] = (new[:, 0] + k3.Sref)[wrote]


@dataclasses.dataclass
class Spec:
    """One put: the planes as (field, lev0, nlev), the call's keywords, the element type, after which flux intervals"""
    tag: str
    planes: tuple
    op: str = "add"
    dtype: type = np.float64
    time_levels: bool = False
    skip: float = None
    ssref: int = 1
    at: tuple = (0, 1, 2)

    def arrays(self, k3, r):
        """(field, array, lev0) from the downloaded state k3: the increment amplitude * sin(point + level / 10 + r),
        added to the field as it stands where the operation is a set; with a skip value, every third point holds it at
        every level"""
        npts, out = k3.npts, []
        for name, lev0, nlev in self.planes:
            pt, lev = np.arange(npts)[None, :], np.arange(lev0, lev0 + nlev)[:, None]
            v = AMPLITUDE[name] * np.sin(pt + lev / 10.0 + r + 0.5)
            if self.op == "set":
                a, l = FIELD_AT[name]
                now = getattr(k3, a)[:, lev0:lev0 + nlev, l].T
                v = (now + k3.Sref[None, :] if name == "S" else now) + v
            v = np.ascontiguousarray(v.astype(self.dtype))
            if self.skip is not None:
                assert float(self.dtype(self.skip)) == self.skip and not (v == self.skip).any()
                v[:, 1::3] = self.skip
            out.append((name, v, lev0))
        return out

    def kw(self):
        return dict(op=self.op, time_levels=self.time_levels, skip=self.skip)


SPECS = {
    # ADD, f64, whole axis, no flag
    "add_f64_whole_axis": Spec("every_step_nz40", (("T", 0, 41), ("u", 0, 41), ("S_anom", 0, 41)), at=(0, 4, 9)),
    # SET, f32, field S (minus Sref, Ssurf restated: L_SSref = 0), both time levels; a range with lev0 > 0; one level
    "set_f32_S_time_levels": Spec("every_step_nz40", (("S", 0, 41), ("v", 3, 20), ("T", 0, 1)), op="set", dtype=np.float32,
                                  time_levels=True, ssref=0, at=(1, 5, 6)),
    # ADD on field S: X2 + v, a third of the points skipped, Ssurf follows where level 1 was written
    "add_S_skip": Spec("every_step_nz40", (("S", 0, 41), ("v", 0, 1)), skip=-999.0, ssref=0, at=(0, 3)),
    # more than 256 columns: ADD, f32, skip, time levels; the one-level path at level 1 and at the last level
    "add_f32_skip_time_levels": Spec("sweep_nd3", (("v", 3, 20), ("T", 0, 1), ("S_anom", 40, 1), ("u", 0, 41)),
                                     dtype=np.float32, time_levels=True, skip=-999.0, at=(0, 3, 6)),
    # SET, f64, the land value of a fetch as the skip value; S with L_SSref set: Ssurf stays
    "set_f64_skip": Spec("sweep_nd3", (("T", 0, 1), ("S", 0, 41), ("u", 5, 1), ("v", 0, 41)), op="set", skip=LAND, at=(1, 2)),
    "set_f64_S_ssref0": Spec("sweep_nd3", (("S", 0, 41), ("T", 0, 41)), op="set", ssref=0, at=(0, 5)),
    # two level tiles: the whole axis, a range that starts in the first tile and ends in the second
    "deep_add_skip_time_levels": Spec("deep_nz100_nd4", (("T", 0, 101), ("S_anom", 60, 41), ("v", 10, 80)), skip=-999.0,
                                      time_levels=True, at=(0, 1)),
    "deep_set_f32_time_levels": Spec("deep_nz100_nd4", (("T", 0, 101), ("S_anom", 0, 101), ("u", 37, 64), ("v", 0, 1)), op="set",
                                     dtype=np.float32, time_levels=True, at=(0, 1)),
}


def test_the_specs_cover_what_the_kernel_can_be_asked():
    s = SPECS.values()
    assert {x.op for x in s} == {"set", "add"} and {x.dtype for x in s} == {np.float64, np.float32}
    assert any(x.time_levels for x in s) and any(not x.time_levels for x in s) and any(x.skip is not None for x in s)
    planes = [(x, p) for x in s for p in x.planes]
    assert any(p[1] > 0 and p[2] > 1 for _, p in planes) and any(p[2] == 1 and p[1] == 0 for _, p in planes)
    assert any(p[2] == 1 and p[1] > 0 for _, p in planes)
    assert any(p[0] == "S" and x.op == "set" for x, p in planes) and any(p[0] == "S" and x.op == "add" for x, p in planes)
    assert any(p[0] == "S_anom" and x.op == "set" for x, p in planes)
    assert any(p[0] == "S" and p[1] == 0 and not x.ssref for x, p in planes) and any(p[0] == "S" and x.ssref for x, p in planes)
    assert all(max(x.at) < lc.nrec(lc.CASES[x.tag]) - 1 or x.tag == "deep_nz100_nd4" for x in s)   # launches follow


def _written(h, k3, kc, nz):
    h.synchronize()
    d = loop_state(h, k3, kc, nz, names=WRITTEN)
    return {n: d[n] for n in WRITTEN}


def _apply(way, h, k3, kc, spec, arrays):
    if way == "dev":
        h.put_dev([(name, _dev(v), lev0) for name, v, lev0 in arrays], **spec.kw())
    elif way == "host":
        h.put_host([(name, v, lev0) for name, v, lev0 in arrays], **spec.kw())
    else:   # the honest host edit: k3 holds the state _state downloaded
        host_put(k3, kc, arrays, **spec.kw())
        h.upload(k3)


def _same_puts(mk, spec, ways):
    """One context per way - ("dev" | "host" | "edit", shards) - through the case, a launch per flux interval, the put
    after the intervals spec.at: the same state, all of it, after every launch, and the written fields right after
    every put."""
    case = _case(spec.tag, spec.ssref)
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    ctx = [resident(mk, case, shards) for _, shards in ways]
    puts = 0
    for r, nt, n in _intervals(case):
        states = []
        for h, kc, k3 in ctx:
            h.fluxes(nt, *rec[r], **args)
            h.step(nt, n)
            states.append(_state(h, k3, kc, case.nz))
        for (way, shards), got in zip(ways[1:], states[1:]):
            assert_same(got, states[0], active, f"{spec.tag}: {way} x{shards} against {ways[0][0]} after step {nt + n - 1}, {puts} puts")
        if r in spec.at:
            arrays = spec.arrays(ctx[0][2], r)
            before = {k: v.copy() for k, v in states[0].items() if k in WRITTEN}
            for (way, _), (h, kc, k3) in zip(ways, ctx):
                _apply(way, h, k3, kc, spec, arrays)
            after = [_written(h, k3, kc, case.nz) for h, kc, k3 in ctx]
            for (way, shards), got in zip(ways[1:], after[1:]):
                assert_same(got, after[0], active, f"{spec.tag}: {way} x{shards} right after the put behind step {nt + n - 1}")
            assert any(not np.array_equal(after[0][k][active], before[k][active]) for k in before), "the put changed nothing"
            puts += 1
    assert puts == len(spec.at) and np.isfinite(states[0]["T"][active]).all()
    for h, _, _ in ctx:
        h.close()


# ---------------------------------------------------------------------------
# 1. identity against the golden record
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_what_fetch_dev_delivered_put_back_changes_nothing(mk, golden, tag):
    """Between every two launches U, V, T and S_ANOM go out through fetch_dev over the whole axis - land points filled
    with the land value, which a put never reads - and come back through put_dev SET: the same bits in the profiles, and
    the references restated from level 1 are what the step left.  The golden digests hold after every call."""
    import torch

    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    h.flux_ring(2)
    out = {n: torch.empty((case.nz + 1, case.ncol), dtype=torch.float64, device="cuda") for n in STATE}

    def back_and_forth(nt):
        h.fetch_dev([(n, o) for n, o in out.items()], land_value=LAND)
        h.put_dev([(n, o) for n, o in out.items()], op="set", fence=True)
        _assert_golden(golden, tag, nt, h, k3, kc, "fetch_dev put back")

    _ring_run(h, case, 2, lambda r: h.flux_ring_put_dev(r, recd[r]), back_and_forth)
    h.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tag", CASES)
def test_an_increment_of_minus_zero_changes_nothing(mk, golden, tag, dtype):
    """x + (-0.0) is x for every x, signed zeros included: planes of -0.0 added to U, V, T, S_ANOM and to both their time
    levels between every two launches, and the golden digests hold after every call."""
    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    h.flux_ring(2)
    zero = _dev(np.full((case.nz + 1, case.ncol), -0.0, dtype=dtype))
    assert np.signbit(zero.cpu().numpy()).all()

    def add(nt):
        h.put_dev([(n, zero) for n in STATE], op="add", time_levels=True)
        _assert_golden(golden, tag, nt, h, k3, kc, "-0.0 added")

    _ring_run(h, case, 2, lambda r: h.flux_ring_put_dev(r, recd[r]), add)
    h.close()


# ---------------------------------------------------------------------------
# 2. a put is the host edit;  3. put_host is put_dev
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPECS))
def test_put_dev_is_the_host_edit(mk, name):
    _same_puts(mk, SPECS[name], [("dev", 0), ("edit", 0)])


@pytest.mark.parametrize("name", ["add_f32_skip_time_levels", "set_f32_S_time_levels", "deep_set_f32_time_levels"])
def test_put_host_is_put_dev(mk, name):
    _same_puts(mk, SPECS[name], [("dev", 0), ("host", 0)])


# ---------------------------------------------------------------------------
# 5. shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["add_f32_skip_time_levels", "set_f64_S_ssref0", "deep_add_skip_time_levels"])
def test_two_shards_take_the_same_puts(mk, name):
    """MckppHipMulti with two shards on the one device against the single context: the same puts, the same states.  An
    increment that two shards both applied to a point, or that none applied, would show."""
    _same_puts(mk, SPECS[name], [("dev", 0), ("dev", 2), ("host", 2)])


# ---------------------------------------------------------------------------
# 4. nothing is cancelled
# ---------------------------------------------------------------------------
PER_LAUNCH, PL, PR, SNAP = 4, 2, 3, 6   # steps of a launch; periods of the "last" and the mean schedule, of the snapshots


def _book(h):
    return [h.window_records(0), h.window_records(1), h.flux_ring_records(), h.restart_snapshots(), h.step_log_count()[:2]]


def test_a_put_cancels_nothing(mk, tmp_path):
    """every_step_nz40 under two output schedules (T and hmix: last every 2 steps; mean, min, max every 3), a flux ring, a
    step log of every column-step and a restart schedule, in launches of 4 steps with a put - T incremented at every
    level with its time levels, SST and SSS set under "ice" at a third of the points - between them, inside windows 1
    and 2 of the mean.  No launch is refused; the bookkeeping is that of the same run without the puts; and the records,
    the log and the snapshots are those of a context that takes the same puts at the same steps but runs a launch per
    step with window_reset / _accumulate / _fetch, status() and save_restart."""
    A = mk.api
    case = lc.CASES["every_step_nz40"]
    rec, args, npts, nz = lc.flux_records(case), flux_args(case), case.ncol, case.nz
    active, ocean = lc.active_columns(case), lc.ocean(case).astype(bool)
    fields = ("T", "hmix")
    add = Spec("every_step_nz40", (("T", 0, nz + 1),), time_levels=True)
    ice = Spec("every_step_nz40", (("T", 0, 1), ("S", 0, 1)), op="set", skip=LAND)

    def puts(h, k3, kc, r):
        """... from the state as it stands (equal in all contexts that take them): the arrays of both puts"""
        h.synchronize()
        h.download(k3)
        a, b = add.arrays(k3, r), ice.arrays(k3, r)
        h.put_dev([(n, _dev(v), l0) for n, v, l0 in a], **add.kw())
        h.put_host([(n, v, l0) for n, v, l0 in b], **ice.kw())

    # the per-step context
    c, kcc, k3c = resident(mk, case)
    ref = PerStep(mk, c, kcc, npts, 1, PL, PR, red=fields, last=fields)
    events, files = [], {}
    for nt in range(1, case.nsteps + 1):
        c.fluxes(nt, *rec[nt - 1], **args)
        c.step(nt, 1)
        ref.after_step(nt)
        st, _, npass = c.status()
        events += [(nt, int(p), int(st[p]), int(npass[p])) for p in active]
        if nt % SNAP == 0:
            files[nt // SNAP - 1] = tmp_path / f"per_step_{nt}"
            c.save_restart(files[nt // SNAP - 1])
        if nt % PER_LAUNCH == 0 and nt < case.nsteps:
            puts(c, k3c, kcc, nt)
    end_c = _state(c, k3c, kcc, nz)
    c.close()

    # the scheduled contexts: with the puts, and without them for the bookkeeping
    made = []
    for with_puts in (True, False):
        h, kc, k3 = resident(mk, case)
        _schedule(mk, h, 1, PL, PR, nrec=8, red=fields, last=fields)
        h.flux_ring(PER_LAUNCH)
        h.step_log(4096, 1)
        h.restart_schedule(1, SNAP, 2)
        made.append((h, kc, k3))
    (h, kc, k3), (plain, _, _) = made
    for nt in range(1, case.nsteps + 1, PER_LAUNCH):
        for x in (h, plain):
            for r in range(nt - 1, nt - 1 + PER_LAUNCH):
                x.flux_ring_put(r, rec[r])
            x.run_forced(nt, PER_LAUNCH, 1, **args)     # (a refused launch raises)
        assert _book(h) == _book(plain), f"after the launch from step {nt}"
        if nt + PER_LAUNCH <= case.nsteps:
            before = _book(h)
            puts(h, k3, kc, nt + PER_LAUNCH - 1)
            assert _book(h) == before == _book(plain), f"after the put behind step {nt + PER_LAUNCH - 1}"
    assert h.window_records(0) == (0, case.nsteps // PL - 1) and h.window_records(1) == (0, case.nsteps // PR - 1)
    assert h.restart_snapshots() == (0, case.nsteps // SNAP - 1) and h.flux_ring_records() == (case.nsteps - PER_LAUNCH, case.nsteps - 1)
    _check_records(mk, h, ref, kc, npts, ocean, "with puts")
    assert sorted(_records(h)) == sorted(events)
    for s, path in files.items():
        h.restart_snapshot_save(s, tmp_path / f"snapshot_{s}")
        _same_bytes(tmp_path / f"snapshot_{s}", path, f"snapshot {s}")
    end_h, end_plain = _state(h, k3, kc, nz), _state(plain, made[1][2], made[1][1], nz)
    assert_same(end_h, end_c, active, "the end state with puts, scheduled against per step")
    assert not np.array_equal(end_h["T"][active], end_plain["T"][active]), "the puts changed nothing"
    h.close()
    plain.close()


# ---------------------------------------------------------------------------
# 6. ordering on the device
# ---------------------------------------------------------------------------
def test_put_dev_waits_for_its_producer_and_the_fence_holds_the_overwrite(mk):
    """The plane is produced on a side stream behind FILLS fills of FILL_BYTES, put_dev follows at once with no host
    synchronisation, and the tensor is overwritten with NaN on that stream right after dev_fence: a library that read
    too early sets the tensor's earlier content (-1), one whose fence did not hold sets NaN.  A race test can only
    fail, never prove: passing shows no more than that this run was ordered."""
    import torch

    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    npts, nzp1, ocean = case.ncol, case.nz + 1, lc.ocean(case).astype(bool)
    values = 10.0 + np.arange(nzp1 * npts, dtype=np.float64).reshape(nzp1, npts) / 128.0
    src = _dev(values)
    side = torch.cuda.Stream()
    big = torch.empty(FILL_BYTES // 8, dtype=torch.float64, device="cuda")
    t = torch.full((nzp1, npts), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for i in range(FILLS):
            big.fill_(float(i))
        t.copy_(src)
    h.put_dev([("T", t)], op="set", stream=side)
    h.dev_fence(side)
    with torch.cuda.stream(side):
        t.fill_(float("nan"))
    h.synchronize()
    h.download(k3)
    assert np.array_equal(_bits(k3.X[ocean, :, 0]), _bits(values.T[ocean])), "the state does not hold the first values"
    assert np.array_equal(k3.Tref[ocean], values[0, ocean])
    side.synchronize()
    h.close()


# ---------------------------------------------------------------------------
# 7. refusals, before anything is queued
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A = mk.api
    case = lc.CASES["every_step_nz40"]
    npts, nzp1 = case.ncol, case.nz + 1
    rec, args = lc.flux_records(case), flux_args(case)
    h, kc, k3 = resident(mk, case)
    _schedule(mk, h, 1, PL, PR, nrec=8, red=("T", "hmix"), last=("T", "hmix"))
    h.flux_ring(4)
    h.step_log(4096, 1)
    h.restart_schedule(1, 2, 4)
    for r in range(4):
        h.flux_ring_put(r, rec[r])
    h.run_forced(1, 4, 1, **args)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()
    P = A._PutPlaneC

    def everything():
        s = _state(h, k3, kc, case.nz)
        return _book(h), {k: _bits(np.nan_to_num(v.astype(np.float64))).copy() for k, v in s.items()}

    before = everything()
    good = torch.zeros((nzp1, npts), dtype=torch.float64, device="cuda")
    pinned = torch.zeros(npts * nzp1, dtype=torch.float64).pin_memory()
    pageable = np.zeros(npts * nzp1)
    big, small, holds = _too_small(torch, npts * nzp1 * 8)
    ok = dict(field=A.OUT["T"], lev0=0, nlev=nzp1, dtype=A.EXP_F64, op=A.PUT_ADD, flags=0, skip_value=0.0)
    forms = {"mckpp_hip_put_dev": lambda n, tab: lib.mckpp_hip_put_dev(h._h, n, tab, None),
             "mckpp_hip_put_host": lambda n, tab: lib.mckpp_hip_put_host(h._h, n, tab)}
    ptr = {"mckpp_hip_put_dev": good.data_ptr(), "mckpp_hip_put_host": pageable.ctypes.data}

    def refused(text, k=0, only=None, first=None, **swap):
        """plane k of a table of k + 1 is the bad one; `first` changes the good planes before it"""
        for name, call in forms.items():
            if only and name != only:
                continue
            base = P(**{**ok, **(first or {})}, **{"in": ptr[name]})
            bad = P(**{**{**ok, "in": ptr[name]}, **swap})
            tab = (P * (k + 1))(*([base] * k + [bad]))
            assert call(k + 1, tab) < 0, (name, text)
            assert err().startswith(name + ": ") and f"planes[{k}]" in err() and text in err(), err()

    refused("unknown output field 99", field=99)
    refused("unknown output field -1", field=-1)
    refused("field 4 is an output of the step, not state", field=A.OUT["hmix"], nlev=1)
    refused("field 16 is an output of the step, not state", k=1, first=dict(nlev=3), field=A.OUT["rho"])
    refused("field 13 is an output of the step", field=A.OUT["difm"])
    refused("lev0=1 nlev=41 is no range of levels of field 2, whose axis has 41", lev0=1)
    refused("lev0=0 nlev=0 is no range", nlev=0)
    refused("lev0=-1 nlev=2 is no range", lev0=-1, nlev=2)
    refused("lev0=41 nlev=1 is no range", field=A.OUT["S"], lev0=41, nlev=1)
    refused("dtype 7 (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", dtype=7)
    refused("dtype 0", dtype=0)
    refused("op 2 (MCKPP_PUT_SET 0, MCKPP_PUT_ADD 1)", op=2)
    refused("op -1", op=-1)
    refused("flags 0x4", flags=4)
    refused("flags 0x9", flags=9)
    refused("the skip value is NaN", flags=A.PUT_SKIP, skip_value=float("nan"))
    refused("planes[1] and planes[0] write the same field (2, 2) at overlapping levels 5..7 and 0..9", k=1,
            first=dict(nlev=10), lev0=5, nlev=3)
    refused("planes[1] and planes[0] write the same field (5, 3) at overlapping levels 40..40 and 40..40", k=1,
            first=dict(field=A.OUT["S_anom"], lev0=40, nlev=1), field=A.OUT["S"], lev0=40, nlev=1)
    dev, host = "mckpp_hip_put_dev", "mckpp_hip_put_host"
    refused("planes[0].in is pinned host memory", only=dev, **{"in": pinned.data_ptr()})
    refused("planes[1].in is host memory", only=dev, k=1, first=dict(field=A.OUT["u"]), **{"in": pageable.ctypes.data})
    refused("planes[0].in is null", only=dev, **{"in": None})
    refused(f"planes[0].in: the allocation holds {holds} bytes from the pointer on, the call needs {npts * nzp1 * 8}", only=dev,
            **{"in": small.data_ptr()})
    refused("planes[0].in is null", only=host, **{"in": None})
    # the table itself, and a context without a state: no plane to name
    tab = (P * 65)(*[P(**ok, **{"in": good.data_ptr()})] * 65)
    for name, call in forms.items():
        assert call(65, tab) < 0 and f"{name}: nplanes=65 (0..64)" in err()
        assert call(1, None) < 0 and f"{name}: nplanes=1 (0..64) or a null table" in err()
        assert call(-1, tab) < 0 and "nplanes=-1" in err()
        assert call(0, None) == 0 and call(0, tab) == 0
    fresh = mk.MckppHip(kc)
    assert lib.mckpp_hip_put_dev(fresh._h, 1, tab, None) < 0 and err() == "mckpp_hip_put_dev: upload the state first"
    assert lib.mckpp_hip_put_host(fresh._h, 1, tab) < 0 and err() == "mckpp_hip_put_host: upload the state first"
    fresh.close()
    # a multi handle checks every plane of every shard before any shard queues
    m, kcm, k3m = resident(mk, case, shards=2)
    m_before = {k: v.copy() for k, v in _state(m, k3m, kcm, case.nz).items()}
    tab2 = (P * 2)(P(**ok, **{"in": good.data_ptr()}), P(**{**ok, "field": A.OUT["u"], "in": pinned.data_ptr()}))
    assert lib.mckpp_hip_multi_put_dev(m._h, 2, tab2, None) < 0
    assert err().startswith("mckpp_hip_multi_put_dev: planes[1].in is pinned host memory"), err()
    tab2[1] = P(**{**ok, "lev0": 3, "nlev": 2, "in": good.data_ptr()})
    assert lib.mckpp_hip_multi_put_host(m._h, 2, tab2) < 0 and "mckpp_hip_multi_put_host: planes[1] and planes[0]" in err()
    assert_same(_state(m, k3m, kcm, case.nz), m_before, slice(None), "the shards after the refusals")
    m.close()
    # the Python layer's texts, and the library's through it
    with pytest.raises(ValueError, match=rf"planes\[0\] array: shape \({small.numel()},\), the call takes {npts * nzp1} elements"):
        h.put_dev([("T", small, 0, nzp1)])
    with pytest.raises(ValueError, match="a host array"):
        h.put_dev([("T", pinned)])
    after = everything()
    assert after[0] == before[0], "a refused put touched the schedules' bookkeeping"
    assert after[1].keys() == before[1].keys() and all(np.array_equal(after[1][k], before[1][k]) for k in before[1]), \
        "a refused put touched the state"
    assert not good.cpu().numpy().any()
    # ... and the run goes on: a good put, the next launch under every schedule
    h.put_dev([("T", good)], op="add")
    for r in range(4, 8):
        h.flux_ring_put(r, rec[r])
    h.run_forced(5, 4, 1, **args)
    assert h.window_records(1) == (0, 1) and h.restart_snapshots()[1] == 3
    h.close()
