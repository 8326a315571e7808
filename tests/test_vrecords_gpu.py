"""Completed records on a caller axis (include/mckpp_hip_vrecords.h: mckpp_hip_vrecords_vaxis_dev, _vaxis_host, _hv_dev
and their multi_ twins; k_vaxis_record_planes, and k_hgrid_out behind it).

Every value comparison is an equality of bits; no test has a tolerance and none skips a case.  The yardsticks are the
existing calls and the two numpy restatements:
  on the record's points  vaxis_ref.vinterp(zm of the kept levels, x, z of the axis) with x mckpp_hip_window_record_fetch
                          of the same schedule, record, field and op - a mean is divided before anything else;
  on a caller grid        hgrid_ref.apply(out table, that plane at each caller level, n, used = the points that are rows
                          of the record, norm, fill);
  where the table's rows meet  a last-step record of period 1 against mckpp_hip_vaxis_fetch_dev / mckpp_hip_hv_fetch_dev.
The contexts are tests/test_remap_gpu.py's Recorded - every_step_nz40 (30 columns of 40 points: one partial 64-row tile,
land, 41 levels), sweep_nd3 (more than 256 columns, tails), deep_nz100_nd4 (101 levels: source rows past one 64-level
tile); schedule 0 unlisted with the whole axis, schedule 1 with a point list and the level zoom KEPT, every op, period 3
in a ring of two, two records complete - and the axes are tests/test_vrecords_cpu.py's caller_axes, which that file
holds to what they claim.  Inputs hold no NaN."""
import numpy as np
import pytest

import hgrid_ref as hr
import ref_loop_cases as lc
import vaxis_ref as vr
from harness import assert_same, flux_args, mk, resident  # noqa: F401
from test_device_arrays_gpu import _bits, _dev, _state
from test_remap_gpu import PERIOD, ZLEV, _define, recorded  # noqa: F401
from test_vaxis_gpu import _short_of
from test_vrecords_cpu import CASES, KEPT, caller_axes, first_outside

pytestmark = pytest.mark.gpu

LAND = hr.LAND
AXES = ("two", "coarse7", "fine130", "equal", "tiles100", "clamps", "inside", "one_out")   # axis numbers 0 .. 7
AX = {a: i for i, a in enumerate(AXES)}
NAMES = ("T", "S")            # S holds Sref already: nothing is added a second time
assert KEPT == ZLEV


# ---------------------------------------------------------------------------
# the contexts and the restatement
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def axed(recorded):  # noqa: F811
    """recorded(tag, shards) with the eight axes defined on its handle"""
    def get(tag, shards=0):
        r = recorded(tag, shards)
        if not hasattr(r, "ax"):
            r.zm = np.array(r.kc.zm[:r.nzp1], dtype=np.float64)
            r.ax = caller_axes(r.zm)
            assert sorted(r.ax) == sorted(AXES)
            for a in AXES:
                r.h.vaxis_define(AX[a], r.ax[a])
            r.src = {}
        return r

    return get


def _source(r, s, rec, name, op):
    """(levels kept, npts): Recorded.source, fetched once"""
    key = (s, rec, name, op)
    if key not in r.src:
        r.src[key] = r.source(s, rec, name, op)
    return r.src[key]


def _on_axis(r, s, rec, name, op, a):
    """(n_axis, npts) on the model's points: vinterp of the record's plane from the levels the schedule keeps; whatever
    it makes of the 5e33 of a point without a row is never looked at"""
    zs = r.zm if s == 0 else r.zm[ZLEV[0]:ZLEV[0] + ZLEV[1]]
    with np.errstate(all="ignore"):
        return vr.vinterp(zs, _source(r, s, rec, name, op), r.ax[a])


def _point_axis(r, s):
    """(point numbers in the order of the schedule's point axis, which of them are rows of its records)"""
    pos = np.arange(r.npts) if s == 0 else np.asarray(r.pts)
    return pos, r.ocean[pos] != 0


def _vaxis_planes():
    """(sched, rec, field, op, axis): every axis and every op from the unlisted schedule, fields and records in turn;
    every op of both fields from the zoomed one through the axis inside its kept levels"""
    out = [(0, (i + op) % 2, NAMES[(i + op // 2) % 2], op, a) for i, a in enumerate(AXES) for op in range(4)]
    out += [(1, (i + op) % 2, name, op, "inside") for i, name in enumerate(NAMES) for op in range(4)]
    assert len(out) <= 64
    return out


def _check_vaxis(r, h, dtype, fill, what, host=False):
    """one call of h - r's context, or another that holds the same records - for all planes, each against the
    restatement applied to r's records"""
    calls, outs, wants = [], [], []
    for k, (s, rec, name, op, a) in enumerate(_vaxis_planes()):
        pos, isrow = _point_axis(r, s)
        held = np.random.default_rng(300 + k).uniform(-3.0, 3.0, (len(r.ax[a]), len(pos))).astype(dtype)
        plane = _on_axis(r, s, rec, name, op, a)[:, pos]
        assert isrow.any() and np.isfinite(plane[:, isrow]).all() and (np.abs(plane[:, isrow]) < 1e6).all(), \
            "a position that is no row was read"
        want = plane.astype(dtype)                       # a float plane is one final conversion
        want[:, ~isrow] = dtype(LAND) if fill else held[:, ~isrow]
        o = held.copy() if host else _dev(held)
        calls.append((s, rec, name, op, AX[a], o))
        outs.append(o)
        wants.append(want)
    if host:
        h.vaxis_records_host(calls, land_value=LAND, fill_land=fill)
    else:
        h.vaxis_records_dev(calls, land_value=LAND, fill_land=fill)
    for c, o, want in zip(calls, outs, wants):
        got = o if host else o.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (what, c[:5], np.dtype(dtype).name, fill, "host" if host else "dev")
    return wants


def _hv_planes():
    """(sched, rec, field, op, grid, axis): both grids, every op, the axes of every branch; the zoomed schedule through
    the axis inside its kept levels"""
    return [(0, 1, "T", 0, 0, "coarse7"), (0, 0, "S", 1, 1, "fine130"), (0, 1, "S", 2, 0, "equal"), (0, 0, "T", 3, 1, "clamps"),
            (0, 1, "S", 0, 1, "tiles100"), (0, 0, "T", 0, 0, "two"), (1, 1, "T", 0, 1, "inside"), (1, 0, "S", 3, 0, "inside"),
            (1, 1, "S", 1, 1, "inside"), (1, 0, "T", 2, 0, "inside")]


def _check_hv(r, h, dtype, norm, fill, what):
    calls, outs, wants = [], [], []
    for k, (s, rec, name, op, g, a) in enumerate(_hv_planes()):
        n, _, tout = r.tabs[g]
        nax = len(r.ax[a])
        held = np.random.default_rng(500 + k).uniform(-3.0, 3.0, (nax, n)).astype(dtype)
        plane = _on_axis(r, s, rec, name, op, a)
        want = np.stack([hr.apply(tout, plane[j], n, r.used(s), norm, fill, LAND, held[j].astype(np.float64)) for j in range(nax)])
        assert np.isfinite(want).all() and (np.abs(want[want != LAND]) < 1e6).all(), "a position that is no row was read"
        o = _dev(held)
        calls.append((s, rec, name, op, g, AX[a], o))
        outs.append(o)
        wants.append(want.astype(dtype))
    h.hv_records_dev(calls, norm=norm, land_value=LAND, fill_land=fill)
    for c, o, want in zip(calls, outs, wants):
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), (what, c[:6], np.dtype(dtype).name, norm, fill)
    return wants


# ---------------------------------------------------------------------------
# 1. - 3. the three calls against the restatements
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_vaxis_records_dev_is_vinterp_of_window_record_fetch(mk, axed, tag, dtype, fill):
    r = axed(tag)
    wants = _check_vaxis(r, r.h, dtype, fill, tag)
    # the mean was divided before it was interpolated: interpolating the sums and dividing afterwards differs somewhere
    s, rec, name, op, a = _vaxis_planes()[4 * AX["fine130"]]
    assert op == 0 and s == 0
    _, isrow = _point_axis(r, 0)
    sums = _source(r, 0, rec, name, 0) * float(PERIOD)
    late = vr.vinterp(r.zm, sums, r.ax[a])[:, isrow] / float(PERIOD)
    assert not np.array_equal(late.astype(dtype), wants[4 * AX["fine130"]][:, isrow]) or dtype is np.float32


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("norm", hr.NORMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_hv_records_dev_is_the_row_sum_of_those_planes(mk, axed, tag, dtype, norm, fill):
    r = axed(tag)
    _check_hv(r, r.h, dtype, norm, fill, tag)


@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_a_caller_point_that_reads_only_unlisted_points_gets_the_land_value(mk, axed, tag):
    """tests/test_remap_gpu.py's grid 2, at every caller level: caller point 0 reads listed resident points, point 1
    resident points that are not in the list, point 2 both"""
    import torch

    r = axed(tag)
    listed = r.pts[r.ocean[r.pts] != 0]
    others = np.setdiff1d(np.nonzero(r.ocean)[0], r.pts)
    tout = hr.csr([[(int(listed[0]), 0.5), (int(listed[1]), 0.25)], [(int(others[0]), 0.5), (int(others[1]), 0.5)],
                   [(int(others[2]), 0.5), (int(listed[2]), 0.75), (int(others[0]), -0.25)]])
    r.h.hgrid_define(2, 3, None, tout)
    nax = len(r.ax["inside"])
    a, b = (torch.zeros((nax, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    r.h.hv_records_dev([(0, 1, "T", 0, 2, AX["inside"], a), (1, 1, "T", 0, 2, AX["inside"], b)], norm="none", land_value=LAND)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    whole, zoom = _on_axis(r, 0, 1, "T", 0, "inside"), _on_axis(r, 1, 1, "T", 0, "inside")
    for j in range(nax):
        assert np.array_equal(_bits(a[j]), _bits(hr.apply(tout, whole[j], 3, r.used(0), "none")))
        assert np.array_equal(_bits(b[j]), _bits(hr.apply(tout, zoom[j], 3, r.used(1), "none")))
    assert LAND not in a and (b[:, 1] == LAND).all() and (b[:, 0] != LAND).all()
    assert np.array_equal(b[:, 2], 0.75 * zoom[:, listed[2]]) and not np.array_equal(b[:, 2], a[:, 2])
    # the zoomed record and the whole one hold the same values at the kept levels: rebased kin reads the same elements
    assert np.array_equal(_bits(whole[:, listed]), _bits(zoom[:, listed]))
    r.h.hgrid_define(2, 0)


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_vaxis_records_host_delivers_the_same_bits_into_numpy_arrays(mk, axed, tag, dtype, fill):
    r = axed(tag)
    _check_vaxis(r, r.h, dtype, fill, tag, host=True)


# ---------------------------------------------------------------------------
# 4. two shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_two_shards_deliver_the_single_contexts_bits(mk, axed, tag):
    """a multi handle of two shards against the restatement applied to the single context's records, for all three
    calls: a shard writes its own points, shard 0 the positions no shard holds; on a grid the used entries are the rows
    of any shard"""
    r, m = axed(tag), axed(tag, 2)
    mask0, n0 = mk.api.host_shard_mask(m.k3.run_physics, 2, 0)
    assert 0 < n0 < len(lc.active_columns(r.case)), "both shards hold columns"
    for dtype, norm, fill in ((np.float64, "used", True), (np.float32, "none", False)):
        _check_vaxis(r, m.h, dtype, fill, f"{tag}, two shards")
        _check_vaxis(r, m.h, dtype, fill, f"{tag}, two shards", host=True)
        _check_hv(r, m.h, dtype, norm, fill, f"{tag}, two shards")
    # ... and a shard's tables follow who addresses it: the single context again, unchanged
    _check_vaxis(r, r.h, np.float64, True, f"{tag}, the single context afterwards")
    _check_hv(r, r.h, np.float64, "used", True, f"{tag}, the single context afterwards")


# ---------------------------------------------------------------------------
# 5. ordering
# ---------------------------------------------------------------------------
def test_a_ring_of_one_record_is_released_and_overwritten_behind_the_delivery(mk):
    """A level zoom with nrec = 1: step, vaxis_records_dev and hv_records_dev, release at once, the next steps at once,
    with no synchronisation anywhere in the loop; compared afterwards with a second context that fetches before it
    releases.  A race test can only fail, never prove."""
    import torch

    A = mk.api
    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    ref, _, _ = resident(mk, case)
    tabs = _define(h, case)
    zm = np.array(kc.zm[:case.nz + 1], dtype=np.float64)
    z = caller_axes(zm)["inside"]
    zs = zm[ZLEV[0]:ZLEV[0] + ZLEV[1]]
    h.vaxis_define(0, z)
    what, nwin, g = [("T", 0), ("S", 3)], 4, 1
    n, _, tout = tabs[g]
    for x in (h, ref):
        x.window_schedule_zoom(0, 1, PERIOD, 1, NAMES, A.WIN_MEAN | A.WIN_LAST, levels=ZLEV)
        x.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    outs = [[torch.full((len(z), case.ncol), -7.0, dtype=torch.float64, device="cuda") for _ in what] for _ in range(nwin)]
    gouts = [[torch.full((len(z), n), -7.0, dtype=torch.float64, device="cuda") for _ in what] for _ in range(nwin)]
    torch.cuda.synchronize()
    for w in range(nwin):
        h.step(w * PERIOD + 1, PERIOD)
        h.vaxis_records_dev([(0, w, name, op, 0, o) for (name, op), o in zip(what, outs[w])], land_value=LAND)
        h.hv_records_dev([(0, w, name, op, g, 0, o) for (name, op), o in zip(what, gouts[w])], norm="used", land_value=LAND)
        h.window_record_release(0, w)
    ocean = lc.ocean(case)
    for w in range(nwin):
        ref.step(w * PERIOD + 1, PERIOD)
        for (name, op), o, go in zip(what, outs[w], gouts[w]):
            x = np.full((case.ncol, ZLEV[1]), 5e33, order="F")
            ref.window_record_fetch(0, w, name, op, x)
            with np.errstate(all="ignore"):
                plane = vr.vinterp(zs, np.ascontiguousarray(x.T), z)
            want = np.where(ocean[None, :] != 0, plane, LAND)
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), ("record", w, name, op)
            gwant = np.stack([hr.apply(tout, plane[j], n, ocean, "used", True, LAND) for j in range(len(z))])
            assert np.array_equal(_bits(go.cpu().numpy()), _bits(gwant)), ("record on the grid", w, name, op)
        ref.window_record_release(0, w)
    h.close()
    ref.close()


# ---------------------------------------------------------------------------
# 6. where the new row of the table meets the old one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["every_step_nz40", "deep_nz100_nd4"])
def test_a_last_step_record_of_period_one_is_vaxis_fetch_dev_and_hv_fetch_dev(mk, tag):
    import torch

    A = mk.api
    case = lc.CASES[tag]
    h, kc, k3 = resident(mk, case)
    tabs = _define(h, case)
    ax = caller_axes(np.array(kc.zm[:case.nz + 1], dtype=np.float64))
    for a in AXES:
        h.vaxis_define(AX[a], ax[a])
    h.window_schedule(0, 1, 1, 1, NAMES, A.WIN_LAST | A.WIN_MEAN)
    h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    for nt in (1, 2):
        h.step(nt, 1)
        for dtype in (torch.float64, torch.float32):
            pairs = []
            for name in NAMES:
                for a in ("coarse7", "fine130", "equal", "clamps"):
                    new, old = (torch.full((len(ax[a]), case.ncol), -3.0, dtype=dtype, device="cuda") for _ in range(2))
                    pairs.append((name, a, new, old))
            h.vaxis_records_dev([(0, nt - 1, name, A.OP_LAST, AX[a], new) for name, a, new, _ in pairs], land_value=LAND)
            h.vaxis_fetch_dev([(name, AX[a], old) for name, a, _, old in pairs], land_value=LAND)
            for name, a, new, old in pairs:
                assert np.array_equal(_bits(new.cpu().numpy()), _bits(old.cpu().numpy())), (tag, nt, name, a, dtype)
                assert (old.cpu().numpy() != -3.0).all()
            g, n = 1, tabs[1][0]
            gp = [(name, a, *(torch.full((len(ax[a]), n), -3.0, dtype=dtype, device="cuda") for _ in range(2)))
                  for name in NAMES for a in ("coarse7", "tiles100")]
            for norm in hr.NORMS:
                h.hv_records_dev([(0, nt - 1, name, A.OP_LAST, g, AX[a], new) for name, a, new, _ in gp], norm=norm, land_value=LAND)
                h.hv_fetch_dev([(name, g, AX[a], old) for name, a, _, old in gp], norm=norm, land_value=LAND)
                for name, a, new, old in gp:
                    assert np.array_equal(_bits(new.cpu().numpy()), _bits(old.cpu().numpy())), (tag, nt, name, a, dtype, norm)
        h.window_record_release(0, nt - 1)
    h.close()


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.api.MckppHipError
    tag = "every_step_nz40"
    case = lc.CASES[tag]
    npts, nzp1 = case.ncol, case.nz + 1
    h, kc, k3 = resident(mk, case)
    tabs = _define(h, case)
    g, n = 1, tabs[1][0]
    h.hgrid_define(3, 5, hr.csr([[(0, 1.0)]] * npts), None)     # no out table
    ax = caller_axes(np.array(kc.zm[:nzp1], dtype=np.float64))
    for a in AXES[:7]:
        h.vaxis_define(AX[a], ax[a])                            # axis 7 stays undefined
    h.vaxis_define(5, ax["one_out"])                            # ... and axis 5 reads one level outside schedule 1's zoom
    nin, nout = len(ax["inside"]), len(ax["one_out"])
    axis_levels = [len(ax[a]) for a in AXES[:5]] + [nout, nin]      # of axes 0 .. 6 as they now stand
    pts = np.array([5, 2, 9, 11], dtype=np.int32)
    h.window_schedule(0, 1, 2, 2, ("T", "hmix", "difm"), A.WIN_MEAN | A.WIN_LAST)
    h.window_schedule_zoom(1, 1, PERIOD, 2, ("T",), A.WIN_MEAN | A.WIN_MIN, points=pts, levels=ZLEV)
    h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    h.step(1, 4)                                                # schedule 0: records 0, 1 complete; schedule 1: record 0
    h.window_record_release(0, 0)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()

    def everything():
        s = _state(h, k3, kc, case.nz)
        recs = []
        for s_, rec, name, op, shape in ((0, 1, "T", 0, (npts, nzp1)), (1, 0, "T", 1, (len(pts), ZLEV[1]))):
            x = np.full(shape, 5e33, order="F")
            h.window_record_fetch(s_, rec, name, op, x)
            recs.append(_bits(x).copy())
        # the axes: what a fetch through each of the seven defined ones delivers, and that the eighth is still undefined
        through = [torch.zeros((nlev, npts), dtype=torch.float64, device="cuda") for nlev in axis_levels]
        h.vaxis_fetch_dev([("T", k, t) for k, t in enumerate(through)], land_value=LAND)
        recs += [_bits(t.cpu().numpy()).copy() for t in through]
        with pytest.raises(ValueError, match="axis 7 is not defined"):
            h.vaxis_fetch_dev([("T", 7, through[0])])
        return ([h.window_records(0), h.window_records(1), h.window_zoom(1)[:3]] + [h.hgrid_info(k) for k in range(2)], recs,
                {k: _bits(np.nan_to_num(v.astype(np.float64))).copy() for k, v in s.items()})

    before = everything()
    out = torch.full((nout, max(n, npts)), -5.0, dtype=torch.float64, device="cuda")
    good = torch.zeros((nout, max(n, npts)), dtype=torch.float64, device="cuda")
    pinned = torch.zeros(nout * max(n, npts), dtype=torch.float64).pin_memory()
    pageable = np.full(nout * max(n, npts), -5.0)
    V, H = A._VaxisRecordPlaneC, A._HvRecordPlaneC
    vok = dict(sched=1, field=A.OUT["T"], op=0, axis=AX["inside"], dtype=A.EXP_F64, fill_land=1, rec=0, land_value=LAND,
               out=out.data_ptr())
    hok = dict(vok, grid=g, norm=0)
    big, small, holds = _short_of(torch, len(pts) * nin * 8)        # an address one double short of a plane of schedule 1
    bigg, smallg, holdsg = _short_of(torch, n * nin * 8)            # ... and of a plane on grid 1

    def vdev(*planes):
        return lib.mckpp_hip_vrecords_vaxis_dev(h._h, len(planes), (V * len(planes))(*[V(**{**vok, **p}) for p in planes]), None)

    def vhost(*planes):
        tab = (V * len(planes))(*[V(**{**vok, "out": pageable.ctypes.data, **p}) for p in planes])
        return lib.mckpp_hip_vrecords_vaxis_host(h._h, len(planes), tab)

    def hv(*planes):
        return lib.mckpp_hip_vrecords_hv_dev(h._h, len(planes), (H * len(planes))(*[H(**{**hok, **p}) for p in planes]), None)

    vname, hname, oname = "mckpp_hip_vrecords_vaxis_dev: ", "mckpp_hip_vrecords_hv_dev: ", "mckpp_hip_vrecords_vaxis_host: "
    hi = ZLEV[0] + ZLEV[1] - 1
    rule = (f"planes[0]: caller level {nout - 1} of axis 5 (z={ax['one_out'][-1]:.17g}) reads model level {hi + 1}, and schedule 1 "
            f"keeps levels {ZLEV[0]}..{hi} of field {A.OUT['T']}")
    zm = np.array(kc.zm[:nzp1], dtype=np.float64)
    assert first_outside(zm, ax["one_out"], *ZLEV) == (nout - 1, hi + 1)
    c7, c7top = first_outside(zm, ax["coarse7"], *ZLEV), first_outside(zm, ax["coarse7"], 0, 1)
    table = []
    for call, name in ((vdev, vname), (hv, hname), (vhost, oname)):
        table += [
            # what records_dev refuses of the plane
            (lambda c=call: c(dict(sched=2)), name + "planes[0]: schedule 2 is not set"),
            (lambda c=call: c(dict(sched=9)), name + "planes[0]: schedule 9"),
            (lambda c=call: c({}, dict(rec=1)), name + "planes[1]: record 1 of schedule 1 (steps 4..6) is incomplete: steps have run up to 4"),
            (lambda c=call: c(dict(sched=0, op=3, rec=0, axis=0)), name + "planes[0]: record 0 of schedule 0 (steps 1..2) has been released"),
            (lambda c=call: c(dict(field=A.OUT["S"])), name + f"planes[0]: field {A.OUT['S']} is not in schedule 1"),
            (lambda c=call: c(dict(op=3)), name + "planes[0]: schedule 1 keeps no op 3 of field 2"),
            (lambda c=call: c(dict(op=4)), name + "planes[0]: op 4 (0 mean, 1 min, 2 max, 3 last)"),
            (lambda c=call: c(dict(dtype=7)), name + "planes[0]: dtype 7"),
            # the axis and the field
            (lambda c=call: c(dict(axis=7)), name + "planes[0]: axis 7 is not defined"),
            (lambda c=call: c({}, dict(axis=-1)), name + "planes[1]: axis -1 is not defined"),
            (lambda c=call: c(dict(sched=0, rec=1, field=A.OUT["hmix"], axis=0)), name + "planes[0]: field 4 (hmix) is two-dimensional"),
            (lambda c=call: c(dict(sched=0, rec=1, field=A.OUT["difm"], axis=0)),
             name + f"planes[0]: field {A.OUT['difm']} (difm) lives on the interface axis"),
            (lambda c=call: c(dict(field=99)), name + "planes[0]: unknown output field 99"),
            # the level rule
            (lambda c=call: c(dict(axis=5)), name + rule),
            (lambda c=call: c(dict(axis=AX["coarse7"])),
             name + "planes[0]: caller level %d of axis 1 (z=%.17g) reads model level %d, and" % (c7[0], ax["coarse7"][c7[0]], c7[1])),
            (lambda c=call: c(dict(out=None)), name + "planes[0].out is null"),
            (lambda c=call, f=getattr(lib, name[:-2]): f(h._h, 65, None, *([None] if c is not vhost else [])), name + "nplanes=65 (0..64)"),
            (lambda c=call, f=getattr(lib, name[:-2]): f(h._h, 1, None, *([None] if c is not vhost else [])),
             name + "nplanes=1 (0..64) or a null table"),
        ]
    table += [
        # the device forms' arrays
        (lambda: vdev(dict(out=small)),
         vname + f"planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {len(pts) * nin * 8}"),
        (lambda: vdev(dict(out=pageable.ctypes.data)), vname + "planes[0].out is host memory"),
        (lambda: vdev({}, dict(out=pinned.data_ptr())), vname + "planes[1].out is pinned host memory"),
        (lambda: hv(dict(out=smallg)),
         hname + f"planes[0].out: the allocation holds {holdsg} bytes from the pointer on, the call needs {n * nin * 8}"),
        (lambda: hv(dict(out=pageable.ctypes.data)), hname + "planes[0].out is host memory"),
        # what remap_records_dev refuses of the grid
        (lambda: hv(dict(grid=-1)), hname + "planes[0]: grid -1 is not defined"),
        (lambda: hv(dict(grid=2)), hname + "planes[0]: grid 2 is not defined"),
        (lambda: hv({}, dict(grid=3, out=good.data_ptr())), hname + "planes[1]: grid 3 has no out table"),
        (lambda: hv(dict(norm=2)), hname + "planes[0]: norm 2 (MCKPP_HGRID_NORM_NONE 0, MCKPP_HGRID_NORM_USED 1)"),
        (lambda: hv({}, dict(out=out.data_ptr() + 8 * n)), hname + "planes[1].out and planes[0].out overlap"),
    ]
    for call, text in table:
        assert call() < 0, text
        assert text in err(), (text, err())
    assert vdev() == 0 and hv() == 0 and vhost() == 0        # no plane: nothing to do
    # no state uploaded; a grid defined for another npts
    fresh = mk.MckppHip(kc)
    assert lib.mckpp_hip_vrecords_vaxis_dev(fresh._h, 1, (V * 1)(V(**vok)), None) < 0 and err() == vname + "upload the state first"
    assert lib.mckpp_hip_vrecords_hv_dev(fresh._h, 1, (H * 1)(H(**hok)), None) < 0 and err() == hname + "upload the state first"
    fresh.close()
    other = lc.CASES["l_rest"]
    assert other.ncol != npts and other.nz == case.nz
    o, kco, k3o = resident(mk, other)
    o.hgrid_define(0, 5, None, hr.csr([[(0, 1.0)]] * 5))
    o.vaxis_define(0, ax["coarse7"])
    o.upload(lc.hip_raw(case)[1])                # the state now has npts points, the grid was defined for other.ncol
    o.init_ocean(0)
    o.window_schedule(0, 1, 1, 1, ("T",), A.WIN_MEAN)
    o.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    o.step(1, 1)
    five = torch.zeros((7, 5), dtype=torch.float64, device="cuda")
    tab = (H * 1)(H(**{**hok, "sched": 0, "axis": 0, "grid": 0, "out": five.data_ptr()}))
    assert lib.mckpp_hip_vrecords_hv_dev(o._h, 1, tab, None) < 0
    assert err() == hname + f"planes[0]: grid 0 was defined for npts={other.ncol}, the state has {npts}: define it again", err()
    o.close()
    # a multi handle checks every plane of every shard before any shard queues
    m, kcm, k3m = resident(mk, case, shards=2)
    m.vaxis_define(0, ax["coarse7"])
    m.window_schedule(0, 1, 1, 1, ("T",), A.WIN_MEAN)
    m.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    m.step(1, 1)
    m_before = {k: v.copy() for k, v in _state(m, k3m, kcm, case.nz).items()}
    seven = torch.full((7, npts), -5.0, dtype=torch.float64, device="cuda")
    mok = dict(vok, sched=0, axis=0, out=seven.data_ptr())
    tab2 = (V * 2)(V(**mok), V(**{**mok, "out": pinned.data_ptr()}))
    assert lib.mckpp_hip_multi_vrecords_vaxis_dev(m._h, 2, tab2, None) < 0
    assert err().startswith("mckpp_hip_multi_vrecords_vaxis_dev: planes[1].out is pinned host memory"), err()
    tab2 = (V * 2)(V(**{**mok, "out": pageable.ctypes.data}), V(**{**mok, "out": pageable.ctypes.data, "rec": 1}))
    assert lib.mckpp_hip_multi_vrecords_vaxis_host(m._h, 2, tab2) < 0
    assert err().startswith("mckpp_hip_multi_vrecords_vaxis_host: planes[1]: record 1 of schedule 0 (steps 2..2) is incomplete"), err()
    assert lib.mckpp_hip_multi_vrecords_hv_dev(m._h, 1, (H * 1)(H(**{**mok, "grid": 0, "norm": 0})), None) < 0
    assert err().startswith("mckpp_hip_multi_vrecords_hv_dev: planes[0]: grid 0 is not defined"), err()
    assert_same(_state(m, k3m, kcm, case.nz), m_before, slice(None), "the shards after the refusals")
    assert (seven.cpu().numpy() == -5.0).all()
    m.close()
    # the Python layer's texts, and the library's through it
    with pytest.raises(ValueError, match="a host array"):
        h.vaxis_records_dev([(1, 0, "T", 0, AX["inside"], pinned[:nin * len(pts)].view(nin, len(pts)))])
    with pytest.raises(E, match=r"mckpp_hip_vrecords_vaxis_dev: planes\[0\]: caller level %d of axis 5 " % (nout - 1)):
        h.vaxis_records_dev([(1, 0, "T", 0, 5, out[:, :len(pts)].contiguous())])
    with pytest.raises(E, match=r"mckpp_hip_vrecords_hv_dev: planes\[0\]: record 5 of schedule 1"):
        h.hv_records_dev([(1, 5, "T", 0, g, AX["inside"], good[:nin, :n].contiguous())])
    after = everything()
    assert after[0] == before[0], "a refused call touched the schedules, the axes or the grids"
    assert all(np.array_equal(x, y) for x, y in zip(after[1], before[1])), "a refused call touched the records"
    assert after[2].keys() == before[2].keys() and all(np.array_equal(after[2][k], before[2][k]) for k in before[2]), \
        "a refused call touched the state"
    assert (out.cpu().numpy() == -5.0).all() and not good.cpu().numpy().any() and (pageable == -5.0).all()
    # ... and the run goes on: good deliveries - the one-double-per-row layout of a single kept level among them -, the
    # next launch under every schedule
    got = torch.full((nin, len(pts)), -5.0, dtype=torch.float64, device="cuda")
    h.vaxis_records_dev([(1, 0, "T", 1, AX["inside"], got)], land_value=LAND)
    sea = lc.ocean(case)[pts] != 0
    assert (got.cpu().numpy()[:, sea] != -5.0).all() and (got.cpu().numpy()[:, ~sea] == LAND).all()
    h.window_record_release(0, 1)
    h.window_record_release(1, 0)
    h.window_schedule_zoom(0, 5, 1, 1, ("T",), A.WIN_LAST, levels=(0, 1))
    h.vaxis_define(6, [kc.zm[0] + 2.0, kc.zm[0] + 1.0])          # above the column: every entry reads level 0
    h.step(5, 1)
    top = torch.full((2, npts), -5.0, dtype=torch.float64, device="cuda")
    h.vaxis_records_dev([(0, 0, "T", 3, 6, top)], land_value=LAND)
    x = np.full((npts, 1), LAND, order="F")
    h.window_record_fetch(0, 0, "T", 3, x)
    assert np.array_equal(_bits(top.cpu().numpy()), _bits(np.stack([x[:, 0], x[:, 0]])))
    with pytest.raises(E, match=r"planes\[0\]: caller level %d of axis 1 \(z=.*\) reads model level %d, and schedule 0 keeps levels "
                                r"0\.\.0" % c7top):
        h.vaxis_records_dev([(0, 0, "T", 3, AX["coarse7"], torch.zeros((7, npts), dtype=torch.float64, device="cuda"))])
    assert h.window_records(1) == (1, 0)
    h.close()
