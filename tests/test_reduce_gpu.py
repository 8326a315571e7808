"""Records of output schedules reduced over levels and points on the device (include/mckpp_hip_reduce.h:
mckpp_hip_reduce_weights, mckpp_hip_records_reduce_dev, mckpp_hip_records_reduce_host and their multi_ twins).

The checker is tests/reduce_ref.py, the header's arithmetic restated in numpy, on what mckpp_hip_window_record_fetch
gives - existing code held to the per-step API elsewhere.  Every comparison is of bit patterns.  Shapes, schedules and
records are those of tests/test_device_records_gpu.py, whose Run is used as it is; one more shape, 20 levels x 40,000
points, exists for the tree alone: 65,536 terms, which any implementation splits over workgroups or stages.  The
environment switch MCKPP_REDUCE_M=64 makes that widest path the small shapes' too."""
import numpy as np
import pytest

import common as cm
import reduce_ref as rr
from harness import mk  # noqa: F401
from test_device_records_gpu import LAND, NREC, PERIOD, PRE, SHAPES, Run, _start, _sub, _too_small

pytestmark = pytest.mark.gpu

AXIS_OPS = DOMAIN_OPS = (rr.NONE, rr.SUM, rr.AVERAGE, rr.MIN, rr.MAX)
PAIRS = [(a, d) for a in AXIS_OPS for d in DOMAIN_OPS if a or d]   # 24


def weights(kc, npts):
    """an area-like point weight - the cosine of a latitude, some of them zero - and hm as the level weight; the
    interface weight is another array, so that a mix-up shows"""
    lat = np.linspace(-np.pi / 2, np.pi / 2, npts)
    wp = np.cos(lat)
    wp[wp < 1e-3] = 0.0
    wp[5::11] = 0.0
    return wp, np.array(kc.hm, dtype=np.float64), np.array(kc.hm, dtype=np.float64)[::-1] * 0.5 + 1.0


class Red:
    """The reductions of a context against the restatement.  A plane is (sched, rec, field, op, axis_op, domain_op,
    weighted, lev0, nlev); geometry(s) -> (points of the positions, is_row of the positions, the zoom's first level)."""

    def __init__(self, h, A, k3, nzp1, geometry, axis, w):
        self.h, self.A, self.k3, self.nzp1, self.geometry, self.axis = h, A, k3, nzp1, geometry, axis
        self.wp, self.wl, self.wi = w
        self.fetched, self.seen = {}, []

    def fetch(self, s, rec, name, op):
        """window_record_fetch of the field and op, (npoints, levels kept), once per record plane"""
        key = (s, rec, name, op)
        if key not in self.fetched:
            npoints, kept = self.axis(s, name)
            out = np.full((npoints,) if self.A.OUT[name] in self.A._OUT_2D else (npoints, kept), LAND, order="F")
            self.h.window_record_fetch(s, rec, name, op, out)
            self.fetched[key] = out.reshape(npoints, -1).copy()
        return self.fetched[key]

    def want(self, p):
        s, rec, name, op, aop, dop, wbits, lev0, nlev = p
        points, is_row, zlev0 = self.geometry(s)
        x = self.fetch(s, rec, name, op)[:, lev0:lev0 + nlev]
        iface = name in ("difm",)
        wl = (self.wi if iface else self.wl)[zlev0 + lev0:zlev0 + lev0 + nlev] if wbits & rr.W_LEVELS else None
        wp = self.wp[points] if wbits & rr.W_POINTS else None
        return rr.reduce_plane(x, is_row, aop, dop, wl, wp, LAND, self.seen)

    def table(self, planes, outs):
        return [(s, rec, name, op, o, aop, dop, wbits, lev0, nlev) for (s, rec, name, op, aop, dop, wbits, lev0, nlev), o in zip(planes, outs)]

    def check(self, planes, form="dev", what=""):
        """64 planes a call, each against the restatement; an array has one element more than the result, which stays"""
        import torch

        for k0 in range(0, len(planes), 64):
            part = planes[k0:k0 + 64]
            wants = [self.want(p) for p in part]
            if form == "dev":
                full = [torch.full((w.size + 1,), PRE, dtype=torch.float64, device="cuda") for w in wants]
                self.h.records_reduce_dev(self.table(part, [f[:-1] for f in full]), land_value=LAND)
                gots = [f.cpu().numpy() for f in full]
            else:
                gots = [np.full(w.size + 1, PRE) for w in wants]
                self.h.records_reduce_host(self.table(part, [g[:-1] for g in gots]), land_value=LAND)
            for p, w, g in zip(part, wants, gots):
                assert np.array_equal(rr.bits(g[:-1]), rr.bits(w)), (what, form, p, g[:-1][:4], w[:4])
                assert g[-1] == PRE, (what, form, p, "the element behind the result was written")

    def order_shows(self):
        """at least one tree sum of the planes checked so far differs in bits from the left-to-right sum of its terms"""
        return any(rr.bits(t) != rr.bits(l) for t, l in self.seen)


def red_of(r):
    """a Red over a Run of tests/test_device_records_gpu.py, its weights set"""
    w = weights(r.kc, r.npts)
    r.h.reduce_weights(*w)

    def geometry(s):
        pts, lev = r.z.get(r.sched[s][0], (None, None))
        points = np.arange(r.npts) if pts is None else np.asarray(pts)
        return points, r.k3.run_physics[points] != 0, (lev[0] if lev else 0)

    return Red(r.h, r.A, r.k3, r.nzp1, geometry, r.axis, w)


def every_op(r, s, rec, fields):
    """the 24 pairs of reductions of each (field, op) of `fields` in record rec of schedule s: the whole kept range,
    weighted wherever a reduction takes weights and unweighted; for the first field also a sub-range from an offset"""
    out = []
    for n, (name, op) in enumerate(fields):
        kept = r.axis(s, name)[1]
        ranges = [(0, kept)]
        if n == 0 and kept > 40:
            ranges.append(_sub(kept))
        elif n == 0 and kept > 3:
            ranges.append((2, kept - 3))
        for lev0, nlev in ranges:
            for aop, dop in PAIRS:
                wbits = (rr.W_LEVELS if aop in (rr.SUM, rr.AVERAGE) and kept > 1 else 0) | (rr.W_POINTS if dop in (rr.SUM, rr.AVERAGE) else 0)
                out.append((s, rec, name, op, aop, dop, wbits, lev0, nlev))
                if wbits:
                    out.append((s, rec, name, op, aop, dop, 0, lev0, nlev))
    return out


# ---------------------------------------------------------------------------
# 1. every op against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nz,grid,ncol,land_every", SHAPES)
def test_every_reduction_is_the_restatement(mk, nz, grid, ncol, land_every):
    """The five axis ops x the five domain ops of T, S (with Sref), hmix (2-D) and difm (interface axis), ops mean and
    last, whole range and a sub-range, weighted and not, of the unzoomed schedule and the four zooms, records 1 and 2 of
    a ring of two: SST domain mean (the level-0 zoom), heat content (axis sum with hm, then the area average) and the
    mean profile (domain average per level: 61, 70, 101 levels, the last two across the 64-level tile) among them.  The
    device form into torch tensors, the host form into numpy."""
    r = Run(mk, nz, grid, ncol, land_every)
    red = red_of(r)
    red.check(every_op(r, 0, 2, [("S", 0), ("T", 3), ("hmix", 0), ("difm", 0)]), "dev", "unzoomed")
    red.check(every_op(r, 0, 1, [("T", 3), ("S", 3), ("hmix", 3), ("difm", 2)])[::3], "host", "unzoomed")
    red.check(every_op(r, 1, 1, [("T", 0), ("hmix", 3)]), "dev", "level 0")
    red.check(every_op(r, 2, 2, [("S", 0), ("difm", 0), ("T", 3)]), "dev", "a third of the points at levels 5..16")
    red.check(every_op(r, 3, 2, [("T", 0), ("S", 3)])[::2], "host", "one point")
    assert red.order_shows(), "no sum of this test tells the tree from the left-to-right sum"
    r.all_zooms()
    red.fetched.clear()
    land = every_op(r, 0, 0, [("T", 0), ("hmix", 3)])
    red.check(land, "dev", "the land points alone")
    red.check(land[::5], "host", "the land points alone")
    for p in land:   # no row: every element is the land value, and the average's 0/0 never reaches out
        assert (red.want(p) == LAND).all(), p
    r.h.close()


def test_the_halving_pass_on_a_small_shape(mk, monkeypatch):
    """MCKPP_REDUCE_M=64: a workgroup finishes 64 terms, so the 512 of the 400-point grid and the 256 of the third are
    halved in place first - the widest path, on a shape whose every other edge is covered above"""
    monkeypatch.setenv("MCKPP_REDUCE_M", "64")
    r = Run(mk, *SHAPES[0])
    red = red_of(r)
    red.check(every_op(r, 0, 2, [("S", 0), ("hmix", 1)]), "dev", "M = 64")
    red.check(every_op(r, 2, 1, [("difm", 2)]), "host", "M = 64, a third")
    # one call with planes that take the pass and planes that do not (one point: one term)
    red.check(every_op(r, 3, 2, [("T", 0)])[:24] + every_op(r, 0, 1, [("T", 3)])[:40], "dev", "M = 64, mixed")
    assert red.order_shows()
    r.h.close()


# ---------------------------------------------------------------------------
# 2. edges of the tree
# ---------------------------------------------------------------------------
def test_point_lists_at_the_edges_of_the_tree(mk):
    """point lists of 1, 2, 64, 255, 256 and 257 points, of ocean points alone and with land among them: a power of
    two, one less, one more; then weights that are zero on every row"""
    A = mk.api
    h, kc, k3 = _start(mk, *SHAPES[0])
    npts, nzp1 = SHAPES[0][2], kc.nzp1
    w = weights(kc, npts)
    h.reduce_weights(*w)
    ocean, land, rng = np.nonzero(k3.run_physics != 0)[0], np.nonzero(k3.run_physics == 0)[0], np.random.default_rng(3)
    lists = []
    for n in (1, 2, 64, 255, 256, 257):
        lists.append(rng.permutation(ocean)[:n])
        first = [land[1]] if n == 1 else [ocean[0], land[1]]   # (one point: a list without a row)
        rest = [p for p in rng.permutation(npts) if p not in first]
        lists.append(rng.permutation(np.array(first + rest[:n - len(first)])))
    fields, ops = ("T", "hmix"), A.WIN_MEAN | A.WIN_LAST
    nt, seen = 1, []
    for g0 in range(0, len(lists), 4):
        group = lists[g0:g0 + 4]
        for s, pts in enumerate(group):
            h.window_schedule_zoom(s, nt, PERIOD, 1, fields, ops, points=pts, levels=(2, 9))
        h.step(nt, PERIOD)
        nt += PERIOD

        def geometry(s):
            return group[s], k3.run_physics[group[s]] != 0, 2

        red = Red(h, A, k3, nzp1, geometry, lambda s, name: (len(group[s]), 1 if name == "hmix" else 9), w)
        planes = []
        for s in range(len(group)):
            for name, op in (("T", 0), ("hmix", 3)):
                for aop, dop in PAIRS:
                    wbits = (rr.W_LEVELS if aop in (1, 2) and name == "T" else 0) | (rr.W_POINTS if dop in (1, 2) else 0)
                    planes.append((s, 0, name, op, aop, dop, wbits, 0, 9 if name == "T" else 1))
        red.check(planes, "dev", "point lists")
        red.check(planes[::7], "host", "point lists")
        seen += red.seen
    assert any(rr.bits(t) != rr.bits(l) for t, l in seen)
    # weights that are zero on every row: the averages are the land value
    zero_p = np.where(k3.run_physics != 0, 0.0, 1.0)
    h.reduce_weights(zero_p, np.zeros(nzp1), None)
    red = Red(h, A, k3, nzp1, geometry, red.axis, (zero_p, np.zeros(nzp1), None))
    planes = [(1, 0, "T", 0, rr.NONE, rr.AVERAGE, rr.W_POINTS, 0, 9), (1, 0, "T", 0, rr.SUM, rr.AVERAGE, rr.W_POINTS, 0, 9),
              (1, 0, "T", 3, rr.AVERAGE, rr.NONE, rr.W_LEVELS, 0, 9), (1, 0, "T", 3, rr.AVERAGE, rr.MAX, rr.W_LEVELS, 2, 3),
              (1, 0, "hmix", 3, rr.MIN, rr.AVERAGE, rr.W_POINTS, 0, 1), (1, 0, "T", 0, rr.SUM, rr.SUM, 3, 0, 9)]
    red.check(planes, "dev", "zero weights")
    red.check(planes, "host", "zero weights")
    assert all((red.want(p) == LAND).all() for p in planes[:5]) and red.want(planes[5])[0] == 0.0
    h.close()


def test_the_tree_over_40000_points(mk):
    """20 levels x 40,000 points, every 7th land, 3 steps, period 3: 65,536 terms a level.  Sum, average, min and max at
    one level and over all 21, with an axis reduction in front and without."""
    A = mk.api
    nz, npts = 20, 40000
    h, kc, k3 = _start(mk, nz, "uniform", npts, 7)
    w = weights(kc, npts)
    h.reduce_weights(*w)
    h.window_schedule(0, 1, PERIOD, 1, ("T", "hmix"), A.WIN_MEAN | A.WIN_LAST)
    h.step(1, PERIOD)
    red = Red(h, A, k3, kc.nzp1, lambda s: (np.arange(npts), k3.run_physics != 0, 0),
              lambda s, name: (npts, 1 if name == "hmix" else kc.nzp1), w)
    planes = []
    for dop in (rr.SUM, rr.AVERAGE, rr.MIN, rr.MAX):
        wb = rr.W_POINTS if dop in (rr.SUM, rr.AVERAGE) else 0
        planes += [(0, 0, "T", 0, rr.NONE, dop, wb, 0, 1), (0, 0, "T", 0, rr.NONE, dop, wb, 0, kc.nzp1),
                   (0, 0, "T", 3, rr.NONE, dop, 0, 3, 5), (0, 0, "T", 0, rr.SUM, dop, wb | rr.W_LEVELS, 0, kc.nzp1),
                   (0, 0, "hmix", 3, rr.NONE, dop, wb, 0, 1)]
    planes.append((0, 0, "T", 0, rr.AVERAGE, rr.NONE, rr.W_LEVELS, 0, kc.nzp1))
    red.check(planes, "dev", "40,000 points")
    red.check(planes[1::5], "host", "40,000 points")
    assert red.order_shows()
    h.close()


# ---------------------------------------------------------------------------
# 3. ordering
# ---------------------------------------------------------------------------
def test_a_scalar_for_a_consumer_on_a_side_stream(mk):
    """The consumer multiplies the scalar on a side stream with no host synchronisation between; the arrays are
    rewritten on that stream before the call, which the delivery must follow."""
    import torch

    r = Run(mk, *SHAPES[0])
    red = red_of(r)
    planes = [(1, 2, "T", 0, rr.NONE, rr.AVERAGE, rr.W_POINTS, 0, 1), (0, 2, "S", 0, rr.SUM, rr.AVERAGE, 3, 0, r.nzp1),
              (0, 1, "T", 3, rr.NONE, rr.AVERAGE, 0, 0, r.nzp1), (2, 1, "difm", 2, rr.MAX, rr.NONE, 0, 0, 12)]
    wants = [red.want(p) for p in planes]
    outs = [torch.zeros(w.size, dtype=torch.float64, device="cuda") for w in wants]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for o in outs:
            o.fill_(-1.0)
        r.h.records_reduce_dev(red.table(planes, outs), land_value=LAND)
        twice = [torch.mul(o, 2.0) for o in outs]
    side.synchronize()
    for p, t, w in zip(planes, twice, wants):
        assert np.array_equal(rr.bits(t.cpu().numpy()), rr.bits(w * 2.0)), p
    r.h.close()


def test_release_and_overwrite_behind_the_reduction(mk):
    """A ring of one record: record w is reduced and released, and the steps that write record w + 1 into its one slot
    are launched at once, with no synchronisation in the loop.  The results are record w's: what the restatement makes
    of a second context's synchronous fetches.  A race test can only fail, never prove."""
    import torch

    ncol = SHAPES[0][2]
    A = mk.api
    names, ops, nwin = ("T", "hmix"), A.WIN_MEAN | A.WIN_LAST, 5
    h, kc, k3 = _start(mk, *SHAPES[0])
    ref, _, _ = _start(mk, *SHAPES[0])
    w = weights(kc, ncol)
    for x in (h, ref):
        x.window_schedule(0, 1, PERIOD, 1, names, ops)
        x.reduce_weights(*w)
    red = Red(ref, A, k3, kc.nzp1, lambda s: (np.arange(ncol), k3.run_physics != 0, 0),
              lambda s, name: (ncol, 1 if name == "hmix" else kc.nzp1), w)
    what = [("T", 0, rr.NONE, rr.AVERAGE, 2, 0, 1), ("T", 0, rr.SUM, rr.AVERAGE, 3, 0, kc.nzp1), ("T", 3, rr.NONE, rr.AVERAGE, 0, 0, kc.nzp1),
            ("hmix", 3, rr.NONE, rr.MAX, 0, 0, 1), ("T", 0, rr.AVERAGE, rr.NONE, 1, 0, kc.nzp1)]
    sizes = [1, 1, kc.nzp1, 1, ncol]
    outs = [[torch.full((n,), PRE, dtype=torch.float64, device="cuda") for n in sizes] for _ in range(nwin)]
    torch.cuda.synchronize()
    for k in range(nwin):
        h.step(k * PERIOD + 1, PERIOD)
        h.records_reduce_dev([(0, k, name, op, o, aop, dop, wb, lev0, nlev) for (name, op, aop, dop, wb, lev0, nlev), o in zip(what, outs[k])],
                             land_value=LAND)
        h.window_record_release(0, k)
    h.step(nwin * PERIOD + 1, PERIOD)   # ... and the last record's slot is overwritten too
    for k in range(nwin):
        ref.step(k * PERIOD + 1, PERIOD)
        for (name, op, aop, dop, wb, lev0, nlev), o in zip(what, outs[k]):
            want = red.want((0, k, name, op, aop, dop, wb, lev0, nlev))
            assert np.array_equal(rr.bits(o.cpu().numpy()), rr.bits(want)), ("record", k, name, aop, dop)
        ref.window_record_release(0, k)
    h.close()
    ref.close()


# ---------------------------------------------------------------------------
# 4. refusals, before anything is queued
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.MckppHipError
    r = Run(mk, *SHAPES[0])
    h, npts, nzp1 = r.h, r.npts, r.nzp1
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()
    P = A._ReducePlaneC
    # the weights' own refusals, first without any set
    wp, wl, wi = weights(r.kc, npts)
    out = torch.full((npts,), PRE, dtype=torch.float64, device="cuda")
    ok = dict(sched=0, field=A.OUT["S"], op=0, lev0=0, nlev=nzp1, axis_op=1, domain_op=0, weighted=0, rec=2, land_value=LAND,
              out=out.data_ptr())

    def refused(text, k=0, fn="mckpp_hip_records_reduce_dev", **swap):
        tab = (P * (k + 1))(*([P(**ok)] * k + [P(**{**ok, **swap})]))
        args = (h._h, k + 1, tab, None) if fn.endswith("_dev") else (h._h, k + 1, tab)
        assert getattr(lib, fn)(*args) == -1, text
        assert err().startswith(fn + ": ") and f"planes[{k}]" in err() and text in err(), err()

    refused("weighted bit 0 (level weights), but no level_w is set (mckpp_hip_reduce_weights", weighted=1)
    refused("weighted bit 1 (point weights), but no point_w is set", axis_op=0, domain_op=2, weighted=2)
    for bad, text in ((dict(point_w=np.where(np.arange(npts) == 7, -1.0, wp)), "point_w[7] = -1: every weight must be finite and >= 0"),
                      (dict(point_w=wp, level_w=np.where(np.arange(nzp1) == 3, np.nan, wl)), "level_w[3] = nan"),
                      (dict(iface_w=np.where(np.arange(nzp1) == nzp1 - 1, np.inf, wi)), f"iface_w[{nzp1 - 1}] = inf")):
        with pytest.raises(E, match=r"mckpp_hip_reduce_weights: " + text.replace("[", r"\[").replace("]", r"\]")):
            h.reduce_weights(**bad)
    refused("no level_w is set", weighted=1)   # a refused call set nothing
    h.reduce_weights(wp, wl, None)
    refused("no iface_w is set (mckpp_hip_reduce_weights; field 13 is on the interface axis)", field=A.OUT["difm"], weighted=1)
    h.reduce_weights(wp, wl, wi)
    with pytest.raises(E, match=r"mckpp_hip_reduce_weights: level_w\[0\] = -"):
        h.reduce_weights(wp, -2.0 * wl, wi)
    red = red_of(r)
    good_planes = [(0, 2, "S", 0, rr.SUM, rr.AVERAGE, 3, 0, nzp1), (2, 1, "T", 3, rr.NONE, rr.SUM, 2, 0, 12),
                   (0, 1, "difm", 2, rr.AVERAGE, rr.NONE, 1, 0, nzp1)]
    rec_planes = [(0, 2, "S", 0, 0, nzp1), (2, 1, "T", 3, 0, 12)]

    def state():
        return [h.window_records(s) for s in range(4)], [rr.bits(r.want(p, LAND)).copy() for p in rec_planes]

    before = state()
    pinned = torch.zeros(npts, dtype=torch.float64).pin_memory()
    pageable = np.zeros(npts)
    big, small, holds = _too_small(torch, npts * 8)

    # the inherited refusals, with the new prefix
    refused("schedule 7 (0..3)", sched=7)
    refused("record 3 of schedule 0 (steps 10..12) is incomplete: steps have run up to 9", k=1, rec=3)
    refused("record 0 of schedule 0 (steps 1..3) has been released", rec=0)
    refused("record -1", rec=-1)
    refused("field 0 is not in schedule 0", field=A.OUT["u"])
    refused("schedule 0 keeps no op 0 of field 2", field=A.OUT["T"])
    refused("op 4 (0 mean, 1 min, 2 max, 3 last)", op=4)
    refused("lev0=30 nlev=40 is no range of the levels schedule 0 keeps of field 5, which are 61", lev0=30, nlev=40)
    refused("lev0=0 nlev=0 is no range", k=2, nlev=0)
    refused("lev0=0 nlev=13 is no range of the levels schedule 2 keeps of field 5, which are 12", sched=2, nlev=13)
    refused("record 3 of schedule 0 (steps 10..12) is incomplete", fn="mckpp_hip_records_reduce_host", rec=3)
    # the new ones
    refused("axis_op and domain_op are both 0 (none): a plane that is not reduced is mckpp_hip_records_dev's", axis_op=0)
    refused("axis_op 5 (0 none, 1 sum, 2 average, 3 min, 4 max)", axis_op=5)
    refused("axis_op -1", axis_op=-1)
    refused("domain_op 7 (0 none", k=1, domain_op=7)
    refused("weighted 0x4 (bit 0: level weights, bit 1: point weights)", weighted=4)
    refused("weighted bit 0 (level weights) with axis_op 3, a reduction that takes no weights", axis_op=3, weighted=1)
    refused("weighted bit 0 (level weights) with axis_op 0", axis_op=0, domain_op=1, weighted=1)
    refused("weighted bit 1 (point weights) with domain_op 0", weighted=2)
    refused("weighted bit 1 (point weights) with domain_op 4", domain_op=4, weighted=2)
    refused("weighted bit 0 (level weights), but field 4 is two-dimensional", field=A.OUT["hmix"], nlev=1, weighted=1)
    refused("planes[0].out is pinned host memory", out=pinned.data_ptr())
    refused("planes[1].out is host memory", k=1, out=pageable.ctypes.data)
    refused("planes[0].out is null", out=None)
    refused("planes[0].out is null", fn="mckpp_hip_records_reduce_host", out=None)
    refused(f"planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {npts * 8}", out=small.data_ptr())
    for fn in ("mckpp_hip_records_reduce_dev", "mckpp_hip_records_reduce_host"):
        tab = (P * 65)(*[P(**ok)] * 65)
        tail = (None,) if fn.endswith("_dev") else ()
        assert getattr(lib, fn)(h._h, 65, tab, *tail) == -1 and fn + ": nplanes=65 (0..64)" in err()
        assert getattr(lib, fn)(h._h, 1, None, *tail) == -1 and fn + ": nplanes=1 (0..64) or a null table" in err()
        assert getattr(lib, fn)(h._h, 0, None, *tail) == 0   # (no plane: nothing to do)
    with pytest.raises(E, match=r"mckpp_hip_records_reduce_dev: planes\[1\]: record 3 of schedule 0 \(steps 10\.\.12\) is incomplete"):
        h.records_reduce_dev([(0, 2, "S", 0, out, "sum", "none"), (0, 3, "S", 0, out, "sum", "none")])
    torch.cuda.synchronize()
    assert bool((out == PRE).all()) and bool((big == 0).all()), "a refused reduction wrote"
    after = state()
    assert after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))
    r.check([(0, 2, "S", 0, 0, nzp1)], what="a records_dev plane after the refusals")
    red.check(good_planes, "dev", "after the refusals")   # the weights are the ones set last, and a good call follows
    red.check(good_planes, "host", "after the refusals")
    h.close()


# ---------------------------------------------------------------------------
# 5. both handles: two shards on the one device
# ---------------------------------------------------------------------------
def test_two_shards_reduce_to_the_single_contexts_bits(mk):
    """Every kind of plane under a multi handle of two shards is the single context's bit for bit - and the
    restatement's -, and the domain sum of axis-reduced terms equals host_reduce_tree of the gathered terms: what a run
    with one process per GPU computes after its gather."""
    import torch

    one, two = Run(mk, *SHAPES[1]), Run(mk, *SHAPES[1], shards=2)
    ra, rb = red_of(one), red_of(two)
    nzp1 = one.nzp1
    planes = []
    for aop, dop in PAIRS:
        wb = (1 if aop in (1, 2) else 0) | (2 if dop in (1, 2) else 0)
        planes += [(0, 2, "S", 0, aop, dop, wb, 0, nzp1), (2, 1, "difm", 2, aop, dop, wb, 1, 9), (1, 1, "hmix", 3, aop, dop, wb & 2, 0, 1),
                   (3, 2, "T", 0, aop, dop, 0, 0, nzp1)]
    for form in ("dev", "host"):
        ra.check(planes if form == "dev" else planes[::3], form, "one context")
        rb.check(planes if form == "dev" else planes[::3], form, "two shards")
    # the gathered terms: the axis-reduced plane, weighted by point on the host, through the host tree
    wp = ra.wp
    for s, rec, name, op, lev0, nlev, pts in ((0, 2, "S", 0, 0, nzp1, None), (2, 1, "T", 3, 2, 7, one.z["third"][0])):
        n = one.npts if pts is None else len(pts)
        terms, total = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        two.h.records_reduce_dev([(s, rec, name, op, terms, "sum", "none", 1, lev0, nlev), (s, rec, name, op, total, "sum", "sum", 3, lev0, nlev)],
                                 land_value=0.0)
        t = terms.cpu().numpy()
        points = np.arange(n) if pts is None else pts
        is_row = one.k3.run_physics[points] != 0
        gathered = np.where(is_row, wp[points] * t, 0.0)
        assert rr.bits(mk.api.host_reduce_tree(gathered)) == rr.bits(total.cpu().numpy()[0]), (s, name)
    for r in (one, two):
        r.all_zooms()
    for red in (ra, rb):
        red.fetched.clear()
    planes = [(0, 0, "T", 0, aop, dop, 0, 0, nzp1) for aop, dop in PAIRS] + [(2, 3, "S", 3, rr.AVERAGE, rr.AVERAGE, 3, 2, 9)]
    ra.check(planes, "dev", "one context, the land list")
    rb.check(planes, "dev", "two shards, the land list")
    rb.check(planes[::4], "host", "two shards, the land list")
    one.h.close()
    two.h.close()


# ---------------------------------------------------------------------------
# 6. the weights are the context's, not the resident state's
# ---------------------------------------------------------------------------
def test_weights_survive_upload(mk):
    """After an upload with another column map and a new schedule, a weighted reduction uses the weights set before
    it and matches the restatement."""
    A = mk.api
    nz, grid, ncol, land_every = SHAPES[0]
    h, kc, k3 = _start(mk, nz, grid, ncol, land_every)
    w = weights(kc, ncol)
    h.reduce_weights(*w)
    _, k3b = cm.make_hip_case(ncol, nz, grid=grid, land_every=5)   # other points are land now
    assert (k3b.run_physics != k3.run_physics).any()
    h.upload(k3b)
    h.init_ocean(0)
    cm.set_forcing_3d(k3b, cm.synth.forcing(ncol, "bench"))
    h.set_forcing(k3b.sflux)
    pts = np.random.default_rng(5).permutation(ncol)[:130]
    h.window_schedule(0, 1, PERIOD, NREC, ("T", "difm"), A.WIN_MEAN | A.WIN_LAST)
    h.window_schedule_zoom(1, 1, PERIOD, NREC, ("T",), A.WIN_MEAN, points=pts, levels=(0, 1))
    h.step(1, PERIOD)

    def geometry(s):
        points = np.arange(ncol) if s == 0 else pts
        return points, k3b.run_physics[points] != 0, 0

    red = Red(h, A, k3b, kc.nzp1, geometry, lambda s, name: (ncol, kc.nzp1) if s == 0 else (len(pts), 1), w)
    planes = [(0, 0, "T", 0, rr.SUM, rr.AVERAGE, 3, 0, kc.nzp1), (0, 0, "difm", 3, rr.AVERAGE, rr.SUM, 3, 0, kc.nzp1),
              (0, 0, "T", 3, rr.NONE, rr.AVERAGE, 2, 0, kc.nzp1), (1, 0, "T", 0, rr.NONE, rr.AVERAGE, 2, 0, 1),
              (0, 0, "T", 0, rr.AVERAGE, rr.NONE, 1, 4, 30)]
    red.check(planes, "dev", "after an upload")
    red.check(planes, "host", "after an upload")
    h.close()
