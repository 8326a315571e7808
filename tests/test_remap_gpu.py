"""Records out and state in on the caller's horizontal grids (include/mckpp_hip_remap.h: mckpp_hip_remap_records_dev,
mckpp_hip_remap_put_dev and their multi_ twins; k_record_planes into the staging and k_hgrid_out, k_remap_put_planes).

Every value comparison is an equality of bits; no test has a tolerance and none skips a case.  The yardsticks are the
existing calls and tests/hgrid_ref.py's numpy restatement of include/mckpp_hip_hgrid.h:
  records out  hgrid_ref.apply(out table, x, n, used = the points that are rows of the record, norm, fill) with x
               mckpp_hip_window_record_fetch of the same schedule, record, field and op, scattered to point numbers;
  state in     on a second context the existing mckpp_hip_put_dev of the plane hgrid_ref.apply(in table, level, npts)
               remapped on the host, with MCKPP_PUT_SKIP on a sentinel at every element the rule leaves alone - an
               empty row, or a skip value read by an entry; and tests/golden/ref_loop.npz where a put changes nothing.
The cases are those of tests/test_put_gpu.py and tests/test_hgrid_gpu.py: every_step_nz40 (40 points, 30 columns: one
partial 64-column tile, land in the map, 41 levels), sweep_nd3 (2000 points with land: more than 256 columns, tails in
the 64- and the 256-column paths) and deep_nz100_nd4 (101 levels: two level tiles, the second one's 16-level groups
partly past the axis).  Grids and tables are hgrid_ref's: rows of 0, 1, 4, 9 and 70 entries, negative weights, repeated
indices.  Inputs hold no NaN."""
import dataclasses

import numpy as np
import pytest

import hgrid_ref as hr
import ref_loop_cases as lc
from harness import assert_same, flux_args, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401
from test_device_arrays_gpu import FILL_BYTES, FILLS, _assert_golden, _bits, _dev, _intervals, _ring_run, _state
from test_put_gpu import AMPLITUDE, STATE, WRITTEN, _book, _case, _written
from test_vaxis_gpu import _short_of
from test_window_schedule_gpu import _schedule

pytestmark = pytest.mark.gpu

CASES = ("every_step_nz40", "sweep_nd3", "deep_nz100_nd4")
LAND = hr.LAND
SENTINEL = -7.5e300           # what put_dev skips on the yardstick's side: no sum comes near it
PERIOD, NREC = 3, 2           # a mean's division by 3 is inexact; two ring slots
FIELDS = ("T", "S", "hmix")   # S adds Sref; hmix is 2-D
ZLEV = (2, 7)                 # the listed schedule keeps levels 2 .. 8
EMPTIED = (3, 17)             # the resident columns (by rank) whose in rows the tests empty


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def _in_table(case, n, seed):
    """hgrid_ref.general_in with the rows of two resident columns emptied: a partner that does not cover them"""
    ptr, idx, w = hr.general_in(case.ncol, n, lc.ocean(case), seed)
    rows = [[(int(i), float(v)) for i, v in zip(idx[ptr[p]:ptr[p + 1]], w[ptr[p]:ptr[p + 1]])] for p in range(case.ncol)]
    for k in EMPTIED:
        rows[int(lc.active_columns(case)[k])] = []
    return hr.csr(rows)


def _out_table(case, n, seed):
    """hgrid_ref.general_out; for a case without land rows of every length of LENGTHS in turn"""
    ocean = lc.ocean(case)
    if (ocean == 0).any():
        return hr.general_out(n, case.ncol, ocean, seed)
    rng = np.random.default_rng(seed)
    return hr.csr([hr._row(rng, hr.LENGTHS[(j + 1) % len(hr.LENGTHS)] if j != 1 else 70, case.ncol) for j in range(n)])


def _tables(case):
    """per grid (n, in table, out table)"""
    return [(n, _in_table(case, n, 7 + g), _out_table(case, n, 17 + g)) for g, n in enumerate(hr.grids(case.ncol))]


def _define(h, case):
    tabs = _tables(case)
    for g, (n, tin, tout) in enumerate(tabs):
        h.hgrid_define(g, n, tin, tout)
    return tabs


def _listed(case):
    """the point list of the listed schedule: fewer than 64 points, land among them, not ascending; the points the rows
    3, 4 and 5 of hgrid_ref.general_out read are in it"""
    ocean = lc.ocean(case)
    sea, land = np.nonzero(ocean)[0], np.nonzero(ocean == 0)[0]
    head = [sea[2], sea[0], sea[3], sea[1]] + ([land[0], land[-1]] if land.size else [])
    rest = [p for p in np.random.default_rng(case.ncol).permutation(case.ncol) if p not in head]
    return np.array(head + rest[:min(42, case.ncol // 2 - len(head))], dtype=np.int32)


def test_the_cases_and_tables_reach_the_paths_of_the_kernels():
    ncol = {t: len(lc.active_columns(lc.CASES[t])) for t in CASES}
    assert ncol["every_step_nz40"] == 30 and lc.CASES["every_step_nz40"].ncol == 40 and lc.CASES["every_step_nz40"].nz + 1 == 41
    assert ncol["sweep_nd3"] > 256 and ncol["sweep_nd3"] % 256 and ncol["sweep_nd3"] % 64 and ncol["sweep_nd3"] < 2000
    nzp1 = lc.CASES["deep_nz100_nd4"].nz + 1
    assert nzp1 == 101 and 64 < nzp1 <= 128 and (nzp1 - 64) % 16     # two level tiles; a 16-level group partly past the axis
    for tag in CASES:
        case = lc.CASES[tag]
        ocean, active = lc.ocean(case), lc.active_columns(case)
        for n, tin, tout in _tables(case):
            lin, lout = np.diff(tin[0]), np.diff(tout[0])
            empty = np.nonzero((lin == 0) & (ocean != 0))[0]
            assert list(empty) == [active[k] for k in EMPTIED], "exactly the emptied rows of resident columns are empty"
            assert lin[active[1 if ocean[1] else 0]] >= 1 and lin.max() == 70 and lout.max() == 70
            assert {1, 4, 70} <= set(lin[active]) and (tin[2] < 0).any() and (tout[2] < 0).any()
            assert any(len(set(tin[1][tin[0][r]:tin[0][r + 1]])) < lin[r] for r in range(case.ncol))   # repeated indices
            if case.ncol > 64:
                assert set(lin[active]) | {0} == set(hr.LENGTHS) and set(lout) == set(hr.LENGTHS)
        pts = _listed(case)
        assert len(pts) < 64 and len(set(pts)) == len(pts) and (np.diff(pts) < 0).any() and (ocean[pts] != 0).sum() >= 4
        if (ocean == 0).any():
            assert (ocean[pts] == 0).any()
            # a caller point whose entries are all resident but unlisted exists in the big grid's out table
            tout, inlist = _tables(case)[1][2], np.isin(np.arange(case.ncol), pts)
            if case.ncol > 64:
                assert any(lo < hi and ocean[tout[1][lo:hi]].all() and not inlist[tout[1][lo:hi]].any()
                           for lo, hi in zip(tout[0][:-1], tout[0][1:]))


# ---------------------------------------------------------------------------
# 1. records out
# ---------------------------------------------------------------------------
class Recorded:
    """A context of a case (shards > 0: a multi handle) with the two grids defined, schedule 0 unlisted and schedule 1
    with the point list of _listed at levels ZLEV, every op of FIELDS, period 3 in a ring of two; two records complete."""

    def __init__(self, mk, tag, shards=0):
        A = self.A = mk.api
        self.case = case = lc.CASES[tag]
        self.h, self.kc, self.k3 = resident(mk, case, shards)
        self.npts, self.nzp1, self.ocean = case.ncol, case.nz + 1, lc.ocean(case)
        self.tabs = _define(self.h, case)
        self.pts = _listed(case)
        every = A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX | A.WIN_LAST
        self.h.window_schedule(0, 1, PERIOD, NREC, FIELDS, every)
        self.h.window_schedule_zoom(1, 1, PERIOD, NREC, FIELDS, every, points=self.pts, levels=ZLEV)
        self.h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
        self.h.step(1, NREC * PERIOD)
        assert self.h.window_records(0) == (0, NREC - 1) == self.h.window_records(1)

    def kept(self, s, name):
        return 1 if self.A.OUT[name] in self.A._OUT_2D else (ZLEV[1] if s else self.nzp1)

    def used(self, s):
        """per point: is it a row of schedule s's records"""
        if s == 0:
            return self.ocean
        u = np.zeros(self.npts, dtype=np.int32)
        u[self.pts] = self.ocean[self.pts]
        return u

    def source(self, s, rec, name, op):
        """(levels kept, npts): window_record_fetch scattered to point numbers; 5e33 where the record has no row"""
        two_d = self.A.OUT[name] in self.A._OUT_2D
        npoints = len(self.pts) if s else self.npts
        out = np.full((npoints,) if two_d else (npoints, self.kept(s, name)), 5e33, order="F")
        self.h.window_record_fetch(s, rec, name, op, out)
        out = out.reshape(npoints, -1).T
        if s == 0:
            return np.ascontiguousarray(out)
        x = np.full((out.shape[0], self.npts), 5e33)
        x[:, self.pts] = out
        return x

    def planes(self):
        """(sched, rec, field, op, grid, lev0, nlev): mean, min, max and last; a 3-D field over its kept axis and over
        a sub-range, SST, a 2-D field; two schedules and two grids"""
        n1 = self.nzp1
        sub = (30, min(40, n1 - 30))     # crosses the 64-level tile where the axis has more
        return [(0, 1, "T", 0, 0, 0, n1), (0, 0, "S", 1, 1, *sub), (0, 1, "S", 2, 0, n1 - 1, 1), (0, 0, "T", 3, 1, 0, 1),
                (0, 1, "hmix", 0, 1, 0, 1), (0, 0, "hmix", 2, 0, 0, 1), (1, 1, "T", 0, 1, 0, ZLEV[1]), (1, 0, "S", 3, 0, 2, 4),
                (1, 1, "hmix", 1, 1, 0, 1), (1, 0, "T", 2, 0, ZLEV[1] - 1, 1), (1, 1, "S", 0, 1, 0, 1)]

    def check(self, h, dtype, norm, fill, what, planes=None):
        """one call of h - this context, or another that holds the same records - for all planes, each against the
        restatement applied to this context's records"""
        calls, outs, wants = [], [], []
        for k, (s, rec, name, op, g, lev0, nlev) in enumerate(planes or self.planes()):
            n, _, tout = self.tabs[g]
            held = np.random.default_rng(100 + k).uniform(-3.0, 3.0, (nlev, n)).astype(dtype)
            o = _dev(held)
            x = self.source(s, rec, name, op)[lev0:lev0 + nlev]
            want = np.stack([hr.apply(tout, x[j], n, self.used(s), norm, fill, LAND, held[j].astype(np.float64)) for j in range(nlev)])
            calls.append((s, rec, name, op, g, o, lev0, nlev))
            outs.append(o)
            wants.append(want.astype(dtype))
        h.remap_records_dev(calls, norm=norm, land_value=LAND, fill_land=fill)
        for c, o, want in zip(calls, outs, wants):
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), (what, c[:5], c[6:], np.dtype(dtype).name, norm, fill)
            assert not (want == dtype(5e33)).any() and np.isfinite(want).all(), "a position that is no row was read"
        return wants


@pytest.fixture(scope="module")
def recorded(mk):
    made = {}

    def get(tag, shards=0):
        if (tag, shards) not in made:
            made[tag, shards] = Recorded(mk, tag, shards)
        return made[tag, shards]

    yield get
    for r in made.values():
        r.h.close()


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("norm", hr.NORMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_records_out_are_the_restatement_of_window_record_fetch(mk, recorded, tag, dtype, norm, fill):
    r = recorded(tag)
    wants = r.check(r.h, dtype, norm, fill, tag)
    if (r.ocean == 0).any() and fill:     # what general_out's rows are built for shows: row 0 empty, row 2 land only
        sst = wants[3][0]
        assert sst[0] == dtype(LAND) and sst[2] == dtype(LAND) and sst[3] != dtype(LAND)
        assert (sst[4] == dtype(LAND)) == (norm == "used")


@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_a_listed_schedule_remaps_from_its_rows_and_from_nothing_else(mk, recorded, tag):
    """Grid 2: caller point 0 reads listed resident points, point 1 resident points that are not in the list, point 2
    both.  From the unlisted schedule all three have values; from the listed one point 1 gets the land value and
    point 2 the sum over its listed entries alone."""
    import torch

    r = recorded(tag)
    listed = r.pts[r.ocean[r.pts] != 0]
    others = np.setdiff1d(np.nonzero(r.ocean)[0], r.pts)
    rows = [[(int(listed[0]), 0.5), (int(listed[1]), 0.25)], [(int(others[0]), 0.5), (int(others[1]), 0.5)],
            [(int(others[2]), 0.5), (int(listed[2]), 0.75), (int(others[0]), -0.25)]]
    tout = hr.csr(rows)
    r.h.hgrid_define(2, 3, None, tout)
    a, b = (torch.zeros((1, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    r.h.remap_records_dev([(0, 1, "T", 0, 2, a, 0, 1), (1, 1, "T", 0, 2, b, 0, 1)], norm="none", land_value=LAND)
    a, b = a.cpu().numpy()[0], b.cpu().numpy()[0]
    whole, zoom = r.source(0, 1, "T", 0)[0], r.source(1, 1, "T", 0)[0]
    assert np.array_equal(_bits(a), _bits(hr.apply(tout, whole, 3, r.used(0), "none")))
    assert np.array_equal(_bits(b), _bits(hr.apply(tout, zoom, 3, r.used(1), "none")))
    assert LAND not in a and b[1] == LAND and b[0] != LAND
    assert b[2] == 0.75 * zoom[listed[2]] and b[2] != a[2]
    r.h.hgrid_define(2, 0)


def test_a_ring_of_one_record_is_released_and_overwritten_behind_the_delivery(mk):
    """A one-level zoom with nrec = 1: step, remap_records_dev, release at once, the next steps at once, with no
    synchronisation anywhere in the loop; compared afterwards with a second context that fetches before it releases.
    A race test can only fail, never prove."""
    import torch

    A = mk.api
    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    ref, _, _ = resident(mk, case)
    tabs = _define(h, case)
    what, nwin = [("T", 0, 1), ("T", 3, 0), ("hmix", 0, 1)], 4
    for x in (h, ref):
        x.window_schedule_zoom(0, 1, PERIOD, 1, ("T", "hmix"), A.WIN_MEAN | A.WIN_LAST, levels=(0, 1))
        x.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    outs = [[torch.full((1, tabs[g][0]), -7.0, dtype=torch.float64, device="cuda") for _, _, g in what] for _ in range(nwin)]
    torch.cuda.synchronize()
    for w in range(nwin):
        h.step(w * PERIOD + 1, PERIOD)
        h.remap_records_dev([(0, w, name, op, g, o, 0, 1) for (name, op, g), o in zip(what, outs[w])], norm="used", land_value=LAND)
        h.window_record_release(0, w)
    for w in range(nwin):
        ref.step(w * PERIOD + 1, PERIOD)
        for (name, op, g), o in zip(what, outs[w]):
            x = np.full((case.ncol,) if name == "hmix" else (case.ncol, 1), 5e33, order="F")
            ref.window_record_fetch(0, w, name, op, x)
            want = hr.apply(tabs[g][2], x.ravel(), tabs[g][0], lc.ocean(case), "used", True, LAND)
            assert np.array_equal(_bits(o.cpu().numpy()[0]), _bits(want)), ("record", w, name, op)
        ref.window_record_release(0, w)
    h.close()
    ref.close()


@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_two_shards_deliver_the_single_contexts_records(mk, recorded, tag):
    """a multi handle of two shards against the restatement applied to the single context's records, for the listed
    and the unlisted schedule: the used entries are the rows of any shard"""
    r, m = recorded(tag), recorded(tag, 2)
    mask0, n0 = mk.api.host_shard_mask(m.k3.run_physics, 2, 0)
    assert 0 < n0 < len(lc.active_columns(r.case)), "both shards hold columns"
    for dtype, norm, fill in ((np.float64, "used", True), (np.float32, "none", False)):
        r.check(m.h, dtype, norm, fill, f"{tag}, two shards")
    # ... and a shard's tables follow who addresses it: the single context again, unchanged
    r.check(r.h, np.float64, "used", True, f"{tag}, the single context afterwards")


# ---------------------------------------------------------------------------
# 2. state in
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class Spec:
    """One put: planes (field, lev0, nlev, grid), the keywords, the caller array's element type, after which intervals"""
    tag: str
    planes: tuple
    op: str = "add"
    dtype: type = np.float64
    time_levels: bool = False
    skip: float = None
    ssref: int = 1
    at: tuple = (0, 1)

    def arrays(self, tabs, r):
        """(field, grid, array (nlev, n), lev0) on the caller grids: amplitude * sin(point + level / 10 + r), around a
        value of the field's size where the operation is a set; with a skip value, every fifth caller point holds it"""
        out = []
        for name, lev0, nlev, g in self.planes:
            n = tabs[g][0]
            pt, lev = np.arange(n)[None, :], np.arange(lev0, lev0 + nlev)[:, None]
            v = AMPLITUDE[name] * np.sin(pt + lev / 10.0 + r + 0.5)
            if self.op == "set":
                v = v * 100.0 + {"T": 12.0, "S": 35.0}.get(name, 0.0)
            v = np.ascontiguousarray(v.astype(self.dtype))
            if self.skip is not None:
                assert float(self.dtype(self.skip)) == self.skip and not (v == self.skip).any()
                v[:, 1::5] = self.skip
            out.append((name, g, v, lev0))
        return out

    def kw(self):
        return dict(op=self.op, time_levels=self.time_levels, skip=self.skip)


def _on_model_points(spec, tabs, arrays, npts):
    """(field, plane (nlev, npts), lev0): the arrays through the in tables by the restatement, SENTINEL where the header
    leaves the element alone - the row is empty, or an entry reads the skip value at that level"""
    out, left = [], 0
    for name, g, v, lev0 in arrays:
        ptr, idx, w = tabs[g][1]
        v64 = v.astype(np.float64)      # widened exactly before anything else
        plane = np.stack([hr.apply((ptr, idx, w), v64[j], npts) for j in range(v64.shape[0])])
        alone = np.broadcast_to(np.diff(ptr) == 0, plane.shape).copy()
        if spec.skip is not None:
            ones = (ptr, idx, np.ones_like(w))
            alone |= np.stack([hr.apply(ones, (v64[j] == spec.skip).astype(np.float64), npts) for j in range(v64.shape[0])]) > 0
        assert not (plane == SENTINEL).any()
        left += int(alone.sum())
        out.append((name, np.where(alone, SENTINEL, plane), lev0))
    return out, left


SPECS = {
    # one partial tile: ADD f64 over the whole axis and a one-level plane at level 0, no flag
    "add_f64_whole_axis": Spec("every_step_nz40", (("T", 0, 41, 1), ("u", 0, 41, 0), ("S_anom", 0, 1, 1)), at=(0, 4)),
    # SET f32 on S (minus Sref; L_SSref = 0: Ssurf restated), both time levels, a range from lev0 > 0, SST alone
    "set_f32_S_time_levels": Spec("every_step_nz40", (("S", 0, 41, 0), ("v", 3, 20, 1), ("T", 0, 1, 1)), op="set", dtype=np.float32,
                                  time_levels=True, ssref=0, at=(1, 5)),
    "add_S_skip_ssref0": Spec("every_step_nz40", (("S", 0, 41, 1), ("v", 0, 1, 0)), skip=-999.0, ssref=0, at=(0, 3)),
    # more than 256 columns: the tails of the 64- and the 256-column paths
    "add_f32_skip_time_levels": Spec("sweep_nd3", (("v", 3, 20, 1), ("T", 0, 1, 0), ("S_anom", 40, 1, 1), ("u", 0, 41, 1)),
                                     dtype=np.float32, time_levels=True, skip=-999.0, at=(0, 3)),
    "set_f64_skip_land": Spec("sweep_nd3", (("T", 0, 1, 1), ("S", 0, 41, 1), ("u", 5, 1, 0)), op="set", skip=LAND, at=(1, 2)),
    "set_f64_S_anom": Spec("sweep_nd3", (("S_anom", 0, 41, 0), ("T", 0, 41, 1)), op="set", at=(0,)),
    # two level tiles: the whole axis, a deep sub-range that starts in the first tile and ends in the second
    "deep_add_skip_time_levels": Spec("deep_nz100_nd4", (("T", 0, 101, 1), ("S_anom", 60, 41, 0), ("v", 10, 80, 1)), skip=-999.0,
                                      time_levels=True, at=(0, 1)),
    "deep_set_f32": Spec("deep_nz100_nd4", (("T", 0, 101, 0), ("S", 0, 101, 1), ("u", 37, 64, 1), ("v", 0, 1, 1)), op="set",
                         dtype=np.float32, ssref=0, at=(0, 1)),
}


def test_the_specs_cover_what_the_kernel_can_be_asked():
    s = SPECS.values()
    assert {x.op for x in s} == {"set", "add"} and {x.dtype for x in s} == {np.float64, np.float32}
    assert {x.time_levels for x in s} == {True, False} and {x.skip is None for x in s} == {True, False}
    assert {x.ssref for x in s} == {0, 1} and {x.tag for x in s} == set(CASES)
    planes = [(x, p) for x in s for p in x.planes]
    assert any(p[1] == 0 and p[2] == 1 for _, p in planes) and any(p[1] > 0 and p[2] == 1 for _, p in planes)
    assert any(p[2] == lc.CASES[x.tag].nz + 1 for x, p in planes) and any(p[1] < 64 < p[1] + p[2] and p[1] > 0 for _, p in planes)
    assert any(p[0] == "S" and x.op == "set" for x, p in planes) and any(p[0] == "S" and x.op == "add" for x, p in planes)
    assert any(p[0] == "S_anom" and x.op == "set" for x, p in planes) and {p[3] for _, p in planes} == {0, 1}


def _same_puts(mk, spec, shards):
    """a: put_dev of the restatement's planes; b (shards: a multi handle): remap_put_dev.  A launch per flux interval,
    the put behind the intervals spec.at: the written fields right after every put and the whole state after every
    launch - the launches behind a put among them."""
    case = _case(spec.tag, spec.ssref)
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    a, kca, k3a = resident(mk, case)
    b, kcb, k3b = resident(mk, case, shards)
    tabs = _define(b, case)
    puts = 0
    for r, nt, n in _intervals(case):
        for h in (a, b):
            h.fluxes(nt, *rec[r], **args)
            h.step(nt, n)
        sa, sb = _state(a, k3a, kca, case.nz), _state(b, k3b, kcb, case.nz)
        assert_same(sb, sa, active, f"{spec.tag} x{shards} after step {nt + n - 1}, {puts} puts")
        if r in spec.at:
            arrays = spec.arrays(tabs, r)
            planes, left = _on_model_points(spec, tabs, arrays, case.ncol)
            assert left >= len(EMPTIED) * sum(p[2] for p in spec.planes)
            a.put_dev([(name, _dev(p), lev0) for name, p, lev0 in planes], op=spec.op, time_levels=spec.time_levels, skip=SENTINEL)
            b.remap_put_dev([(name, g, _dev(v), lev0) for name, g, v, lev0 in arrays], **spec.kw())
            wa, wb = _written(a, k3a, kca, case.nz), _written(b, k3b, kcb, case.nz)
            assert_same(wb, wa, active, f"{spec.tag} x{shards} right after the put behind step {nt + n - 1}")
            assert any(not np.array_equal(wa[k][active], sa[k][active]) for k in WRITTEN), "the put changed nothing"
            puts += 1
        if puts == len(spec.at) and r > max(spec.at):
            break                       # (a further launch has followed the last put)
    assert puts == len(spec.at) and r > max(spec.at) and np.isfinite(sa["T"][active]).all()
    a.close()
    b.close()


@pytest.mark.parametrize("name", sorted(SPECS))
def test_remap_put_dev_is_put_dev_of_the_restatements_plane(mk, name):
    _same_puts(mk, SPECS[name], 0)


@pytest.mark.parametrize("name", ["add_f32_skip_time_levels", "set_f32_S_time_levels", "deep_add_skip_time_levels"])
def test_two_shards_take_the_same_puts(mk, name):
    _same_puts(mk, SPECS[name], 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_minus_zero_through_an_identity_table_leaves_the_golden_run_on_its_digests(mk, golden, tag, dtype):
    """x + 1.0 * (-0.0) is x for every x: planes of -0.0 on a permuted caller grid added to U, V, T, S_ANOM and their time
    levels between every two launches."""
    case = lc.CASES[tag]
    n = hr.grids(case.ncol)[1]
    table, perm = hr.identity_in(case.ncol, n, 31)
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    h.hgrid_define(3, n, table)
    h.flux_ring(2)
    zero = _dev(np.full((case.nz + 1, n), -0.0, dtype=dtype))

    def add(nt):
        h.remap_put_dev([(f, 3, zero) for f in STATE], op="add", time_levels=True)
        _assert_golden(golden, tag, nt, h, k3, kc, "-0.0 added through an identity table")

    _ring_run(h, case, 2, lambda r: h.flux_ring_put_dev(r, recd[r]), add)
    h.close()


PER_LAUNCH, PL, PR, SNAP = 4, 2, 3, 6   # steps of a launch; periods of the "last" and the mean schedule, of the snapshots


def test_a_remap_put_cancels_nothing(mk):
    """every_step_nz40 under two output schedules, an export, a flux ring, a step log of every column-step, a restart
    schedule and a series of bottom temperatures, in launches of 4 steps with a put between them: no launch is refused,
    the bookkeeping is that of the same run without puts, and records, log and state are those of a context that takes
    the restatement's planes through put_dev - which cancels nothing (tests/test_put_gpu.py)."""
    A = mk.api
    case = lc.CASES["every_step_nz40"]
    rec, args, npts, nzp1 = lc.flux_records(case), flux_args(case), case.ncol, case.nz + 1
    active = lc.active_columns(case)
    add = Spec("every_step_nz40", (("T", 0, nzp1, 1),), time_levels=True)
    ice = Spec("every_step_nz40", (("T", 0, 1, 0), ("S", 0, 1, 0)), op="set", skip=LAND)
    made = []
    for way in ("remap", "put", None):
        h, kc, k3 = resident(mk, case)
        tabs = _define(h, case)
        _schedule(mk, h, 1, PL, PR, nrec=8, red=("T", "hmix"), last=("T", "hmix"))
        h.window_export(1, "f8", LAND)
        h.flux_ring(PER_LAUNCH)
        h.step_log(4096, 1)
        h.restart_schedule(1, SNAP, 2)
        bt = np.stack([k3.X[:, case.nz, 0] - 0.5 + 0.1 * r for r in range(case.nsteps // PER_LAUNCH)])
        h.set_ancillary_series(A.ANC_BOTTOM_TEMP, 0, bt)
        h.ancillary_schedule(A.ANC_BOTTOM_TEMP, 1, PER_LAUNCH, list(range(len(bt))))
        made.append((way, h, kc, k3))
    for nt in range(1, case.nsteps + 1, PER_LAUNCH):
        for way, h, kc, k3 in made:
            for r in range(nt - 1, nt - 1 + PER_LAUNCH):
                h.flux_ring_put(r, rec[r])
            h.run_forced(nt, PER_LAUNCH, 1, **args)     # (a refused launch raises)
        books = [_book(h) for _, h, _, _ in made]
        assert books[0] == books[1] == books[2], f"after the launch from step {nt}"
        if nt + PER_LAUNCH <= case.nsteps:
            for way, h, kc, k3 in made[:2]:
                for spec in (add, ice):
                    arrays = spec.arrays(tabs, nt)
                    if way == "remap":
                        h.remap_put_dev([(f, g, _dev(v), l0) for f, g, v, l0 in arrays], **spec.kw())
                    else:
                        planes, _ = _on_model_points(spec, tabs, arrays, npts)
                        h.put_dev([(f, _dev(p), l0) for f, p, l0 in planes], op=spec.op, time_levels=spec.time_levels, skip=SENTINEL)
                assert _book(h) == books[2], f"{way}: after the puts behind step {nt + PER_LAUNCH - 1}"
    (_, h, kc, k3), (_, p, kcp, k3p), (_, plain, kcn, k3n) = made
    assert h.window_records(0) == (0, case.nsteps // PL - 1) and h.window_records(1) == (0, case.nsteps // PR - 1)
    assert h.restart_snapshots() == (0, case.nsteps // SNAP - 1)
    for s, period, fields, ops in ((0, PL, ("T", "hmix"), (3,)), (1, PR, ("T", "hmix"), (0, 1, 2))):
        for w in range(case.nsteps // period):
            for f in fields:
                for op in ops:
                    shape = (npts,) if f == "hmix" else (npts, nzp1)
                    x, y = np.full(shape, LAND, order="F"), np.full(shape, LAND, order="F")
                    h.window_record_fetch(s, w, f, op, x)
                    p.window_record_fetch(s, w, f, op, y)
                    assert np.array_equal(_bits(x), _bits(y)), ("schedule", s, "record", w, f, op)
                    if s == 1:
                        z = np.full(shape, -1.0, order="F")
                        h.window_export_fetch(1, w, f, op, z)
                        assert np.array_equal(_bits(z), _bits(x)), ("export", w, f, op)
    assert [np.array_equal(u, v) for u, v in zip(h.step_log_fetch(), p.step_log_fetch())] == [True] * 4
    end_h, end_p, end_plain = _state(h, k3, kc, case.nz), _state(p, k3p, kcp, case.nz), _state(plain, k3n, kcn, case.nz)
    assert_same(end_h, end_p, active, "the end state: remap puts against put_dev")
    assert not np.array_equal(end_h["T"][active], end_plain["T"][active]), "the puts changed nothing"
    for _, x, _, _ in made:
        x.close()


def test_remap_put_dev_waits_for_its_producer_and_the_fence_holds_the_overwrite(mk):
    """The plane is produced on a side stream behind FILLS fills of FILL_BYTES, remap_put_dev follows at once with no host
    synchronisation, and the tensor is overwritten with a large value on that stream right after dev_fence: a library
    that read too early sets the tensor's earlier content (-1), one whose fence did not hold the later one.  A race test
    can only fail, never prove."""
    import torch

    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    npts, nzp1, ocean = case.ncol, case.nz + 1, lc.ocean(case).astype(bool)
    n = hr.grids(npts)[1]
    table, perm = hr.identity_in(npts, n, 35)
    h.hgrid_define(0, n, table)
    values = 10.0 + np.arange(nzp1 * npts, dtype=np.float64).reshape(nzp1, npts) / 128.0
    src = _dev(hr.through(perm, n, values))
    side = torch.cuda.Stream()
    big = torch.empty(FILL_BYTES // 8, dtype=torch.float64, device="cuda")
    t = torch.full((nzp1, n), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for i in range(FILLS):
            big.fill_(float(i))
        t.copy_(src)
    h.remap_put_dev([("T", 0, t)], op="set", stream=side)
    h.dev_fence(side)
    with torch.cuda.stream(side):
        t.fill_(7e33)
    h.synchronize()
    h.download(k3)
    assert np.array_equal(_bits(k3.X[ocean, :, 0]), _bits(values.T[ocean])), "the state does not hold the first values"
    assert np.array_equal(k3.Tref[ocean], values[0, ocean])
    side.synchronize()
    h.close()


# ---------------------------------------------------------------------------
# 3. refusals, before anything is queued
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.MckppHipError
    case = lc.CASES["every_step_nz40"]
    npts, nzp1 = case.ncol, case.nz + 1
    rec, args = lc.flux_records(case), flux_args(case)
    h, kc, k3 = resident(mk, case)
    tabs = _define(h, case)
    n = tabs[1][0]
    h.hgrid_define(2, n, tabs[1][1], None)      # no out table
    h.hgrid_define(3, n, None, tabs[1][2])      # no in table
    _schedule(mk, h, 1, PL, PR, nrec=2, red=("T", "hmix"), last=("T", "hmix"))
    h.flux_ring(4)
    for r in range(4):
        h.flux_ring_put(r, rec[r])
    h.run_forced(1, 4, 1, **args)               # schedule 0 (last, period 2): records 0, 1; schedule 1 (period 3): record 0
    h.window_record_release(0, 0)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()

    def everything():
        s = _state(h, k3, kc, case.nz)
        return ([h.window_records(0), h.window_records(1), h.flux_ring_records()] + [h.hgrid_info(g) for g in range(2)],
                {k: _bits(np.nan_to_num(v.astype(np.float64))).copy() for k, v in s.items()})

    before = everything()
    out = torch.full((nzp1, n), -5.0, dtype=torch.float64, device="cuda")
    good = torch.zeros((nzp1, n), dtype=torch.float64, device="cuda")
    pinned = torch.zeros(n * nzp1, dtype=torch.float64).pin_memory()
    pageable = np.zeros(n * nzp1)
    big, small, holds = _short_of(torch, n * 8)      # an address with room for n - 1 doubles
    R, P = A._RemapRecordPlaneC, A._RemapPutPlaneC
    rok = dict(sched=1, field=A.OUT["T"], op=0, lev0=0, nlev=nzp1, dtype=A.EXP_F64, grid=1, norm=0, fill_land=1, rec=0,
               land_value=LAND, out=out.data_ptr())
    pok = dict(field=A.OUT["T"], lev0=0, nlev=nzp1, dtype=A.EXP_F64, op=A.PUT_ADD, flags=0, grid=1, skip_value=0.0)

    def records(*planes):
        return lib.mckpp_hip_remap_records_dev(h._h, len(planes), (R * len(planes))(*[R(**{**rok, **p}) for p in planes]), None)

    def put(*planes):
        tab = (P * len(planes))(*[P(**{**pok, "in": good.data_ptr(), **p}) for p in planes])
        return lib.mckpp_hip_remap_put_dev(h._h, len(planes), tab, None)

    rname, pname = "mckpp_hip_remap_records_dev: ", "mckpp_hip_remap_put_dev: "
    table = [   # (call, message fragment)
        # what records_dev refuses of the plane
        (lambda: records(dict(sched=2)), rname + "planes[0]: schedule 2 is not set"),
        (lambda: records(dict(sched=9)), rname + "planes[0]: schedule 9"),
        (lambda: records({}, dict(rec=1)), rname + "planes[1]: record 1 of schedule 1 (steps 4..6) is incomplete: steps have run up to 4"),
        (lambda: records(dict(sched=0, op=3, rec=0)), rname + "planes[0]: record 0 of schedule 0 (steps 1..2) has been released"),
        (lambda: records(dict(field=A.OUT["S"])), rname + f"planes[0]: field {A.OUT['S']} is not in schedule 1"),
        (lambda: records(dict(op=3)), rname + "planes[0]: schedule 1 keeps no op 3 of field 2"),
        (lambda: records(dict(op=4)), rname + "planes[0]: op 4 (0 mean, 1 min, 2 max, 3 last)"),
        (lambda: records(dict(lev0=nzp1 - 1, nlev=2)), rname + "planes[0]: lev0="),
        (lambda: records(dict(nlev=0)), rname + "planes[0]: lev0=0 nlev=0"),
        (lambda: records(dict(dtype=7)), rname + "planes[0]: dtype 7"),
        # what hgrid_fetch_dev refuses
        (lambda: records(dict(grid=-1)), rname + "planes[0]: grid -1 is not defined"),
        (lambda: records({}, dict(grid=2, out=good.data_ptr())), rname + "planes[1]: grid 2 has no out table"),
        (lambda: records(dict(norm=2)), rname + "planes[0]: norm 2 (MCKPP_HGRID_NORM_NONE 0, MCKPP_HGRID_NORM_USED 1)"),
        (lambda: records(dict(nlev=2), dict(out=out.data_ptr() + 8 * n, nlev=1, field=A.OUT["hmix"])),
         rname + "planes[1].out and planes[0].out overlap"),
        (lambda: records(dict(out=small, nlev=1)),
         rname + f"planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {8 * n}"),
        (lambda: records(dict(out=pageable.ctypes.data, nlev=1)), rname + "planes[0].out is host memory"),
        (lambda: records(dict(out=pinned.data_ptr(), nlev=1)), rname + "planes[0].out is pinned host memory"),
        (lambda: records(dict(out=None)), rname + "planes[0].out is null"),
        (lambda: lib.mckpp_hip_remap_records_dev(h._h, 65, (R * 65)(), None), rname + "nplanes=65 (0..64)"),
        (lambda: lib.mckpp_hip_remap_records_dev(h._h, 1, None, None), rname + "nplanes=1 (0..64) or a null table"),
        # what put_dev refuses
        (lambda: put(dict(field=99)), pname + "planes[0]: unknown output field 99"),
        (lambda: put(dict(field=A.OUT["hmix"], nlev=1)), pname + "planes[0]: field 4 is an output of the step, not state"),
        (lambda: put({}, dict(field=A.OUT["rho"])), pname + "planes[1]: field 16 is an output of the step"),
        (lambda: put(dict(lev0=1)), pname + "planes[0]: lev0=1 nlev=41 is no range of levels of field 2, whose axis has 41"),
        (lambda: put(dict(nlev=0)), pname + "planes[0]: lev0=0 nlev=0 is no range"),
        (lambda: put(dict(dtype=0)), pname + "planes[0]: dtype 0"),
        (lambda: put(dict(op=2)), pname + "planes[0]: op 2 (MCKPP_PUT_SET 0, MCKPP_PUT_ADD 1)"),
        (lambda: put(dict(flags=4)), pname + "planes[0]: flags 0x4"),
        (lambda: put(dict(flags=A.PUT_SKIP, skip_value=float("nan"))), pname + "planes[0]: the skip value is NaN"),
        (lambda: put(dict(nlev=10), dict(lev0=5, nlev=3)),
         pname + "planes[1] and planes[0] write the same field (2, 2) at overlapping levels 5..7 and 0..9"),
        (lambda: put(dict(field=A.OUT["S_anom"], lev0=40, nlev=1), dict(field=A.OUT["S"], lev0=40, nlev=1, grid=0)),
         pname + "planes[1] and planes[0] write the same field (5, 3) at overlapping levels 40..40 and 40..40"),
        (lambda: put({"in": pinned.data_ptr()}), pname + "planes[0].in is pinned host memory"),
        (lambda: put({}, {"field": A.OUT["u"], "in": pageable.ctypes.data}), pname + "planes[1].in is host memory"),
        (lambda: put({"in": None}), pname + "planes[0].in is null"),
        # the grid
        (lambda: put(dict(grid=7)), pname + "planes[0]: grid 7 is not defined"),
        (lambda: put({}, dict(field=A.OUT["u"], grid=3)), pname + "planes[1]: grid 3 has no in table"),
        (lambda: put({"in": small, "nlev": 1}),
         pname + f"planes[0].in: the allocation holds {holds} bytes from the pointer on, the call needs {8 * n}"),
        (lambda: lib.mckpp_hip_remap_put_dev(h._h, 65, (P * 65)(), None), pname + "nplanes=65 (0..64)"),
        (lambda: lib.mckpp_hip_remap_put_dev(h._h, -1, (P * 1)(), None), pname + "nplanes=-1"),
        (lambda: lib.mckpp_hip_remap_put_dev(h._h, 1, None, None), pname + "nplanes=1 (0..64) or a null table"),
    ]
    for call, text in table:
        assert call() < 0, text
        assert text in err(), (text, err())
    assert records() == 0 and put() == 0        # no plane: nothing to do
    # no state uploaded; a grid defined for another npts
    fresh = mk.MckppHip(kc)
    tab = (P * 1)(P(**pok, **{"in": good.data_ptr()}))
    assert lib.mckpp_hip_remap_put_dev(fresh._h, 1, tab, None) < 0 and err() == pname + "upload the state first"
    assert lib.mckpp_hip_remap_records_dev(fresh._h, 1, (R * 1)(R(**rok)), None) < 0 and err().startswith(rname)
    fresh.close()
    other = lc.CASES["l_rest"]
    assert other.ncol != npts and other.nz == case.nz
    g, kcg, k3g = resident(mk, other)
    g.hgrid_define(0, 5, hr.csr([[(0, 1.0)]] * other.ncol), hr.csr([[(0, 1.0)]] * 5))
    g.window_schedule(0, 1, 1, 1, ("T",), A.WIN_MEAN)
    g.step(1, 1)
    k3w = lc.hip_raw(case)[1]
    g.upload(k3w)                                # the state now has npts points, the grid was defined for other.ncol
    g.init_ocean(0)
    five = torch.zeros((nzp1, 5), dtype=torch.float64, device="cuda")
    tab = (P * 1)(P(**{**pok, "grid": 0, "in": five.data_ptr()}))
    assert lib.mckpp_hip_remap_put_dev(g._h, 1, tab, None) < 0
    assert err() == pname + f"planes[0]: grid 0 was defined for npts={other.ncol}, the state has {npts}: define it again", err()
    g.window_schedule(0, 1, 1, 1, ("T",), A.WIN_MEAN)
    g.step(1, 1)
    assert lib.mckpp_hip_remap_records_dev(g._h, 1, (R * 1)(R(**{**rok, "sched": 0, "grid": 0, "out": five.data_ptr()})), None) < 0
    assert err() == rname + f"planes[0]: grid 0 was defined for npts={other.ncol}, the state has {npts}: define it again", err()
    g.close()
    # a multi handle checks every plane of every shard before any shard queues
    m, kcm, k3m = resident(mk, case, shards=2)
    _define(m, case)
    m_before = {k: v.copy() for k, v in _state(m, k3m, kcm, case.nz).items()}
    tab2 = (P * 2)(P(**pok, **{"in": good.data_ptr()}), P(**{**pok, "field": A.OUT["u"], "in": pinned.data_ptr()}))
    assert lib.mckpp_hip_multi_remap_put_dev(m._h, 2, tab2, None) < 0
    assert err().startswith("mckpp_hip_multi_remap_put_dev: planes[1].in is pinned host memory"), err()
    assert lib.mckpp_hip_multi_remap_records_dev(m._h, 1, (R * 1)(R(**rok)), None) < 0
    assert err().startswith("mckpp_hip_multi_remap_records_dev: planes[0]: schedule 1 is not set"), err()
    assert_same(_state(m, k3m, kcm, case.nz), m_before, slice(None), "the shards after the refusals")
    m.close()
    # the Python layer's texts, and the library's through it
    with pytest.raises(ValueError, match="a host array"):
        h.remap_put_dev([("T", 1, pinned)])
    with pytest.raises(E, match=r"mckpp_hip_remap_records_dev: planes\[0\]: record 5 of schedule 1"):
        h.remap_records_dev([(1, 5, "T", 0, 1, out)])
    after = everything()
    assert after[0] == before[0], "a refused call touched the schedules, the ring or the grids"
    assert after[1].keys() == before[1].keys() and all(np.array_equal(after[1][k], before[1][k]) for k in before[1]), \
        "a refused call touched the state"
    assert (out.cpu().numpy() == -5.0).all() and not good.cpu().numpy().any()
    # ... and the run goes on: a good delivery, a good put, the next launch under every schedule
    h.remap_records_dev([(1, 0, "T", 0, 1, out), (0, 1, "hmix", 3, 0, torch.zeros((1, tabs[0][0]), dtype=torch.float64, device="cuda"))])
    assert (out.cpu().numpy() != -5.0).all()
    h.remap_put_dev([("T", 1, good)], op="add")
    h.window_record_release(0, 1)
    h.window_record_release(1, 0)
    for r in range(4, 8):
        h.flux_ring_put(r, rec[r])
    h.run_forced(5, 4, 1, **args)
    assert h.window_records(1) == (1, 1)
    h.close()
