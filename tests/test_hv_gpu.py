"""A caller grid and a caller axis in one call (include/mckpp_hip_hv.h: mckpp_hip_hv_fetch_dev, mckpp_hip_hv_put_dev and
their multi_ twins; k_vaxis_fetch_planes into the staging and k_hgrid_out, k_hv_put_planes).

Every value comparison is an equality of bits; no test has a tolerance and none skips a case.  The yardsticks are the
existing calls and the two numpy restatements, tests/hgrid_ref.py of include/mckpp_hip_hgrid.h and tests/vaxis_ref.py of
include/mckpp_hip_vaxis.h, composed in the order the header states:
  fields out  hgrid_ref.apply(out table, x[j], n, used = the resident points, norm, fill) per caller level j, with x
              mckpp_hip_vaxis_fetch_dev's array of the same field and axis on the model's points - itself held to
              vaxis_ref.vinterp of mckpp_hip_window_fetch;
  state in    on a second context the existing mckpp_hip_put_dev of the plane formed on the host - hgrid_ref.apply in
              the in direction per caller level, then vaxis_ref.vinterp onto zm - with MCKPP_PUT_SKIP on a sentinel at
              every element the header leaves alone: the row is empty, or an entry reads the skip value at a caller
              level the model level's branch reads.
Cases, axes and tables are those of tests/test_remap_gpu.py and tests/test_vaxis_gpu.py: every_step_nz40 (30 columns of
40 points: one partial column tile, 41 levels), sweep_nd3 (more than 256 columns, no multiple of 64) and deep_nz100_nd4
(101 levels: two model-level tiles, an 8-level group partly past the axis); the axes two, coarse7, fine130 and equal;
the two grids of hgrid_ref.grids with rows of 0, 1, 4 and 70 entries, negative weights and repeated indices, the in rows
of two resident columns emptied.  Two shards are two contexts on the one device, as everywhere in this suite."""
import dataclasses

import numpy as np
import pytest

import hgrid_ref as hr
import ref_loop_cases as lc
import vaxis_ref as vr
from harness import assert_same, flux_args, mk, resident  # noqa: F401
from test_device_arrays_gpu import FILL_BYTES, FILLS, _bits, _dev, _intervals, _state
from test_put_gpu import WRITTEN, _book, _case, _written
from test_remap_gpu import EMPTIED, _tables
from test_remap_gpu import _define as _define_grids
from test_vaxis_gpu import AMPLITUDE, AXES, AXIS_NO, _short_of
from test_vaxis_gpu import _define as _define_axes
from test_window_schedule_gpu import _schedule

pytestmark = pytest.mark.gpu

CASES = ("every_step_nz40", "sweep_nd3", "deep_nz100_nd4")
LAND = hr.LAND
SKIP = -999.0
SENTINEL = -7.5e300           # what put_dev skips on the yardstick's side: no value comes near it
HELD = -7.0                   # what the out arrays hold before a delivery
FETCHED = ("T", "S", "u", "rho", "dbloc")
COMBOS = [(axis, g) for axis in AXES for g in (0, 1)]
# ten planes of one call: every field on two (axis, grid) pairs, every axis on both grids
FETCH_PLANES = [(f,) + COMBOS[(2 * i + j) % len(COMBOS)] for i, f in enumerate(FETCHED) for j in (0, 1)]
STATE_NAME = {"u": "U", "v": "V", "T": "T", "S_anom": "S", "S": "S"}


def _zm(kc, case):
    return np.array(kc.zm[:case.nz + 1])


def test_cases_axes_and_tables_reach_the_paths_of_the_kernels():
    ncol = {t: len(lc.active_columns(lc.CASES[t])) for t in CASES}
    assert ncol["every_step_nz40"] == 30 and lc.CASES["every_step_nz40"].ncol == 40 and lc.CASES["every_step_nz40"].nz + 1 == 41
    assert ncol["sweep_nd3"] > 256 and ncol["sweep_nd3"] % 64 and ncol["sweep_nd3"] < lc.CASES["sweep_nd3"].ncol
    nzp1 = lc.CASES["deep_nz100_nd4"].nz + 1
    assert nzp1 == 101 and 64 < nzp1 <= 128 and (nzp1 - 64) % 8      # two level tiles; an 8-level group partly past the axis
    assert set(FETCH_PLANES) >= {(f,) + c for f, c in zip(FETCHED, COMBOS[::2])} and {p[1:] for p in FETCH_PLANES} == set(COMBOS)
    for tag in CASES:
        case = lc.CASES[tag]
        kc, _ = lc.hip_raw(case)
        zm = _zm(kc, case)
        ax = vr.axes(kc.zm[:case.nz + 1])
        assert set(ax) == set(AXES)
        # fields out: the caller's levels against zm
        out_branch = {a: list(vr.carried_brackets(zm, ax[a])[0]) for a in AXES}
        assert out_branch["two"] == [vr.ABOVE, vr.BELOW]                                     # both clamps
        assert len(ax["fine130"]) == 130 > 128 and {vr.ABOVE, vr.BELOW, vr.BRACKET} == set(out_branch["fine130"])   # three tiles
        assert set(out_branch["coarse7"]) == {vr.BRACKET} == set(out_branch["equal"])
        assert sum(z in zm for z in ax["equal"]) >= 4                                        # the equality branch
        # state in: zm against the caller's levels
        in_tab = {a: vr.carried_brackets(ax[a], zm) for a in AXES}
        assert set(in_tab["two"][0]) == {vr.BRACKET} and set(in_tab["two"][1]) == {0}
        assert {vr.ABOVE, vr.BELOW, vr.BRACKET} == set(in_tab["coarse7"][0])                 # clamps above and below
        assert (np.diff(in_tab["fine130"][1]) > 1).any()           # caller levels between two model levels: kin skips
        assert (np.diff(in_tab["coarse7"][1]) == 0).any()          # neighbouring model levels share a caller level
        assert set(in_tab["equal"][0]) == {vr.BRACKET} and in_tab["equal"][1][0] == 0 and in_tab["equal"][1][-1] == len(ax["equal"]) - 2
        # the tables
        ocean, active = lc.ocean(case), lc.active_columns(case)
        for n, tin, tout in _tables(case):
            lin, lout = np.diff(tin[0]), np.diff(tout[0])
            empty = np.nonzero((lin == 0) & (ocean != 0))[0]
            assert list(empty) == [active[k] for k in EMPTIED], "exactly the emptied rows of resident columns are empty"
            assert {1, 4, 70} <= set(lin[active]) and lout.max() == 70 and (tin[2] < 0).any() and (tout[2] < 0).any()
            assert any(len(set(tin[1][tin[0][r]:tin[0][r + 1]])) < lin[r] for r in range(case.ncol))   # repeated indices
            assert (tin[1] % 3 == 1).any() and n % 64                # an entry reads a skipped caller point; a grid's tail


# ---------------------------------------------------------------------------
# 1. fields out
# ---------------------------------------------------------------------------
class Stepped:
    """A context of a case (shards > 0: a multi handle) a few steps on, the two grids and the four axes defined; for
    the single context window_fetch of the fetched fields, vaxis_fetch_dev's arrays on the model's points - NaN where
    no column is resident - and the restatement of every plane of FETCH_PLANES, each computed once."""

    def __init__(self, mk, tag, shards=0):
        import torch

        self.case = case = lc.CASES[tag]
        self.h, self.kc, self.k3 = resident(mk, case, shards)
        self.tabs = _define_grids(self.h, case)
        self.ax = _define_axes(self.h, self.kc)
        self.ocean = lc.ocean(case)
        rec, args, steps = lc.flux_records(case), flux_args(case), 0
        for r, nt, n in _intervals(case):
            if steps >= 3:
                break
            self.h.fluxes(nt, *rec[r], **args)
            self.h.step(nt, n)
            steps += n
        assert steps >= 3
        self.wants = {}
        if shards:
            return
        zm, sea = _zm(self.kc, case), self.ocean.astype(bool)
        self.x = {}
        pairs = [(f, axis) for f in FETCHED for axis in AXES]
        outs = [torch.full((len(self.ax[axis]), case.ncol), float("nan"), dtype=torch.float64, device="cuda") for _, axis in pairs]
        self.h.vaxis_fetch_dev([(f, AXIS_NO[axis], o) for (f, axis), o in zip(pairs, outs)], fill_land=False)
        model = {}
        for f in FETCHED:
            out = np.full((case.ncol, case.nz + 1), LAND, order="F")
            self.h.window_fetch(mk.api._win_field(f), mk.api.OP_INSTANT, out)
            model[f] = np.ascontiguousarray(out.T)
        for (f, axis), o in zip(pairs, outs):
            x = o.cpu().numpy()
            assert np.array_equal(_bits(x[:, sea]), _bits(vr.vinterp(zm, model[f], self.ax[axis])[:, sea])), (tag, f, axis)
            assert np.isnan(x[:, ~sea]).all()
            x.flags.writeable = False
            self.x[f, axis] = x

    def want(self, norm, fill):
        """per plane of FETCH_PLANES the restatement (n_axis, n_grid) in doubles, for out arrays that held HELD"""
        if (norm, fill) not in self.wants:
            made = []
            for f, axis, g in FETCH_PLANES:
                n, _, tout = self.tabs[g]
                x = self.x[f, axis]
                w = np.stack([hr.apply(tout, x[j], n, self.ocean, norm, fill, LAND, np.full(n, HELD)) for j in range(x.shape[0])])
                assert np.isfinite(w).all(), "a position that is no row was read"
                w.flags.writeable = False
                made.append(w)
            self.wants[norm, fill] = made
        return self.wants[norm, fill]

    def fetch(self, h, dtype, norm, fill):
        import torch

        tdt = torch.float64 if dtype == np.float64 else torch.float32
        outs = [torch.full((len(self.ax[axis]), self.tabs[g][0]), HELD, dtype=tdt, device="cuda") for _, axis, g in FETCH_PLANES]
        h.hv_fetch_dev([(f, g, AXIS_NO[axis], o) for (f, axis, g), o in zip(FETCH_PLANES, outs)], norm=norm, land_value=LAND,
                       fill_land=fill)
        return [o.cpu().numpy() for o in outs]


@pytest.fixture(scope="module")
def stepped(mk):
    made = {}

    def get(tag, shards=0):
        if (tag, shards) not in made:
            made[tag, shards] = Stepped(mk, tag, shards)
        return made[tag, shards]

    yield get
    for s in made.values():
        s.h.close()


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("norm", hr.NORMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", CASES)
def test_fetch_is_the_restatement_of_vaxis_fetch_dev(mk, stepped, tag, dtype, norm, fill):
    """Ten planes of five fields, four axes and two grids in one call."""
    s = stepped(tag)
    wants = s.want(norm, fill)
    for p, got, want in zip(FETCH_PLANES, s.fetch(s.h, dtype, norm, fill), wants):
        assert got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want.astype(dtype))), (tag, p, np.dtype(dtype).name, norm, fill)
    if (s.ocean == 0).any():     # what general_out's rows are built for shows at every caller level
        for p, want in zip(FETCH_PLANES, wants):
            none = LAND if fill else HELD
            assert (want[:, 0] == none).all() and (want[:, 2] == none).all() and (want[:, 3] != none).all(), p
            assert (want[:, 4] == none).all() == (norm == "used"), p


# ---------------------------------------------------------------------------
# 2. state in
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class Spec:
    """One put: planes (field, axis name, grid), the keywords, the caller array's element type"""
    tag: str
    planes: tuple
    op: str = "add"
    dtype: type = np.float64
    time_levels: bool = False
    skip: bool = False
    ssref: int = 1

    def arrays(self, tabs, ax, r=0):
        """(field, axis name, grid, array (n_axis, n_grid)): amplitude * sin(point + height / 20 + plane + r), around a
        value of the field's size where the operation is a set; with skip, every third caller point holds the skip value
        at one caller level only, the middle one"""
        out = []
        for i, (name, axis, g) in enumerate(self.planes):
            n, z = tabs[g][0], ax[axis]
            v = AMPLITUDE[name] * np.sin(np.arange(n)[None, :] + z[:, None] / 20.0 + i + r + 0.5)
            if self.op == "set":
                v = v * 100.0 + {"T": 12.0, "S": 35.0}.get(name, 0.0)
            v = np.ascontiguousarray(v.astype(self.dtype))
            if self.skip:
                assert float(self.dtype(SKIP)) == SKIP and not (v == SKIP).any()
                v[len(z) // 2, 1::3] = SKIP
            out.append((name, axis, g, v))
        return out

    def kw(self):
        return dict(op=self.op, time_levels=self.time_levels, skip=SKIP if self.skip else None)


def _on_model_points_and_levels(spec, tabs, ax, arrays, npts):
    """[(field, plane (nzp1, npts), alone (nzp1, npts))]: the arrays through the in tables per caller level and then
    through vinterp onto zm, by the two restatements; alone: the elements the header leaves as they are - the row is
    empty, or an entry of it reads the skip value at a caller level the model level's branch reads"""
    out = []
    for name, axis, g, v in arrays:
        ptr, idx, w = tabs[g][1]
        z, zm = ax[axis], ax["zm"]
        v64 = v.astype(np.float64)      # widened exactly before anything else
        sums = np.stack([hr.apply((ptr, idx, w), v64[k], npts) for k in range(len(z))])
        plane = vr.vinterp(z, sums, zm)
        empty = np.diff(ptr) == 0
        alone = np.broadcast_to(empty, plane.shape).copy()
        if spec.skip:
            ones = (ptr, idx, np.ones_like(w))
            reads = np.stack([hr.apply(ones, (v64[k] == SKIP).astype(np.float64), npts) for k in range(len(z))]) > 0
            alone |= vr.untouched(z, np.where(reads, SKIP, 0.0), zm, SKIP)
            # ... which is: the model levels that read the middle caller level, of the columns with an entry at a
            # caller point that holds the skip value, and the columns with emptied rows
            level = np.array([len(z) // 2 in lv for lv in vr.levels_read(z, zm)])
            column = np.array([(idx[ptr[c]:ptr[c + 1]] % 3 == 1).any() for c in range(npts)])
            assert np.array_equal(alone, np.outer(level, column) | empty[None, :]) and level.any() and column.any()
            assert not alone[:, ~column & ~empty].any() and not alone.all()
        assert not (plane == SENTINEL).any() and not (plane == SKIP).any()
        out.append((name, plane, alone))
    return out


SPECS = {
    "add_f64": Spec("every_step_nz40", (("T", "coarse7", 1), ("u", "two", 0), ("S_anom", "equal", 1))),
    # SET f32 on S (minus Sref; L_SSref = 0: Ssurf restated), both time levels; many caller levels per model level
    "set_f32_S_time_levels": Spec("every_step_nz40", (("S", "fine130", 0), ("v", "coarse7", 1), ("T", "equal", 0)), op="set",
                                  dtype=np.float32, time_levels=True, ssref=0),
    "add_skip_two_levels": Spec("every_step_nz40", (("T", "two", 1), ("S", "equal", 0)), skip=True, ssref=0),
    # more than 256 columns, a tail of the 64-column tiles
    "add_f32_S_skip_time_levels": Spec("sweep_nd3", (("u", "coarse7", 1), ("T", "equal", 0), ("S", "fine130", 1)), dtype=np.float32,
                                       time_levels=True, skip=True, ssref=0),
    "set_f64_skip": Spec("sweep_nd3", (("T", "fine130", 1), ("S", "coarse7", 0), ("v", "two", 1)), op="set", skip=True),
    # two model-level tiles, the second one's 8-level groups partly past the axis
    "deep_add_skip_time_levels": Spec("deep_nz100_nd4", (("T", "fine130", 1), ("S_anom", "coarse7", 0), ("v", "equal", 1)), skip=True,
                                      time_levels=True),
    "deep_set_f32": Spec("deep_nz100_nd4", (("T", "coarse7", 0), ("S_anom", "equal", 1), ("u", "fine130", 1), ("v", "two", 0)),
                         op="set", dtype=np.float32),
}


def test_the_specs_cover_what_the_kernel_can_be_asked():
    s = SPECS.values()
    assert {x.op for x in s} == {"set", "add"} and {x.dtype for x in s} == {np.float64, np.float32}
    assert {x.time_levels for x in s} == {True, False} and {x.skip for x in s} == {True, False}
    assert {x.ssref for x in s} == {0, 1} and {x.tag for x in s} == set(CASES)
    assert any(x.skip and x.op == "set" for x in s) and any(x.skip and x.op == "add" for x in s)
    planes = [(x, p) for x in s for p in x.planes]
    assert {p[1:] for _, p in planes} == set(COMBOS)                                  # every axis on both grids
    assert {p[1] for x, p in planes if x.skip} == set(AXES)
    assert any(p[0] == "S" and x.op == "set" and not x.ssref for x, p in planes)     # minus Sref, Ssurf restated
    assert any(p[0] == "S" and x.op == "add" for x, p in planes) and any(p[0] == "S" and x.ssref for x, p in planes)
    assert any(p[0] == "S_anom" and x.op == "set" for x, p in planes)


def _same_put(mk, spec, shards=0):
    """Context a takes hv_put_dev (`shards` > 0: a multi handle), context b put_dev with skip of the plane formed on the
    host: the sixteen written arrays right after the put, and the whole state three steps later.  With skip, the
    elements that stayed as they were are exactly those the header leaves alone."""
    case = _case(spec.tag, spec.ssref)
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    a, kca, k3a = resident(mk, case, shards)
    b, kcb, k3b = resident(mk, case)
    tabs = _define_grids(a, case)
    ax = _define_axes(a, kca)
    ax["zm"] = _zm(kca, case)
    both = ((a, kca, k3a), (b, kcb, k3b))
    intervals = list(_intervals(case))

    def advance(r, nt, n):
        for h, _, _ in both:
            h.fluxes(nt, *rec[r], **args)
            h.step(nt, n)

    advance(*intervals[0])
    before = _state(b, k3b, kcb, case.nz)
    assert_same(_state(a, k3a, kca, case.nz), before, active, f"{spec.tag} x{shards}: before the put")
    arrays = spec.arrays(tabs, ax)
    model = _on_model_points_and_levels(spec, tabs, ax, arrays, case.ncol)
    a.hv_put_dev([(f, g, AXIS_NO[axis], _dev(v)) for f, axis, g, v in arrays], **spec.kw())
    b.put_dev([(f, _dev(np.where(alone, SENTINEL, plane)), 0) for f, plane, alone in model], op=spec.op,
              time_levels=spec.time_levels, skip=SENTINEL)
    got, want = _written(a, k3a, kca, case.nz), _written(b, k3b, kcb, case.nz)
    assert_same(got, want, active, f"{spec.tag} x{shards}: right after the put")
    assert any(not np.array_equal(got[k][active], before[k][active]) for k in WRITTEN), "the put changed nothing"
    for f, plane, alone in model:      # ... seen on the state itself: those elements, and no others, stayed as they were
        stayed = _bits(got[STATE_NAME[f]][active]) == _bits(before[STATE_NAME[f]][active])
        assert np.array_equal(stayed, alone.T[active]), (spec.tag, f)
        assert stayed[[EMPTIED[0], EMPTIED[1]]].all()
    steps = 0
    for r, nt, n in intervals[1:]:
        if steps >= 3:
            break
        advance(r, nt, n)
        steps += n
    assert steps >= 3
    end = _state(b, k3b, kcb, case.nz)
    assert_same(_state(a, k3a, kca, case.nz), end, active, f"{spec.tag} x{shards}: {steps} steps after the put")
    assert np.isfinite(end["T"][active]).all()
    a.close()
    b.close()


@pytest.mark.parametrize("name", sorted(SPECS))
def test_hv_put_dev_is_put_dev_of_the_restatements_plane(mk, name):
    _same_put(mk, SPECS[name])


# ---------------------------------------------------------------------------
# 3. two shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_two_shards_deliver_the_single_contexts_bits(mk, stepped, tag):
    """a multi handle of two shards against the single context's deliveries and the restatement applied to the single
    context's arrays: the used entries are the columns of any shard"""
    one, m = stepped(tag), stepped(tag, 2)
    mask0, n0 = mk.api.host_shard_mask(m.k3.run_physics, 2, 0)
    assert 0 < n0 < len(lc.active_columns(one.case)), "both shards hold columns"
    for dtype, norm, fill in ((np.float64, "used", True), (np.float32, "none", False)):
        a, b, wants = one.fetch(one.h, dtype, norm, fill), one.fetch(m.h, dtype, norm, fill), one.want(norm, fill)
        for p, x, y, want in zip(FETCH_PLANES, a, b, wants):
            assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(y), _bits(want.astype(dtype))), (tag, p, norm, fill)
    # ... and a shard's tables follow who addresses it: the single context again, unchanged
    for p, x, want in zip(FETCH_PLANES, one.fetch(one.h, np.float64, "used", True), one.want("used", True)):
        assert np.array_equal(_bits(x), _bits(want)), (tag, p, "the single context afterwards")


@pytest.mark.parametrize("name", ["add_f32_S_skip_time_levels", "set_f32_S_time_levels", "deep_add_skip_time_levels"])
def test_two_shards_take_the_same_put(mk, name):
    _same_put(mk, SPECS[name], shards=2)


# ---------------------------------------------------------------------------
# 4. ordering on the device
# ---------------------------------------------------------------------------
def test_hv_put_dev_waits_for_its_producer_and_the_fence_holds_the_overwrite(mk):
    """The plane is produced on a side stream behind FILLS fills of FILL_BYTES, hv_put_dev follows at once with no host
    synchronisation, and the tensor is overwritten with a large value on that stream right after dev_fence: a library
    that read too early sets what the tensor's earlier content (-1) interpolates to, one whose fence did not hold the
    later one.  A race test can only fail, never prove."""
    import torch

    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    npts, ocean = case.ncol, lc.ocean(case).astype(bool)
    n = hr.grids(npts)[1]
    table, perm = hr.identity_in(npts, n, 35)
    h.hgrid_define(0, n, table)
    z, zm = _define_axes(h, kc)["coarse7"], _zm(kc, case)
    values = 10.0 + np.arange(len(z) * npts, dtype=np.float64).reshape(len(z), npts) / 128.0
    src = _dev(hr.through(perm, n, values))
    side = torch.cuda.Stream()
    big = torch.empty(FILL_BYTES // 8, dtype=torch.float64, device="cuda")
    t = torch.full((len(z), n), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for i in range(FILLS):
            big.fill_(float(i))
        t.copy_(src)
    h.hv_put_dev([("T", 0, AXIS_NO["coarse7"], t)], op="set", stream=side)
    h.dev_fence(side)
    with torch.cuda.stream(side):
        t.fill_(7e33)
    h.synchronize()
    h.download(k3)
    want = vr.vinterp(z, values, zm)
    assert np.array_equal(_bits(k3.X[ocean, :, 0]), _bits(want.T[ocean])), "the state does not hold the first values"
    assert np.array_equal(k3.Tref[ocean], want[0, ocean])
    side.synchronize()
    h.close()


def test_hv_fetch_dev_for_a_consumer_on_a_side_stream(mk, stepped):
    """The consumer's kernels follow the call on a side stream with no host synchronisation between; the arrays are
    rewritten on that stream before the call, which the delivery must follow."""
    import torch

    s = stepped("sweep_nd3")
    f, axis, g = FETCH_PLANES[4]
    n, nax = s.tabs[g][0], len(s.ax[axis])
    side = torch.cuda.Stream()
    out = torch.empty((nax, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out.fill_(HELD)
        s.h.hv_fetch_dev([(f, g, AXIS_NO[axis], out)], norm="none", land_value=LAND, fill_land=False)
        total = torch.add(out, 1.0)
    side.synchronize()
    want = s.want("none", False)[4]
    assert np.array_equal(_bits(total.cpu().numpy()), _bits(want + 1.0))


# ---------------------------------------------------------------------------
# 5. nothing is cancelled
# ---------------------------------------------------------------------------
PER_LAUNCH, PL, PR, SNAP = 4, 2, 3, 6   # steps of a launch; periods of the "last" and the mean schedule, of the snapshots


def test_an_hv_put_cancels_nothing(mk):
    """every_step_nz40 under two output schedules, an export, a flux ring, a step log of every column-step, a restart
    schedule and a series of bottom temperatures, in launches of 4 steps with a put between them: no launch is refused,
    the bookkeeping is that of the same run without puts, and records, log and state are those of a context that takes
    the restatement's planes through put_dev - which cancels nothing (tests/test_put_gpu.py)."""
    A = mk.api
    case = lc.CASES["every_step_nz40"]
    rec, args, npts, nzp1 = lc.flux_records(case), flux_args(case), case.ncol, case.nz + 1
    active = lc.active_columns(case)
    add = Spec("every_step_nz40", (("T", "coarse7", 1),), time_levels=True)
    ice = Spec("every_step_nz40", (("u", "two", 0), ("S", "equal", 0)), op="set", skip=True)
    made = []
    for way in ("hv", "put", None):
        h, kc, k3 = resident(mk, case)
        tabs = _define_grids(h, case)
        ax = _define_axes(h, kc)
        ax["zm"] = _zm(kc, case)
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
                    arrays = spec.arrays(tabs, ax, nt)
                    if way == "hv":
                        h.hv_put_dev([(f, g, AXIS_NO[axis], _dev(v)) for f, axis, g, v in arrays], **spec.kw())
                    else:
                        model = _on_model_points_and_levels(spec, tabs, ax, arrays, npts)
                        h.put_dev([(f, _dev(np.where(alone, SENTINEL, plane)), 0) for f, plane, alone in model], op=spec.op,
                                  time_levels=spec.time_levels, skip=SENTINEL)
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
    assert_same(end_h, end_p, active, "the end state: hv puts against put_dev")
    assert not np.array_equal(end_h["T"][active], end_plain["T"][active]), "the puts changed nothing"
    for _, x, _, _ in made:
        x.close()


# ---------------------------------------------------------------------------
# 6. refusals, before anything is queued
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.MckppHipError
    case = lc.CASES["every_step_nz40"]
    npts, nzp1 = case.ncol, case.nz + 1
    rec, args = lc.flux_records(case), flux_args(case)
    h, kc, k3 = resident(mk, case)
    tabs = _define_grids(h, case)
    ax = _define_axes(h, kc)
    n, c7, fine = tabs[1][0], AXIS_NO["coarse7"], AXIS_NO["fine130"]
    n7 = len(ax["coarse7"])
    h.hgrid_define(2, n, tabs[1][1], None)      # no out table
    h.hgrid_define(3, n, None, tabs[1][2])      # no in table
    h.fluxes(1, *rec[0], **args)
    h.step(1, 1)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()

    def everything():
        s = _state(h, k3, kc, case.nz)
        return ([h.hgrid_info(g) for g in range(2)], {k: _bits(np.nan_to_num(v.astype(np.float64))).copy() for k, v in s.items()})

    before = everything()
    out = torch.full((n7, n), -5.0, dtype=torch.float64, device="cuda")
    good = torch.zeros((n7, n), dtype=torch.float64, device="cuda")
    pinned = torch.zeros(n * n7, dtype=torch.float64).pin_memory()
    pageable = np.zeros(n * n7)
    big, small, holds = _short_of(torch, n * 130 * 8)      # room for the model's levels and for coarse7, not for fine130
    assert holds > n * nzp1 * 8 > n * n7 * 8
    F, P = A._HvPlaneC, A._HvPutPlaneC
    fok = dict(field=A.OUT["T"], axis=c7, dtype=A.EXP_F64, grid=1, norm=0, fill_land=1, land_value=LAND, out=out.data_ptr())
    pok = dict(field=A.OUT["T"], axis=c7, dtype=A.EXP_F64, op=A.PUT_ADD, flags=0, grid=1, skip_value=0.0)

    def fetch(*planes):
        return lib.mckpp_hip_hv_fetch_dev(h._h, len(planes), (F * len(planes))(*[F(**{**fok, **p}) for p in planes]), None)

    def put(*planes):
        tab = (P * len(planes))(*[P(**{**pok, "in": good.data_ptr(), **p}) for p in planes])
        return lib.mckpp_hip_hv_put_dev(h._h, len(planes), tab, None)

    fname, pname = "mckpp_hip_hv_fetch_dev: ", "mckpp_hip_hv_put_dev: "
    table = [   # (call, message fragment)
        # what vaxis_fetch_dev refuses of the field and the axis
        (lambda: fetch(dict(field=A.OUT["wT"])), fname + "planes[0]: field 9 (wT) lives on the interface axis"),
        (lambda: fetch({}, dict(field=A.OUT["difm"])), fname + "planes[1]: field 13 (difm) lives on the interface axis"),
        (lambda: fetch(dict(field=A.OUT["hmix"])), fname + "planes[0]: field 4 (hmix) is two-dimensional"),
        (lambda: fetch(dict(field=A.OUT["solar_in"])), fname + "planes[0]: field 28 is two-dimensional"),
        (lambda: fetch(dict(field=99)), fname + "planes[0]: unknown output field 99"),
        (lambda: fetch(dict(axis=6)), fname + "planes[0]: axis 6 is not defined"),
        (lambda: fetch({}, dict(axis=-1)), fname + "planes[1]: axis -1 is not defined"),
        (lambda: fetch(dict(dtype=7)), fname + "planes[0]: dtype 7"),
        # what hgrid_fetch_dev refuses of the grid, the norm and the array
        (lambda: fetch(dict(grid=-1)), fname + "planes[0]: grid -1 is not defined"),
        (lambda: fetch(dict(grid=9)), fname + "planes[0]: grid 9 is not defined"),
        (lambda: fetch({}, dict(grid=2, out=good.data_ptr())), fname + "planes[1]: grid 2 has no out table"),
        (lambda: fetch(dict(norm=2)), fname + "planes[0]: norm 2 (MCKPP_HGRID_NORM_NONE 0, MCKPP_HGRID_NORM_USED 1)"),
        (lambda: fetch({}, dict(out=out.data_ptr() + 8 * n * (n7 - 2), axis=AXIS_NO["two"])),
         fname + "planes[1].out and planes[0].out overlap"),
        (lambda: fetch(dict(out=small, axis=fine)),
         fname + f"planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {8 * n * 130}"),
        (lambda: fetch(dict(out=pageable.ctypes.data)), fname + "planes[0].out is host memory"),
        (lambda: fetch(dict(out=pinned.data_ptr())), fname + "planes[0].out is pinned host memory"),
        (lambda: fetch(dict(out=None)), fname + "planes[0].out is null"),
        (lambda: lib.mckpp_hip_hv_fetch_dev(h._h, 65, (F * 65)(), None), fname + "nplanes=65 (0..64)"),
        (lambda: lib.mckpp_hip_hv_fetch_dev(h._h, 1, None, None), fname + "nplanes=1 (0..64) or a null table"),
        # what vaxis_put_dev refuses of the axis and the planes
        (lambda: put(dict(axis=6)), pname + "planes[0]: axis 6 is not defined"),
        (lambda: put({}, dict(field=A.OUT["u"], axis=-1)), pname + "planes[1]: axis -1 is not defined"),
        (lambda: put(dict(field=99)), pname + "planes[0]: unknown output field 99"),
        (lambda: put(dict(field=A.OUT["hmix"])), pname + "planes[0]: field 4 is an output of the step, not state"),
        (lambda: put({}, dict(field=A.OUT["rho"])), pname + "planes[1]: field 16 is an output of the step"),
        (lambda: put(dict(dtype=0)), pname + "planes[0]: dtype 0"),
        (lambda: put(dict(op=2)), pname + "planes[0]: op 2 (MCKPP_PUT_SET 0, MCKPP_PUT_ADD 1)"),
        (lambda: put(dict(flags=4)), pname + "planes[0]: flags 0x4"),
        (lambda: put(dict(flags=A.PUT_SKIP, skip_value=float("nan"))), pname + "planes[0]: the skip value is NaN"),
        (lambda: put({}, dict(axis=AXIS_NO["two"], grid=0)), pname + "planes[1] and planes[0] write the same field (2, 2)"),
        (lambda: put(dict(field=A.OUT["S_anom"]), dict(field=A.OUT["S"])), pname + "planes[1] and planes[0] write the same field (5, 3)"),
        # what remap_put_dev refuses of the grid and the array
        (lambda: put(dict(grid=7)), pname + "planes[0]: grid 7 is not defined"),
        (lambda: put({}, dict(field=A.OUT["u"], grid=3)), pname + "planes[1]: grid 3 has no in table"),
        (lambda: put({"in": pinned.data_ptr()}), pname + "planes[0].in is pinned host memory"),
        (lambda: put({}, {"field": A.OUT["u"], "in": pageable.ctypes.data}), pname + "planes[1].in is host memory"),
        (lambda: put({"in": None}), pname + "planes[0].in is null"),
        (lambda: put({"in": small, "axis": fine}),
         pname + f"planes[0].in: the allocation holds {holds} bytes from the pointer on, the call needs {8 * n * 130}"),
        (lambda: lib.mckpp_hip_hv_put_dev(h._h, 65, (P * 65)(), None), pname + "nplanes=65 (0..64)"),
        (lambda: lib.mckpp_hip_hv_put_dev(h._h, -1, (P * 1)(), None), pname + "nplanes=-1"),
        (lambda: lib.mckpp_hip_hv_put_dev(h._h, 1, None, None), pname + "nplanes=1 (0..64) or a null table"),
    ]
    for call, text in table:
        assert call() < 0, text
        assert text in err(), (text, err())
    assert fetch() == 0 and put() == 0        # no plane: nothing to do
    # no state uploaded; a grid defined for another npts
    fresh = mk.MckppHip(kc)
    fresh.vaxis_define(c7, ax["coarse7"])
    tab = (P * 1)(P(**pok, **{"in": good.data_ptr()}))
    assert lib.mckpp_hip_hv_put_dev(fresh._h, 1, tab, None) < 0 and err() == pname + "upload the state first"
    assert lib.mckpp_hip_hv_fetch_dev(fresh._h, 1, (F * 1)(F(**fok)), None) < 0 and err() == fname + "upload the state first"
    fresh.close()
    other = lc.CASES["l_rest"]
    assert other.ncol != npts and other.nz == case.nz
    g, kcg, k3g = resident(mk, other)
    g.hgrid_define(0, 5, hr.csr([[(0, 1.0)]] * other.ncol), hr.csr([[(0, 1.0)]] * 5))
    g.vaxis_define(c7, ax["coarse7"])
    g.upload(lc.hip_raw(case)[1])                # the state now has npts points, the grid was defined for other.ncol
    g.init_ocean(0)
    five = torch.zeros((n7, 5), dtype=torch.float64, device="cuda")
    tab = (P * 1)(P(**{**pok, "grid": 0, "in": five.data_ptr()}))
    assert lib.mckpp_hip_hv_put_dev(g._h, 1, tab, None) < 0
    assert err() == pname + f"planes[0]: grid 0 was defined for npts={other.ncol}, the state has {npts}: define it again", err()
    assert lib.mckpp_hip_hv_fetch_dev(g._h, 1, (F * 1)(F(**{**fok, "grid": 0, "out": five.data_ptr()})), None) < 0
    assert err() == fname + f"planes[0]: grid 0 was defined for npts={other.ncol}, the state has {npts}: define it again", err()
    g.close()
    # a multi handle checks every plane of every shard before any shard queues
    m, kcm, k3m = resident(mk, case, shards=2)
    _define_grids(m, case)
    _define_axes(m, kcm)
    m_before = {k: v.copy() for k, v in _state(m, k3m, kcm, case.nz).items()}
    tab2 = (P * 2)(P(**pok, **{"in": good.data_ptr()}), P(**{**pok, "field": A.OUT["u"], "in": pinned.data_ptr()}))
    assert lib.mckpp_hip_multi_hv_put_dev(m._h, 2, tab2, None) < 0
    assert err().startswith("mckpp_hip_multi_hv_put_dev: planes[1].in is pinned host memory"), err()
    assert lib.mckpp_hip_multi_hv_fetch_dev(m._h, 2, (F * 2)(F(**fok), F(**{**fok, "field": A.OUT["hmix"]})), None) < 0
    assert err().startswith("mckpp_hip_multi_hv_fetch_dev: planes[1]: field 4 (hmix) is two-dimensional"), err()
    assert_same(_state(m, k3m, kcm, case.nz), m_before, slice(None), "the shards after the refusals")
    m.close()
    # the Python layer's texts, and the library's through it
    with pytest.raises(ValueError, match="a host array"):
        h.hv_put_dev([("T", 1, c7, pinned.reshape(n7, n))])
    with pytest.raises(E, match=r"mckpp_hip_hv_fetch_dev: planes\[0\]: grid 2 has no out table"):
        h.hv_fetch_dev([("T", 2, c7, out)])
    after = everything()
    assert after[0] == before[0], "a refused call touched the grids"
    assert after[1].keys() == before[1].keys() and all(np.array_equal(after[1][k], before[1][k]) for k in before[1]), \
        "a refused call touched the state"
    assert (out.cpu().numpy() == -5.0).all() and not good.cpu().numpy().any()
    # ... and the run goes on: a good delivery, a good put, the next launch
    h.hv_fetch_dev([("T", 1, c7, out)], norm="used", land_value=LAND)
    assert (out.cpu().numpy() != -5.0).all()
    h.hv_put_dev([("T", 1, c7, out)], op="add", skip=LAND)
    h.fluxes(2, *rec[1], **args)
    h.step(2, 1)
    again = everything()
    assert not np.array_equal(again[1]["T"], before[1]["T"])
    h.close()
