"""Records of output schedules delivered into arrays in device memory (include/mckpp_hip_device_records.h:
mckpp_hip_records_dev and its multi_ twin).

The yardstick is mckpp_hip_window_record_fetch - existing code, itself held to the per-step API by
tests/test_window_schedule_gpu.py and tests/test_window_zoom_gpu.py - into a host array that holds the land value, or,
where fill_land is off, what the device array held.  Every comparison is of bit patterns; a float plane is compared with
numpy's float32 of the double plane (one conversion, rounded to nearest even).  The device arrays are torch tensors.

Shapes are those of the zoom tests - 60 uniform levels x 400 points, 69 stretched x 300, 100 x 250, every 7th point
land (every 3rd of the 400, so that a land list is longer than two tiles) - small on purpose: the kernel can go wrong at
edges, not at size.  A context holds four schedules, so the five kinds of schedule take two calls: the unzoomed one with
three zooms, then - the unzoomed one replaced - all four zooms."""
import numpy as np
import pytest

import common as cm
import ref_loop_cases as lc
from harness import assert_same, flux_args, loop_state, mk, resident  # noqa: F401
from test_device_arrays_gpu import _bits

pytestmark = pytest.mark.gpu

LAND = 1e20
PRE = -7.0
PERIOD, NREC = 3, 2   # a mean's division by 3 is inexact; two ring slots
SHAPES = [(60, "uniform", 400, 3), (69, "stretched", 300, 7), (100, "uniform", 250, 7)]   # levels, grid, points, land every
FIELDS = ("T", "S", "hmix", "difm")   # S adds Sref; hmix is 2-D; difm is on the interface axis


def _ops(A, gaps):
    """per field of FIELDS: with gaps, T keeps min|last (no mean) and difm mean|max; S and hmix keep all four"""
    every = A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX | A.WIN_LAST
    return (A.WIN_MIN | A.WIN_LAST, every, every, A.WIN_MEAN | A.WIN_MAX) if gaps else (every,) * 4


def _kept_ops(A, gaps, name):
    return [op for op in range(4) if (_ops(A, gaps)[FIELDS.index(name)] >> op) & 1]


def _start(mk, nz, grid, ncol, land_every, shards=0):
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, land_every=land_every)
    h = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
    h.set_forcing(k3.sflux)
    return h, kc, k3


def _zooms(kc, k3, npts):
    """name -> (points or None, (lev0, nlev) or None): every point at level 0; a shuffled third of the points, land
    among them, at levels 5..16; one point with the whole axis; the land points alone"""
    rng = np.random.default_rng(npts)
    third = rng.permutation(npts)[:npts // 3]
    land = np.nonzero(k3.run_physics == 0)[0][::-1]
    ocean = np.nonzero(k3.run_physics != 0)[0]
    assert (k3.run_physics[third] == 0).any() and (k3.run_physics[third] != 0).any() and len(land) > 0
    return {"level0": (None, (0, 1)), "third": (third, (5, 12)), "one": (ocean[len(ocean) // 2:][:1], None), "land": (land, None)}


def _want(h, A, plane, axis, prefill):
    """window_record_fetch of the plane's field and op - axis: (npoints, levels kept) - into a host array holding
    `prefill`, as the (nlev, npoints) plane the delivery writes"""
    s, rec, name, op, lev0, nlev = plane
    npoints, kept = axis
    out = np.full((npoints,) if A.OUT[name] in A._OUT_2D else (npoints, kept), prefill, order="F")
    h.window_record_fetch(s, rec, name, op, out)
    return np.ascontiguousarray(out.reshape(npoints, -1).T[lev0:lev0 + nlev])


class Run:
    """A context with schedule 0 unzoomed (ops with gaps) and schedules 1-3 the zooms level0, third (ops with gaps) and
    one; steps 1..6, record 0 released, steps 7..9: records 1 and 2 are complete, in ring slots 1 and 0.  all_zooms():
    records up to 1 released, schedule 0 replaced by the zoom `land`, steps 10..12: record 3 of schedules 1-3 (slot 1)
    and record 0 of schedule 0 are complete as well."""

    def __init__(self, mk, nz, grid, ncol, land_every, shards=0):
        A = self.A = mk.api
        self.h, self.kc, self.k3 = _start(mk, nz, grid, ncol, land_every, shards)
        self.npts, self.nzp1 = ncol, self.kc.nzp1
        self.z = _zooms(self.kc, self.k3, ncol)
        h = self.h
        self.sched = {0: ("unzoomed", True), 1: ("level0", False), 2: ("third", True), 3: ("one", False)}
        h.window_schedule(0, 1, PERIOD, NREC, FIELDS, _ops(A, True))
        for s in (1, 2, 3):
            pts, lev = self.z[self.sched[s][0]]
            h.window_schedule_zoom(s, 1, PERIOD, NREC, FIELDS, _ops(A, self.sched[s][1]), points=pts, levels=lev)
        h.step(1, 2 * PERIOD)
        for s in range(4):
            h.window_record_release(s, 0)
        h.step(2 * PERIOD + 1, PERIOD)
        for s in range(4):
            assert h.window_records(s) == (1, 2)

    def all_zooms(self):
        h = self.h
        for s in (1, 2, 3):
            h.window_record_release(s, 1)
        pts, lev = self.z["land"]
        h.window_schedule_zoom(0, 3 * PERIOD + 1, PERIOD, NREC, FIELDS, _ops(self.A, False), points=pts, levels=lev)
        self.sched[0] = ("land", False)
        h.step(3 * PERIOD + 1, PERIOD)
        assert h.window_records(0) == (0, 0) and h.window_records(2) == (2, 3)

    def axis(self, s, name):
        """(npoints, levels kept) of a plane of field `name` in schedule s"""
        pts, lev = self.z.get(self.sched[s][0], (None, None))
        two_d = self.A.OUT[name] in self.A._OUT_2D
        return (self.npts if pts is None else len(pts)), 1 if two_d else (lev[1] if lev else self.nzp1)

    def planes(self, s, recs, sub=()):
        """every kept (field, op) of schedule s in records recs, the whole kept range; sub: more (name, op, lev0, nlev)"""
        out = []
        for rec in recs:
            for name in FIELDS:
                for op in _kept_ops(self.A, self.sched[s][1], name):
                    out.append((s, rec, name, op, 0, self.axis(s, name)[1]))
            out += [(s, rec, name, op, lev0, nlev) for name, op, lev0, nlev in sub]
        return out

    def want(self, plane, prefill):
        """window_record_fetch into a host array holding `prefill`, as the (nlev, npoints) plane the delivery writes"""
        return _want(self.h, self.A, plane, self.axis(plane[0], plane[2]), prefill)

    def tensors(self, planes, dtype=np.float64, prefill=PRE):
        import torch

        tdt = torch.float64 if dtype == np.float64 else torch.float32
        return [torch.full((p[5], self.axis(p[0], p[2])[0]), prefill, dtype=tdt, device="cuda") for p in planes]

    def deliver(self, planes, outs, **kw):
        self.h.records_dev([(s, rec, name, op, o, lev0, nlev) for (s, rec, name, op, lev0, nlev), o in zip(planes, outs)],
                           land_value=LAND, **kw)

    def check(self, planes, dtype=np.float64, fill_land=True, what=""):
        """one call for all planes, each against the yardstick"""
        assert len(planes) <= 64
        outs = self.tensors(planes, dtype)
        self.deliver(planes, outs, fill_land=fill_land)
        for p, o in zip(planes, outs):
            want = self.want(p, LAND if fill_land else PRE).astype(dtype)
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), (what, p, np.dtype(dtype).name, fill_land)


def _sub(nzp1):
    """a sub-range from an offset: levels 30..69, which cross the 64-level tile, or as many as the axis has"""
    return 30, min(40, nzp1 - 30)


# ---------------------------------------------------------------------------
# 1. the unzoomed schedule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nz,grid,ncol,land_every", SHAPES)
def test_unzoomed_records_are_window_record_fetch(mk, nz, grid, ncol, land_every):
    """Records 1 and 2 of a ring of two (slots 1 and 0), period 3, ops with gaps: every kept plane over the whole axis -
    61, 70 and 101 levels, the last two across the 64-level tile - and ranges from an offset, SST among them; the
    resident columns are a multiple of neither 64 nor 256.  float64 and float32, fill_land on and off."""
    r = Run(mk, nz, grid, ncol, land_every)
    assert r.h.ncolumns % 64 and r.h.ncolumns % 256 and r.h.ncolumns < ncol
    lev0, nlev = _sub(r.nzp1)
    sub = [("S", 0, lev0, nlev), ("T", 3, lev0, nlev), ("T", 3, 0, 1), ("difm", 2, 7, 3), ("S", 2, r.nzp1 - 1, 1)]
    for rec in (2, 1):
        planes = r.planes(0, [rec], sub)
        assert {p[3] for p in planes} == {0, 1, 2, 3}
        for dtype in (np.float64, np.float32):
            for fill in (True, False):
                r.check(planes, dtype, fill, "unzoomed")
    r.h.close()


# ---------------------------------------------------------------------------
# 2. planes of different schedules, shapes and maps in one launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nz,grid,ncol,land_every", SHAPES)
def test_zoomed_and_unzoomed_planes_in_one_call(mk, nz, grid, ncol, land_every):
    """One call with planes of the unzoomed schedule and of three zooms - every point at level 0, a shuffled third at
    levels 5..16, one point with the whole axis - from records 1 and 2; then, schedule 0 replaced, one call with all
    four zooms: the list of land points has no row, so the fill alone writes, and without fill_land nothing does."""
    r = Run(mk, nz, grid, ncol, land_every)
    lev0, nlev = _sub(r.nzp1)
    first = (r.planes(1, [1]) + r.planes(2, [2, 1], [("S", 0, 3, 8), ("difm", 2, 11, 1)])
             + r.planes(3, [2], [("T", 0, lev0, nlev)]) + [(0, 1, "S", 0, 0, r.nzp1), (0, 2, "T", 3, 0, 1), (0, 2, "hmix", 1, 0, 1)])
    assert {p[0] for p in first} == {0, 1, 2, 3}
    for dtype, fill in ((np.float64, True), (np.float32, False)):
        r.check(first, dtype, fill, "unzoomed and three zooms")
    r.all_zooms()
    land = [(0, 0, "T", 0, 0, r.nzp1), (0, 0, "hmix", 3, 0, 1), (0, 0, "S", 2, lev0, nlev)]
    second = land + r.planes(1, [3]) + r.planes(2, [3, 2], [("S", 1, 11, 1)]) + r.planes(3, [3])
    for dtype, fill in ((np.float64, True), (np.float32, True), (np.float64, False)):
        r.check(second, dtype, fill, "four zooms")
    outs = r.tensors(land)   # zero rows: every element is the land value
    r.deliver(land, outs)
    assert all(bool((o == LAND).all()) for o in outs)
    r.h.close()


# ---------------------------------------------------------------------------
# 3. ordering
# ---------------------------------------------------------------------------
def test_records_dev_for_a_consumer_on_a_side_stream(mk):
    """The consumer's kernels follow the call on a side stream with no host synchronisation between; the arrays are
    rewritten on that stream before the call, which the delivery must follow."""
    import torch

    r = Run(mk, *SHAPES[0])
    planes = [(0, 2, "S", 0, 0, r.nzp1), (1, 2, "T", 0, 0, 1), (2, 1, "difm", 2, 0, 12)]
    outs = r.tensors(planes)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for o in outs:
            o.fill_(-1.0)
        r.deliver(planes, outs)
        twice = [torch.mul(o, 2.0) for o in outs]
    side.synchronize()
    for p, t in zip(planes, twice):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(r.want(p, LAND) * 2.0)), p
    r.h.close()


def test_release_and_overwrite_behind_the_delivery(mk):
    """A coupler's ring of one record: record w is delivered and released, and the steps that write record w + 1 into
    its one slot are launched at once, with no synchronisation anywhere in the loop.  The delivered arrays hold record
    w: what a second context running the same steps fetches, synchronously, before it releases.  A race test can only
    fail, never prove."""
    import torch

    ncol = SHAPES[0][2]
    A = mk.api
    names, ops, nwin = ("T", "S", "hmix"), A.WIN_MEAN | A.WIN_LAST, 5
    h, kc, _ = _start(mk, *SHAPES[0])
    ref, _, _ = _start(mk, *SHAPES[0])
    for x in (h, ref):
        x.window_schedule(0, 1, PERIOD, 1, names, ops)
    what = [("T", 0, kc.nzp1), ("S", 3, kc.nzp1), ("hmix", 0, 1), ("T", 3, 1)]
    outs = [[torch.full((nlev, ncol), PRE, dtype=torch.float64, device="cuda") for _, _, nlev in what] for _ in range(nwin)]
    torch.cuda.synchronize()
    for w in range(nwin):
        h.step(w * PERIOD + 1, PERIOD)
        h.records_dev([(0, w, name, op, o, 0, nlev) for (name, op, nlev), o in zip(what, outs[w])], land_value=LAND)
        h.window_record_release(0, w)
    h.step(nwin * PERIOD + 1, PERIOD)   # ... and the last record's slot is overwritten too
    for w in range(nwin):
        ref.step(w * PERIOD + 1, PERIOD)
        for (name, op, nlev), o in zip(what, outs[w]):
            want = _want(ref, A, (0, w, name, op, 0, nlev), (ncol, kc.nzp1), LAND)   # (an unzoomed record: the whole axis)
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), ("record", w, name, op)
        ref.window_record_release(0, w)
    h.close()
    ref.close()


# ---------------------------------------------------------------------------
# 4. refusals, before anything is queued
# ---------------------------------------------------------------------------
def _too_small(torch, need_bytes):
    """A tensor in device memory with fewer than need_bytes from its first element to the end of its allocation: the
    tail of a block that torch's allocator got from the runtime for this tensor alone (requests above 10 MiB have a
    segment of their own once nothing cached can serve them)."""
    torch.cuda.empty_cache()
    big = torch.zeros(12 << 17, dtype=torch.float64, device="cuda")   # 12 MiB
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= big.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1
    slack = seg[0]["address"] + seg[0]["total_size"] - (big.data_ptr() + big.numel() * 8)
    n = (need_bytes - 8 - slack) // 8
    assert 0 < n < big.numel(), "the allocator left more room behind the tensor than the plane needs"
    return big, big[-n:], n * 8 + slack


def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.MckppHipError
    r = Run(mk, *SHAPES[0])
    h, npts, nzp1 = r.h, r.npts, r.nzp1
    h.window_schedule(3, 1, PERIOD, NREC, (), 0)   # cancelled: a schedule that is not set
    r.sched.pop(3)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()
    P = A._DevRecordPlaneC
    good_planes = [(0, 2, "S", 0, 0, nzp1), (2, 1, "T", 3, 0, 12)]

    def state():
        return ([h.window_records(s) for s in range(3)], [_bits(r.want(p, LAND)).copy() for p in good_planes])

    before = state()
    out = torch.full((nzp1, npts), PRE, dtype=torch.float64, device="cuda")
    pinned = torch.zeros(npts * nzp1, dtype=torch.float64).pin_memory()
    pageable = np.zeros(npts * nzp1)
    big, small, holds = _too_small(torch, npts * nzp1 * 8)
    assert small.numel() < npts * nzp1
    ok = dict(sched=0, field=A.OUT["S"], op=0, lev0=0, nlev=nzp1, dtype=A.EXP_F64, fill_land=1, rec=2, land_value=LAND,
              out=out.data_ptr())

    def refused(text, k=0, **swap):
        tab = (P * (k + 1))(*([P(**ok)] * k + [P(**{**ok, **swap})]))
        assert lib.mckpp_hip_records_dev(h._h, k + 1, tab, None) == -1, text
        assert err().startswith("mckpp_hip_records_dev: ") and f"planes[{k}]" in err() and text in err(), err()

    refused("schedule 7 (0..3)", sched=7)
    refused("schedule -1 (0..3)", k=2, sched=-1)
    refused("record 3 of schedule 0 (steps 10..12) is incomplete: steps have run up to 9", k=1, rec=3)
    refused("record 0 of schedule 0 (steps 1..3) has been released", rec=0)
    refused("record -1", rec=-1)
    refused("field 0 is not in schedule 0", field=A.OUT["u"])
    refused("schedule 0 keeps no op 0 of field 2", field=A.OUT["T"])
    refused("schedule 0 keeps no op 1 of field 13", k=3, field=A.OUT["difm"], op=1)
    refused("op 4 (0 mean, 1 min, 2 max, 3 last)", op=4)
    refused("lev0=30 nlev=40 is no range of the levels schedule 0 keeps of field 5, which are 61", lev0=30, nlev=40)
    refused("lev0=0 nlev=0 is no range", nlev=0)
    refused("lev0=-1 nlev=2 is no range", lev0=-1, nlev=2)
    refused("lev0=0 nlev=13 is no range of the levels schedule 2 keeps of field 5, which are 12", sched=2, nlev=13)
    refused("lev0=1 nlev=1 is no range of the levels schedule 1 keeps of field 5, which are 1", sched=1, lev0=1, nlev=1)
    refused("lev0=0 nlev=2 is no range of the levels schedule 0 keeps of field 4, which are 1", field=A.OUT["hmix"], nlev=2)
    refused("dtype 7 (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", dtype=7)
    refused("dtype 0", k=1, dtype=0)
    refused("planes[0].out is pinned host memory", out=pinned.data_ptr())
    refused("planes[1].out is host memory", k=1, out=pageable.ctypes.data)
    refused("planes[0].out is null", out=None)
    refused(f"planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {npts * nzp1 * 8}",
            out=small.data_ptr())
    refused("schedule 3 is not set", sched=3)
    tab = (P * 65)(*[P(**ok)] * 65)
    assert lib.mckpp_hip_records_dev(h._h, 65, tab, None) == -1 and "mckpp_hip_records_dev: nplanes=65 (0..64)" in err()
    assert lib.mckpp_hip_records_dev(h._h, 1, None, None) == -1 and "mckpp_hip_records_dev: nplanes=1 (0..64) or a null table" in err()
    assert lib.mckpp_hip_records_dev(h._h, -1, tab, None) == -1 and "nplanes=-1" in err()
    # the Python layer refuses a tensor that is too small before the library is reached, and the library's texts arrive
    with pytest.raises(ValueError, match=rf"planes\[0\] out: shape \({small.numel()},\), the call takes {npts * nzp1} elements"):
        h.records_dev([(0, 2, "S", 0, small, 0, nzp1)])
    with pytest.raises(E, match=r"mckpp_hip_records_dev: planes\[1\]: record 3 of schedule 0 \(steps 10\.\.12\) is incomplete"):
        h.records_dev([(0, 2, "S", 0, out), (0, 3, "S", 0, out)])
    torch.cuda.synchronize()
    assert bool((out == PRE).all()) and bool((big == 0).all()), "a refused delivery wrote"
    after = state()
    assert after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))
    r.check(good_planes + [(1, 2, "hmix", 2, 0, 1)], what="after the refusals")   # ... and a good call follows
    assert lib.mckpp_hip_records_dev(h._h, 0, None, None) == 0   # (no plane: nothing to do)
    h.close()


# ---------------------------------------------------------------------------
# 5. both handles: two shards on the one device
# ---------------------------------------------------------------------------
def test_two_shards_deliver_the_single_contexts_planes(mk):
    """The planes of a multi handle are the single context's bit for bit, and its own window_record_fetch's: every shard
    writes its rows, shard 0 the positions no shard holds - of the grid, and of each point list - and the others none,
    so with fill_land those hold the land value, without it what the array held, and no other element does."""
    one, two = Run(mk, *SHAPES[1]), Run(mk, *SHAPES[1], shards=2)

    def both(planes, listed):
        for dtype, fill in ((np.float64, True), (np.float32, True), (np.float64, False)):
            a, b = one.tensors(planes, dtype), two.tensors(planes, dtype)
            one.deliver(planes, a, fill_land=fill)
            two.deliver(planes, b, fill_land=fill)
            for p, x, y in zip(planes, a, b):
                x, y = x.cpu().numpy(), y.cpu().numpy()
                assert np.array_equal(_bits(x), _bits(y)), (p, dtype, fill)
                pts = listed.get(p[0])
                ocean = (one.k3.run_physics != 0) if pts is None else (one.k3.run_physics[pts] != 0)
                mark = x.dtype.type(LAND) if fill else x.dtype.type(PRE)
                assert np.all(y[:, ~ocean] == mark) and not np.any(y[:, ocean] == mark), (p, dtype, fill)
        two.check(planes, what="2 shards against their own window_record_fetch")

    third, point = one.z["third"][0], one.z["one"][0]
    both([(0, 2, "S", 0, 0, one.nzp1), (0, 1, "T", 3, 0, 1), (0, 2, "hmix", 2, 0, 1), (1, 1, "T", 0, 0, 1),
          (2, 2, "difm", 0, 0, 12), (2, 1, "hmix", 3, 0, 1), (3, 2, "S", 1, 0, one.nzp1)], {2: third, 3: point})
    for r in (one, two):
        r.all_zooms()
    both([(0, 0, "T", 0, 0, one.nzp1), (0, 0, "hmix", 0, 0, 1), (2, 3, "S", 3, 2, 9), (1, 3, "hmix", 1, 0, 1)],
         {0: one.z["land"][0], 2: third})
    one.h.close()
    two.h.close()


# ---------------------------------------------------------------------------
# 6. the coupled loop on interval means
# ---------------------------------------------------------------------------
COUPLED = ("T", "u", "v", "S", "hmix", "taux_in", "nsolar_in")
K, INTERVALS = 3, 12


def _instant(h, A, npts, nzp1, name):
    """window_fetch(field, OP_INSTANT) into an array holding the land value, as the plane (nlev, npts) fetch_dev writes"""
    f = A._win_field(name)
    out = np.full((npts,) if f in A._OUT_2D else (npts, nzp1), LAND, order="F")
    h.window_fetch(f, A.OP_INSTANT, out)
    return np.ascontiguousarray(out.reshape(npts, -1).T)


def test_coupled_loop_on_interval_means(mk):
    """every_step_nz40, 12 coupling intervals of 3 steps behind a first one: the interval mean of SST - a level-0 zoomed
    schedule with a ring of one record - goes out through records_dev and is released at once; a toy atmosphere in torch,
    shf = (tair - mean sst) * 20, every arithmetic operation a torch call of its own; fluxes_dev; step(nt, 3).  Against
    the same loop through window_record_fetch, numpy and fluxes: the mean and every compared field bit for bit after
    every interval - the device loop keeps them in device arrays and holds no synchronisation until its final download."""
    import torch

    A = mk.api
    case = lc.CASES["every_step_nz40"]
    npts, nzp1, args = case.ncol, case.nz + 1, flux_args(case)
    rec = lc.flux_records(case)
    tair = 18.0 + 4.0 * np.sin(np.arange(npts) / 3.0)

    def begin(h):
        h.window_schedule_zoom(1, 1, K, 1, ("T",), A.WIN_MEAN, levels=(0, 1))
        return h

    # the host loop
    a, kca, k3a = resident(mk, case)
    begin(a).fluxes(1, *rec[0], **args)
    a.step(1, K)
    want = []
    for w in range(INTERVALS):
        sst = a.window_record_fetch(1, w, "T", A.OP_MEAN, np.full((npts, 1), LAND, order="F"))[:, 0].copy()
        a.window_record_release(1, w)
        f = list(rec[(w + 1) % len(rec)])
        f[5] = np.multiply(np.subtract(tair, sst), 20.0)
        nt = (w + 1) * K + 1
        a.fluxes(nt, *f, **args)
        a.step(nt, K)
        want.append(dict({n: _instant(a, A, npts, nzp1, n) for n in COUPLED}, mean_sst=sst[None, :]))
    a.synchronize()
    end_a = loop_state(a, k3a, kca, case.nz)
    a.close()

    # the device loop
    b, kcb, k3b = resident(mk, case)
    recd, taird = torch.from_numpy(rec).cuda(), torch.from_numpy(tair).cuda()
    kept = [dict({n: torch.empty((1 if A.OUT[n] in A._OUT_2D else nzp1, npts), dtype=torch.float64, device="cuda") for n in COUPLED},
                 mean_sst=torch.empty((1, npts), dtype=torch.float64, device="cuda")) for _ in range(INTERVALS)]
    begin(b).fluxes_dev(1, recd[0], **args)
    b.step(1, K)
    torch.cuda.synchronize()
    for w in range(INTERVALS):
        sstd = kept[w]["mean_sst"]
        b.records_dev([(1, w, "T", A.OP_MEAN, sstd)], land_value=LAND)
        b.window_record_release(1, w)
        f = [recd[(w + 1) % len(rec), m] for m in range(8)]
        f[5] = torch.mul(torch.sub(taird, sstd[0]), 20.0)
        nt = (w + 1) * K + 1
        b.fluxes_dev(nt, f, **args)
        b.step(nt, K)
        b.fetch_dev([(n, o) for n, o in kept[w].items() if n != "mean_sst"], land_value=LAND)
    b.synchronize()
    end_b = loop_state(b, k3b, kcb, case.nz)
    for w, (x, k) in enumerate(zip(want, kept)):
        for n in x:
            assert np.array_equal(_bits(k[n].cpu().numpy()), _bits(x[n])), (n, "after interval", w)
    assert_same(end_b, end_a, lc.active_columns(case), "the coupled loop's end state")
    assert not np.array_equal(_bits(want[0]["mean_sst"]), _bits(want[-1]["mean_sst"])), "the mean SST never changes"
    b.close()


