"""The device-array interface (include/mckpp_hip_device.h): forcing from arrays in device memory - at once
(mckpp_hip_fluxes_dev) and into the flux ring (mckpp_hip_flux_ring_put_dev) -, output fields into arrays in device memory
(mckpp_hip_fetch_dev), ordered on the device by events on the caller's stream (mckpp_hip_dev_fence).

The yardstick is tests/golden/ref_loop.npz, the compiled reference's own time loop (tests/ref_loop_cases.py); where a
comparison has no golden record it is against the host path of the same library - mckpp_hip_fluxes,
mckpp_hip_window_fetch(field, 3) - bit for bit.  Every comparison is an equality.  The device arrays are torch tensors
made with torch.from_numpy(...).cuda()."""
import ctypes as C

import numpy as np
import pytest

import anc_cases as ac
import ref_loop_cases as lc
from harness import assert_loop_step, assert_same, flux_args, initialised, loop_state, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401

pytestmark = pytest.mark.gpu

LAND = 1e20
PER_CALL = 2


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_golden(golden, tag, nt, h, k3, kc, what):
    h.synchronize()
    h.download(k3)
    assert_loop_step(golden, tag, nt, k3, kc, what)


def _state(h, k3, kc, nz):
    h.synchronize()
    return loop_state(h, k3, kc, nz)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---------------------------------------------------------------------------
# 1. the ring fed from device arrays, against the golden record after every call
# ---------------------------------------------------------------------------
RING_CASES = ("every_step_nz40", "l_rest", "no_flux_file", "namelist_nz69_nd2", "deep_nz100_nd4", "sweep_nd3")


def _ring_run(h, case, nslots, put, after_call):
    """Put PER_CALL records, run_forced over their steps, until the case ends; returns the calls whose records' slots wrap"""
    n, nd, wraps = lc.nrec(case), case.ndtocn, 0
    for r0 in range(0, n, PER_CALL):
        count = min(PER_CALL, n - r0)
        for r in range(r0, r0 + count):
            put(r)
        assert h.flux_ring_records() == (max(0, r0 + count - nslots), r0 + count - 1)
        wraps += r0 % nslots + count > nslots
        nt0, nt1 = r0 * nd + 1, min((r0 + count) * nd, case.nsteps)
        h.run_forced(nt0, nt1 - nt0 + 1, nd, **flux_args(case))
        after_call(nt1)
    return wraps


def test_the_ring_cases_reach_their_paths():
    assert set(RING_CASES) <= set(lc.CASES)
    assert lc.CASES["l_rest"].l_rest == 1 and not lc.CASES["no_flux_file"].flux_file
    assert lc.CASES["every_step_nz40"].land_every and lc.CASES["every_step_nz40"].calm_every
    assert lc.CASES["deep_nz100_nd4"].nz == 100 and lc.CASES["namelist_nz69_nd2"].nz == 69
    c = lc.CASES["sweep_nd3"]
    assert len(lc.active_columns(c)) % 256 and len(lc.active_columns(c)) > 256 and lc.nrec(c) >= 4   # block tails; a wrapping call


@pytest.mark.parametrize("nslots", [2, 3])
@pytest.mark.parametrize("tag", RING_CASES)
def test_golden_cases_through_the_ring_from_device_arrays(mk, golden, tag, nslots):
    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    h.flux_ring(nslots)
    assert h.flux_ring_records() == (-1, -1)
    wraps = _ring_run(h, case, nslots, lambda r: h.flux_ring_put_dev(r, recd[r]),
                      lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, f"device puts, ring of {nslots}"))
    if nslots == 3 and tag == "sweep_nd3":
        assert wraps >= 1, "no launch of the case holds records whose slots wrap"
    h.close()


@pytest.mark.parametrize("nslots", [2, 3])
def test_host_and_device_puts_alternate_in_one_ring(mk, golden, nslots):
    """Even records from the host, odd ones from device arrays handed over as eight separate arrays."""
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    rec = lc.flux_records(case)
    recd = _dev(rec)
    h, kc, k3 = resident(mk, case)
    h.flux_ring(nslots)

    def put(r):
        if r % 2:
            h.flux_ring_put_dev(r, [recd[r, m] for m in range(8)])
        else:
            h.flux_ring_put(r, rec[r])

    _ring_run(h, case, nslots, put, lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, "host and device puts"))
    h.close()


# ---------------------------------------------------------------------------
# 2. fluxes_dev is fluxes
# ---------------------------------------------------------------------------
def _intervals(case):
    for r in range(lc.nrec(case)):
        nt = r * case.ndtocn + 1
        yield r, nt, min(case.ndtocn, case.nsteps - nt + 1)


def _host_and_device_paths(mk, golden, tag, shards=0):
    """One context fed through fluxes, one through fluxes_dev (`shards` > 0: a multi handle), a launch per update
    interval: after every interval the same state bit for bit, and the golden digests."""
    case = lc.CASES[tag]
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    recd = _dev(rec)
    a, kca, k3a = resident(mk, case)
    b, kcb, k3b = resident(mk, case, shards)
    for r, nt, n in _intervals(case):
        a.fluxes(nt, *rec[r], **args)
        a.step(nt, n)
        b.fluxes_dev(nt, recd[r], **args)
        b.step(nt, n)
        want, got = _state(a, k3a, kca, case.nz), _state(b, k3b, kcb, case.nz)
        assert_same(got, want, active, f"{tag}: fluxes_dev against fluxes after step {nt + n - 1}")
        _assert_golden(golden, tag, nt + n - 1, b, k3b, kcb, "fluxes_dev")
    a.close()
    b.close()


@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_fluxes_dev_is_fluxes(mk, golden, tag):
    _host_and_device_paths(mk, golden, tag)


# ---------------------------------------------------------------------------
# 3. ordering on the device
# ---------------------------------------------------------------------------
FILL_BYTES, FILLS = 256 << 20, 12   # per record 3 GiB of fills ahead of the producer: milliseconds, a few seconds over a case


def test_fluxes_dev_waits_for_its_producer_and_the_fence_holds_the_overwrite(mk, golden):
    """The record is produced on a side stream behind FILLS fills of FILL_BYTES, fluxes_dev follows at once and the
    tensor is overwritten with NaN on that stream right after: a library that read too early sees the previous record
    (or NaN), one whose fence did not hold sees NaN, and the golden digests differ.  A race test can only fail, never
    prove: passing shows no more than that this run was ordered."""
    import torch

    tag = "every_step_nz40"
    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    side = torch.cuda.Stream()
    big = torch.empty(FILL_BYTES // 8, dtype=torch.float64, device="cuda")
    t = torch.full((8, case.ncol), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for r, nt, n in _intervals(case):
        with torch.cuda.stream(side):
            for i in range(FILLS):
                big.fill_(float(i))
            t.copy_(recd[r])
        h.fluxes_dev(nt, t, stream=side, fence=True, **flux_args(case))
        with torch.cuda.stream(side):
            t.fill_(float("nan"))
        h.step(nt, n)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "produced on a side stream, overwritten behind the fence")
    h.close()


def test_ring_put_dev_waits_for_its_producer_and_dev_fence_holds_the_overwrite(mk, golden):
    """The same for flux_ring_put_dev followed by dev_fence, two records per run_forced.  Can only fail, never prove."""
    import torch

    tag = "every_step_nz40"
    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    h.flux_ring(2)
    side = torch.cuda.Stream()
    big = torch.empty(FILL_BYTES // 8, dtype=torch.float64, device="cuda")
    t = torch.full((8, case.ncol), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def put(r):
        with torch.cuda.stream(side):
            for i in range(FILLS):
                big.fill_(float(i))
            t.copy_(recd[r])
        h.flux_ring_put_dev(r, t, stream=side)
        h.dev_fence(side)
        with torch.cuda.stream(side):
            t.fill_(float("nan"))

    _ring_run(h, case, 2, put, lambda nt: None)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "ring puts produced on a side stream")
    h.close()


# ---------------------------------------------------------------------------
# 4. fetch_dev is window_fetch(field, 3) into an array pre-filled with the land value
# ---------------------------------------------------------------------------
def _want(h, A, npts, nzp1, field, lev0, nlev, prefill=LAND):
    """window_fetch(field, OP_INSTANT) into an array holding `prefill`, as the plane (nlev, npts) fetch_dev writes"""
    f = A._win_field(field)
    out = np.full((npts,) if f in A._OUT_2D else (npts, nzp1), prefill, order="F")
    h.window_fetch(f, A.OP_INSTANT, out)
    return np.ascontiguousarray(out.reshape(npts, -1).T[lev0:lev0 + nlev])


def _fetch_and_compare(h, A, npts, nzp1, planes, dtype=np.float64, fill_land=True, prefill=-7.0, what=""):
    import torch

    tdt = torch.float64 if dtype == np.float64 else torch.float32
    outs = [torch.full((nlev, npts), prefill, dtype=tdt, device="cuda") for _, _, nlev in planes]
    h.fetch_dev([(f, o, lev0, nlev) for (f, lev0, nlev), o in zip(planes, outs)], land_value=LAND, fill_land=fill_land)
    for (f, lev0, nlev), o in zip(planes, outs):
        want = _want(h, A, npts, nzp1, f, lev0, nlev, LAND if fill_land else prefill).astype(dtype)
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), (what, f, lev0, nlev, dtype.__name__, fill_land)


@pytest.fixture(scope="module")
def stepped(mk):
    """sweep_nd3 and deep_nz100_nd4 after their first flux interval"""
    made = {}

    def get(tag):
        if tag not in made:
            case = lc.CASES[tag]
            h, kc, k3 = resident(mk, case)
            h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
            h.step(1, case.ndtocn)
            made[tag] = (h, kc, case)
        return made[tag]

    yield get
    for h, _, _ in made.values():
        h.close()


def test_fetch_dev_all_fields_in_one_call(mk):
    """All 35 output fields on an optional-physics context (the correction rows exist), 77 points of which 11 are land:
    35 planes in one launch, the two-dimensional ones through the column-per-thread path."""
    A = mk.api
    ncol, nz = 77, 40
    oc, ob, kc, k3, TS = ac.both(ncol, nz, L_RELAX_SST=1, L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1)
    h = mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    h.set_flux_series(0, ac.flux_series(ncol, 2, 31))
    h.run_forced(1, 4, 2)
    assert len(A.OUT_FIELDS) == 35 and 0 < h.ncolumns < ncol
    planes = [(f, 0, 1 if i in A._OUT_2D else nz + 1) for i, f in enumerate(A.OUT_FIELDS)]
    _fetch_and_compare(h, A, ncol, nz + 1, planes, what="35 fields")
    _fetch_and_compare(h, A, ncol, nz + 1, planes, dtype=np.float32, what="35 fields")
    h.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fill_land", [True, False])
def test_fetch_dev_paths(mk, stepped, dtype, fill_land):
    """One level and a two-dimensional field on more than 256 resident columns with a tail (the column-per-thread
    path); all 41 levels of 2000 points (point tiles with a tail, one level tile); on 101 levels the whole axis and
    levels 30..99, which cross the 64-level tile edge, the second from an offset.  float32 planes are numpy.float32 of
    the double plane; without fill_land the land points keep what the array held."""
    A = mk.api
    h, kc, case = stepped("sweep_nd3")
    assert h.ncolumns > 256 and h.ncolumns % 256 and h.ncolumns % 64 and h.ncolumns < case.ncol
    planes = [("T", 0, 1), ("hmix", 0, 1), ("u", 0, 41), ("S", 0, 41), ("v", 40, 1), ("difm", 7, 3), ("solar_in", 0, 1)]
    _fetch_and_compare(h, A, case.ncol, 41, planes, dtype, fill_land, what="sweep_nd3")
    h, kc, case = stepped("deep_nz100_nd4")
    planes = [("T", 0, 101), ("S", 30, 70), ("wT", 63, 2), ("hmix", 0, 1)]
    _fetch_and_compare(h, A, case.ncol, 101, planes, dtype, fill_land, what="deep_nz100_nd4")


def test_fetch_dev_for_a_consumer_on_a_side_stream(mk, stepped):
    """The consumer's kernels follow the call on a side stream with no host synchronisation between; the arrays are
    rewritten on that stream before the call, which the delivery must follow."""
    import torch

    A = mk.api
    h, kc, case = stepped("sweep_nd3")
    npts = case.ncol
    side = torch.cuda.Stream()
    sst = torch.empty((1, npts), dtype=torch.float64, device="cuda")
    prof = torch.empty((41, npts), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sst.fill_(-1.0)
        prof.fill_(-1.0)
        h.fetch_dev([("T", sst, 0, 1), ("T", prof, 0, 41)])
        twice = torch.mul(sst, 2.0)
        total = torch.add(prof, 1.0)
    side.synchronize()
    want = _want(h, A, npts, 41, "T", 0, 41)
    assert np.array_equal(_bits(twice.cpu().numpy()), _bits(want[0:1] * 2.0))
    assert np.array_equal(_bits(total.cpu().numpy()), _bits(want + 1.0))


# ---------------------------------------------------------------------------
# 5. refusals, before anything is queued
# ---------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(mk, golden):
    import torch

    A, E = mk.api, mk.MckppHipError
    tag = "namelist_nz69_nd2"
    case = lc.CASES[tag]
    nd, args, npts = case.ndtocn, flux_args(case), case.ncol
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case)
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()
    before = _state(h, k3, kc, case.nz)

    def ptrs(**swap):
        p = [recd[0, m].data_ptr() for m in range(8)]
        for m, v in swap.items():
            p[int(m[1:])] = v
        return (C.c_void_p * 8)(*p)

    pinned = torch.zeros(npts, dtype=torch.float64).pin_memory()
    assert lib.mckpp_hip_fluxes_dev(h._h, 1, ptrs(f5=pinned.data_ptr()), 0, lc.FLSN, lc.EL, None) < 0
    assert "mckpp_hip_fluxes_dev: fields[5] (shf) is pinned host memory" in err() and "context is on device 0" in err()
    pageable = np.zeros(npts)
    assert lib.mckpp_hip_fluxes_dev(h._h, 1, ptrs(f0=pageable.ctypes.data), 0, lc.FLSN, lc.EL, None) < 0
    assert "fields[0] (taux) is host memory" in err() and "context is on device 0" in err()
    assert lib.mckpp_hip_fluxes_dev(h._h, 1, ptrs(f2=None), 0, lc.FLSN, lc.EL, None) < 0
    assert "fields[2] (swf) is null" in err() and "context is on device 0" in err()
    with pytest.raises(E, match="mckpp_hip_flux_ring_put_dev: no flux ring is set"):      # a put with no ring
        h.flux_ring_put_dev(0, recd[0])
    h.flux_ring(2)
    assert lib.mckpp_hip_flux_ring_put_dev(h._h, 0, ptrs(f7=pinned.data_ptr()), None) < 0
    assert "mckpp_hip_flux_ring_put_dev: fields[7] (snow) is pinned host memory" in err()
    assert h.flux_ring_records() == (-1, -1), "a refused put counts as put"
    h.flux_ring_put_dev(0, recd[0])
    with pytest.raises(E, match=r"mckpp_hip_flux_ring_put_dev: record 3, but the records arrive in order: the next one is record 1"):
        h.flux_ring_put_dev(3, recd[3])                                                  # a put out of order
    with pytest.raises(E, match=r"record 0, but the records arrive in order: the next one is record 1"):
        h.flux_ring_put_dev(0, recd[0])
    assert h.flux_ring_records() == (0, 0)
    # planes: a diagnostic-axis range of no level, a correction field without its rows, a host array, an unknown dtype
    out = torch.full((1, npts), -7.0, dtype=torch.float64, device="cuda")
    plane = (A._DevPlaneC * 1)(A._DevPlaneC(A.OUT["difm"], 0, 0, A.EXP_F64, 1, LAND, out.data_ptr()))
    assert lib.mckpp_hip_fetch_dev(h._h, 1, plane, None) < 0
    assert "mckpp_hip_fetch_dev: planes[0]: lev0=0 nlev=0 is no range of levels of field 13, whose axis has 70" in err()
    with pytest.raises(E, match="field 18 needs the correction rows"):                  # scorr on default physics
        h.fetch_dev([("T", out, 0, 1), ("scorr", out, 0, 1)])
    plane[0] = A._DevPlaneC(A.OUT["T"], 0, 1, A.EXP_F64, 1, LAND, pinned.data_ptr())
    assert lib.mckpp_hip_fetch_dev(h._h, 1, plane, None) < 0 and "planes[0].out is pinned host memory" in err()
    plane[0] = A._DevPlaneC(A.OUT["T"], 0, 1, 7, 1, LAND, out.data_ptr())
    assert lib.mckpp_hip_fetch_dev(h._h, 1, plane, None) < 0 and "planes[0]: dtype 7" in err()
    plane[0] = A._DevPlaneC(99, 0, 1, A.EXP_F64, 1, LAND, out.data_ptr())
    assert lib.mckpp_hip_fetch_dev(h._h, 1, plane, None) < 0 and "unknown output field 99" in err()
    assert np.array_equal(out.cpu().numpy(), np.full((1, npts), -7.0)), "a refused delivery wrote"
    assert_same(_state(h, k3, kc, case.nz), before, slice(None), "after the refusals")
    # ... and good calls then end in the golden state
    for r in range(1, lc.nrec(case)):
        h.flux_ring_put_dev(r, recd[r])
        if r % 2:
            h.run_forced((r - 1) * nd + 1, 2 * nd, nd, **args)
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "after the refusals")
    h.close()


# ---------------------------------------------------------------------------
# 6. both handles: two shards on the one device
# ---------------------------------------------------------------------------
def test_two_shards_ring_from_device_arrays(mk, golden):
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    recd = _dev(lc.flux_records(case))
    h, kc, k3 = resident(mk, case, shards=2)
    h.flux_ring(3)
    wraps = _ring_run(h, case, 3, lambda r: h.flux_ring_put_dev(r, recd[r]),
                      lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, "2 shards, device puts"))
    assert wraps >= 1
    h.close()


@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3"])
def test_two_shards_fluxes_dev_is_fluxes(mk, golden, tag):
    _host_and_device_paths(mk, golden, tag, shards=2)


def test_two_shards_fetch_dev(mk, stepped):
    """The planes of a multi handle are those of the single context bit for bit; with fill_land every land point holds the
    land value and no ocean point does (shard 0 fills the points no shard holds, shard 1 none); without it the land
    points keep what the array held."""
    import torch

    A = mk.api
    one, kc, case = stepped("sweep_nd3")
    m, kcm, k3m = resident(mk, case, shards=2)
    m.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    m.step(1, case.ndtocn)
    npts, ocean = case.ncol, lc.ocean(case).astype(bool)
    planes = [("T", 0, 1), ("hmix", 0, 1), ("u", 0, 41), ("S", 3, 30), ("wT", 0, 41)]
    for dtype, fill in [(torch.float64, True), (torch.float32, True), (torch.float64, False)]:
        outs = {}
        for name, h in (("one", one), ("multi", m)):
            outs[name] = [torch.full((nlev, npts), -7.0, dtype=dtype, device="cuda") for _, _, nlev in planes]
            h.fetch_dev([(f, o, lev0, nlev) for (f, lev0, nlev), o in zip(planes, outs[name])], land_value=LAND, fill_land=fill)
        for p, a, b in zip(planes, outs["one"], outs["multi"]):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(_bits(a), _bits(b)), (p, dtype, fill)
            assert np.all(b[:, ~ocean] == (a.dtype.type(LAND) if fill else -7.0)), (p, dtype, fill, "land points")
            assert not np.any(b[:, ocean] == a.dtype.type(LAND)) and not np.any(b[:, ocean] == -7.0), (p, "ocean points")
    _fetch_and_compare(m, A, npts, 41, planes, what="2 shards against their own window_fetch")
    m.close()


def _alone(mk, m, d):
    """Shard d of the multi handle m as a context of its own (mckpp_hip_multi_ctx): m's records of its schedules and
    grids, the shard's handle.  The multi handle owns the context: drop the wrapper with _let_go, never close it."""
    one = mk.MckppHip.__new__(mk.MckppHip)
    one.__dict__.update(m.__dict__)
    one._h = C.c_void_p(mk.api._lib().mckpp_hip_multi_ctx(m._h, d))
    assert one._h
    return one


def _let_go(one):
    one._h = C.c_void_p()


def test_a_shard_addressed_alone_between_two_multi_calls(mk):
    """A multi call that fills the points no shard holds leaves shard 0 with the lists and out tables of the union of the
    shards' columns.  The same call on shard 0's own handle then delivers what a context of its own with shard 0's
    run_physics mask delivers, bit for bit - shard 1's points are land to it -, and the multi call after it delivers what
    the first did: fetch_dev, records_dev on a listed and on an unlisted schedule, hgrid_fetch_dev, and records_reduce_dev
    with axis-only planes, all filling."""
    import torch

    import hgrid_ref as hr

    A = mk.api
    case = lc.CASES["sweep_nd3"]
    npts, nd, ocean = case.ncol, case.ndtocn, lc.ocean(case)
    n = hr.grids(npts)[1]
    tout = hr.general_out(n, npts, ocean, 17)
    pts = np.random.default_rng(5).permutation(npts)[:300]
    NL = 9   # the levels the listed schedule keeps

    def start(h):
        h.hgrid_define(0, n, None, tout)
        h.window_schedule_zoom(1, 1, nd, 2, ("T", "hmix"), A.WIN_MEAN | A.WIN_LAST, points=pts, levels=(2, NL))
        h.window_schedule(2, 1, nd, 2, ("S",), A.WIN_LAST)
        h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
        h.step(1, nd)

    def outs(*shapes):
        return [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in shapes]

    def fetch(h):
        o = outs((1, npts), (41, npts), (1, npts))
        h.fetch_dev([("T", o[0], 0, 1), ("u", o[1], 0, 41), ("hmix", o[2], 0, 1)], land_value=LAND, fill_land=True)
        return o

    def records(h):
        o = outs((NL, len(pts)), (1, len(pts)), (41, npts))
        h.records_dev([(1, 0, "T", A.OP_MEAN, o[0]), (1, 0, "hmix", A.OP_LAST, o[1]), (2, 0, "S", A.OP_LAST, o[2])],
                      land_value=LAND, fill_land=True)
        return o

    def hgrid(h):
        o = outs((3, n), (1, n))
        h.hgrid_fetch_dev([("T", 0, o[0], 0, 3), ("hmix", 0, o[1])], norm="used", land_value=LAND, fill_land=True)
        return o

    def reduce(h):
        o = outs((len(pts),), (npts,))
        h.records_reduce_dev([(1, 0, "T", A.OP_MEAN, o[0], "sum", "none"), (2, 0, "S", A.OP_LAST, o[1], "max", "none")],
                             land_value=LAND)
        return o

    def got(call, h):
        return [_bits(o.cpu().numpy()) for o in call(h)]

    m, kcm, k3m = resident(mk, case, shards=2)
    start(m)
    mask0, n0 = A.host_shard_mask(k3m.run_physics, 2, 0)
    assert 0 < n0 < len(lc.active_columns(case)), "both shards hold columns"
    kc, k3 = lc.hip_raw(case)
    k3.run_physics[:] = mask0
    fresh = initialised(mk, kc, k3)
    start(fresh)
    shard0 = _alone(mk, m, 0)
    try:
        for call in (fetch, records, hgrid, reduce):
            first = got(call, m)
            alone = got(call, shard0)
            again = got(call, m)
            want = got(call, fresh)
            for k, (f, a, g, w) in enumerate(zip(first, alone, again, want)):
                assert np.array_equal(a, w), (call.__name__, k, "shard 0 alone against a context with its mask")
                assert np.array_equal(g, f), (call.__name__, k, "the multi call after against the one before")
                assert not np.array_equal(a, f), (call.__name__, k, "shard 0 alone delivers what both shards do")
    finally:
        _let_go(shard0)
    fresh.close()
    m.close()


# ---------------------------------------------------------------------------
# 7. the coupled loop
# ---------------------------------------------------------------------------
COUPLED = ("T", "u", "v", "S", "hmix", "taux_in", "solar_in", "nsolar_in", "PminusE_in")


@pytest.mark.parametrize("shards", [0, 2])
def test_coupled_loop_on_the_device(mk, shards):
    """every_step_nz40, 12 intervals of one step: SST out through fetch_dev, a toy atmosphere in torch - sensible heat
    shf = (tair - sst) * 20, every arithmetic operation a torch call of its own, so nothing contracts into an FMA -,
    the other seven fields from the case's records, fluxes_dev, step.  Against the same loop through window_fetch, numpy
    and fluxes: every compared field bit for bit after every interval - the device loop keeps them in device arrays, for
    it holds no synchronisation until its final download."""
    import torch

    A = mk.api
    case = lc.CASES["every_step_nz40"]
    npts, nzp1, args = case.ncol, case.nz + 1, flux_args(case)
    rec = lc.flux_records(case)
    tair = 18.0 + 4.0 * np.sin(np.arange(npts) / 3.0)
    n2d = [f for f in COUPLED if A.OUT[f] in A._OUT_2D]

    # the host loop
    a, kca, k3a = resident(mk, case)
    want = []
    for nt in range(1, case.nsteps + 1):
        sst = _want(a, A, npts, nzp1, "T", 0, 1)[0]
        f = list(rec[nt - 1])
        f[5] = np.multiply(np.subtract(tair, sst), 20.0)
        a.fluxes(nt, *f, **args)
        a.step(nt, 1)
        want.append({n: _want(a, A, npts, nzp1, n, 0, 1 if n in n2d else nzp1) for n in COUPLED})
    end_a = _state(a, k3a, kca, case.nz)
    a.close()

    # the device loop
    b, kcb, k3b = resident(mk, case, shards)
    recd, taird = _dev(rec), _dev(tair)
    sstd = torch.empty((1, npts), dtype=torch.float64, device="cuda")
    kept = [{n: torch.empty((1 if n in n2d else nzp1, npts), dtype=torch.float64, device="cuda") for n in COUPLED}
            for _ in range(case.nsteps)]
    torch.cuda.synchronize()
    for nt in range(1, case.nsteps + 1):
        b.fetch_dev([("T", sstd, 0, 1)], land_value=LAND)
        shf = torch.mul(torch.sub(taird, sstd[0]), 20.0)
        f = [recd[nt - 1, m] for m in range(8)]
        f[5] = shf
        b.fluxes_dev(nt, f, **args)
        b.step(nt, 1)
        b.fetch_dev([(n, o) for n, o in kept[nt - 1].items()], land_value=LAND)
    end_b = _state(b, k3b, kcb, case.nz)
    for nt, (w, k) in enumerate(zip(want, kept), 1):
        for n in COUPLED:
            assert np.array_equal(_bits(k[n].cpu().numpy()), _bits(w[n])), (n, "after interval", nt)
    assert_same(end_b, end_a, lc.active_columns(case), "the coupled loop's end state")
    assert not np.array_equal(end_a["T"], _unforced_T(mk, case)), "the toy atmosphere changes nothing"
    b.close()


def _unforced_T(mk, case):
    """T after the case's steps under its own records: what the coupled loop must differ from"""
    h, kc, k3 = resident(mk, case)
    h.set_flux_series(0, lc.flux_records(case))
    h.run_forced(1, case.nsteps, case.ndtocn, **flux_args(case))
    out = _state(h, k3, kc, case.nz)["T"]
    h.close()
    return out
