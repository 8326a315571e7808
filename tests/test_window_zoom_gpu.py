"""Output schedules over chosen points and levels (mckpp_hip_window_schedule_zoom): records, export slots and fetches
sized to a list of points and a range of levels.  The oracle of a zoomed record is the unzoomed schedule of the same
fields, operations, origin and period in the same launch of the same context, restricted with numpy to the points and
levels - the unzoomed schedule itself is held to the per-step API by tests/test_window_schedule_gpu.py.  Everything is
compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401
from harness import shape as _shape

pytestmark = pytest.mark.gpu

FIELDS = ("T", "S", "hmix", "difm", "wT", "rho")   # S adds Sref; hmix is 2-D; difm and wT are on the interface axis
FILL = -7.0
ENV = ("MCKPP_PS", "MCKPP_XCC_DROP", "MCKPP_SOLVER_MODE", "MCKPP_SOLO_LIMIT", "MCKPP_MULTISTEP")


def _all_ops(A):
    return A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX | A.WIN_LAST


def _cut(kc, name, a, lev0=0):
    """level nzp1 of Rig and Shsq is never written by the model (the _cut of test_window_schedule_gpu.py, for a plane
    that begins at level lev0)"""
    return a[:, :max(kc.nz - lev0, 0)] if name in ("Rig", "Shsq") else a


def _ld_out(nlev):
    return 1 if nlev == 1 else (nlev + 7) // 8 * 8


def _start(mk, ncol, nz, grid="uniform", land_every=7, nsteps=12, forced=True, shards=0):
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, land_every=land_every)
    h = mk.MckppHip(kc) if shards == 0 else mk.MckppHipMulti(kc, [0] * shards)
    h.upload(k3)
    h.init_ocean(0)
    if forced:
        h.set_flux_series(0, cm.synth.flux_series(ncol, 1, nsteps, kc.dto))
    else:
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        h.set_forcing(k3.sflux)
    return h, kc, k3


def _zooms(kc, npts):
    """the four zooms: (points or None, (lev0, nlev) or None)"""
    rng = np.random.default_rng(npts)
    third = rng.permutation(npts)[:npts // 3]
    assert (third % 7 == 0).any()   # land among them
    ending = np.concatenate([rng.permutation(npts - 1)[:10], [npts - 1]])
    return [(None, (0, 1)), (third, (5, 12)), (np.array([npts // 2 + 1]), None), (ending, (kc.nzp1 - 3, 3))]


def _fetch_zoomed(h, kc, s, rec, name, op, npoints, nlev, fill=FILL, dtype=np.float64, export=False):
    shape = (npoints,) if len(_shape(kc, 1, name)) == 1 else (npoints, nlev)
    out = np.full(shape, fill, dtype=dtype, order="F")
    (h.window_export_fetch if export else h.window_record_fetch)(s, rec, name, op, out)
    return out


def _restricted(kc, full, name, pts, lev):
    """the plane of an unzoomed record at the points and levels of a zoom"""
    p = np.arange(full.shape[0]) if pts is None else np.asarray(pts)
    if full.ndim == 1:
        return full[p]
    lev0, nlev = lev if lev is not None else (0, kc.nzp1)
    return full[p][:, lev0:lev0 + nlev]


def _compare(h, kc, npts, unzoomed, zoomed, recs, fields=FIELDS, ops=(0, 1, 2, 3), cache=None):
    """zoomed: {schedule: (points, levels)}; every plane of every record against schedule `unzoomed` restricted"""
    cache = {} if cache is None else cache
    n = 0
    for rec in recs:
        for name in fields:
            for op in ops:
                if (rec, name, op) not in cache:
                    cache[rec, name, op] = h.window_record_fetch(unzoomed, rec, name, op,
                                                                 np.full(_shape(kc, npts, name), FILL, order="F")).copy()
                full = cache[rec, name, op]
                for s, (pts, lev) in zoomed.items():
                    npoints = npts if pts is None else len(pts)
                    lev0, nlev = lev if lev is not None else (0, kc.nzp1)
                    got = _fetch_zoomed(h, kc, s, rec, name, op, npoints, nlev)
                    want = _restricted(kc, full, name, pts, lev)
                    assert got.shape == want.shape
                    assert np.array_equal(_cut(kc, name, got, lev0), _cut(kc, name, want, lev0)), (s, rec, name, op)
                    n += 1
    return n


def _ring_bytes(kc, k3, pts, lev, nrec, nops, fields=FIELDS):
    ocean = k3.run_physics != 0
    rows = int(ocean.sum()) if pts is None else int(ocean[np.asarray(pts)].sum())
    nlev = lev[1] if lev is not None else kc.nzp1
    return sum(nrec * nops * rows * (1 if len(_shape(kc, 1, f)) == 1 else _ld_out(nlev)) * 8 for f in fields)


@pytest.mark.parametrize("nz,grid,ncol", [(60, "uniform", 400), (69, "stretched", 300), (100, "uniform", 250)])
def test_zoomed_records_equal_the_unzoomed_restricted(mk, nz, grid, ncol):
    """12 steps in one run_forced, land every 7th point: schedule 0 unzoomed, schedules 1-3 zoomed, mean, min, max and
    last of six fields every 4 steps.  The four zooms - every point at level 0; a shuffled third of the points, land
    included, levels 5..16; one point with the whole axis; a list ending at the last point with the last three levels -
    take two runs of three zoomed schedules (the fourth zoom with the first two again)."""
    A = mk.api
    for group in ((0, 1, 2), (3, 0, 1)):
        h, kc, k3 = _start(mk, ncol, nz, grid)
        zs = _zooms(kc, ncol)
        h.window_schedule(0, 1, 4, 3, FIELDS, _all_ops(A))
        zoomed = {}
        for s, z in zip((1, 2, 3), group):
            pts, lev = zs[z]
            h.window_schedule_zoom(s, 1, 4, 3, FIELDS, _all_ops(A), points=pts, levels=lev)
            zoomed[s] = (pts, lev)
            npoints, lev0, nlev, rb = h.window_zoom(s)
            assert (npoints, lev0, nlev) == (ncol if pts is None else len(pts), *(lev if lev is not None else (0, kc.nzp1)))
            assert rb == _ring_bytes(kc, k3, pts, lev, 3, 4)
        npoints, lev0, nlev, rb = h.window_zoom(0)   # an unzoomed schedule: the rows of the state
        assert (npoints, lev0, nlev) == (ncol, 0, kc.nzp1)
        ld = 64 * ((kc.nzp1 + 2 + 63) // 64)   # the rows of the state (DESIGN, data layout)
        assert rb == sum(3 * 4 * int((k3.run_physics != 0).sum()) * (1 if f == "hmix" else ld) * 8 for f in FIELDS)
        h.run_forced(1, 12, 1)
        for s in range(4):
            assert h.window_records(s) == (0, 2)
        assert _compare(h, kc, ncol, 0, zoomed, range(3)) == 3 * 6 * 4 * 3
        h.close()


def test_station_series_equals_the_instantaneous_fields_step_by_step(mk):
    """Every step's profile at five points: period 1, "last", 24 steps in one step(1, 24), against a second context
    stepped one launch at a time with window_fetch(field, OP_INSTANT) after each step, read at those points."""
    A = mk.api
    ncol, nz, nsteps = 300, 60, 24
    pts = np.array([299, 14, 1, 150, 77])   # (14 and 77 are land)
    names = ("T", "S", "hmix", "u")
    h, kc, k3 = _start(mk, ncol, nz, forced=False)
    h.window_schedule_zoom(1, 1, 1, nsteps, names, A.WIN_LAST, points=pts)
    h.step(1, nsteps)
    assert h.window_records(1) == (0, nsteps - 1)
    r, _, _ = _start(mk, ncol, nz, forced=False)
    for nt in range(1, nsteps + 1):
        r.step(nt, 1)
        for n in names:
            full = r.window_fetch(A.OUT[n], A.OP_INSTANT, np.full(_shape(kc, ncol, n), FILL, order="F"))
            got = _fetch_zoomed(h, kc, 1, nt - 1, n, A.OP_LAST, len(pts), kc.nzp1)
            assert np.array_equal(got, full[pts]), (nt, n)
    h.close()
    r.close()


@pytest.mark.parametrize("ncol,nz,nsteps,env", [(64, 100, 12, {}), (300, 60, 10, {"MCKPP_XCC_DROP": "0x55"}),
                                                 (64, 60, 12, {"MCKPP_PS": "15x8x2"})])
def test_lagging_columns_keep_their_zoomed_windows_in_order(mk, monkeypatch, ncol, nz, nsteps, env):
    """The workloads of test_lagging_columns_finish_their_windows_in_order (fewer columns than slots, many columns at
    itermax, columns windows apart): a zoomed schedule against an unzoomed one in the same launch."""
    A = mk.api
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fields = ("T", "hmix", "difm", "Rig")
    h, kc, k3 = _start(mk, ncol, nz, land_every=9, forced=False)
    pts = np.random.default_rng(5).permutation(ncol)[:ncol // 3]
    h.window_schedule(0, 1, 3, 4, fields, _all_ops(A))
    h.window_schedule_zoom(1, 1, 3, 4, fields, _all_ops(A), points=pts, levels=(5, 12))
    h.window_schedule_zoom(2, 1, 3, 4, fields, _all_ops(A), levels=(nz - 4, 5))   # (up to the level Rig never writes)
    h.step(1, nsteps)
    recs = range(nsteps // 3)
    assert h.window_records(1) == (0, nsteps // 3 - 1)
    _compare(h, kc, ncol, 0, {1: (pts, (5, 12)), 2: (None, (nz - 4, 5))}, recs, fields=fields)
    h.close()


@pytest.mark.parametrize("env", [{}, {"MCKPP_MULTISTEP": "0"}])
def test_steps_in_two_calls_and_a_launch_per_step(mk, monkeypatch, env):
    """Steps 1..5 and 6..12 in two calls - a record begun in one is completed in the next - as one launch per call, and
    as a launch per step (MCKPP_MULTISTEP=0)."""
    A = mk.api
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ncol, nz = 300, 60
    h, kc, k3 = _start(mk, ncol, nz, land_every=6, forced=False)
    pts = np.random.default_rng(11).permutation(ncol)[:100]
    h.window_schedule(0, 1, 4, 3, FIELDS, _all_ops(A))
    h.window_schedule_zoom(1, 1, 4, 3, FIELDS, _all_ops(A), points=pts, levels=(5, 12))
    h.step(1, 5)
    assert h.window_records(1) == (0, 0)
    h.step(6, 7)
    assert h.window_records(1) == (0, 2)
    _compare(h, kc, ncol, 0, {1: (pts, (5, 12))}, range(3))
    h.close()


def _check_export(A, h, kc, s, recs, npoints, nlev, dtype, land, fields=FIELDS, ops=(0, 1, 2, 3)):
    """the export of zoomed schedule `s` against window_record_fetch into arrays pre-filled with land (narrowed for f4);
    returns the planes of the whole-record fetches, by record (the padding between planes is nobody's)"""
    np_t, bits = {"f8": (np.float64, np.uint64), "f4": (np.float32, np.uint32)}[dtype]
    planes, record_bytes = h.window_export_layout(s)
    two_d = [len(_shape(kc, 1, name)) == 1 for name in fields]
    assert [(f, op) for f, op, _, _ in planes] == [(A.OUT[name], op) for name in fields for op in ops]
    assert [nl for _, _, nl, _ in planes] == [1 if t else nlev for t in two_d for _ in ops]
    assert all(off % 256 == 0 for _, _, _, off in planes) and record_bytes % 256 == 0
    size = np.dtype(np_t).itemsize
    for (_, _, nl, off), nxt in zip(planes, [p[3] for p in planes[1:]] + [record_bytes]):
        assert off + npoints * nl * size <= nxt < off + npoints * nl * size + 256
    whole = {}
    for rec in recs:
        record = h.window_export_fetch_record(s, rec, np.zeros(record_bytes // size, dtype=np_t))
        whole[rec] = []
        k = 0
        for name in fields:
            for op in ops:
                want = _fetch_zoomed(h, kc, s, rec, name, op, npoints, nlev, fill=land).astype(np_t, order="F")
                got = _fetch_zoomed(h, kc, s, rec, name, op, npoints, nlev, fill=0, dtype=np_t, export=True)
                assert np.array_equal(got.view(bits), want.view(bits)), (rec, name, op)
                _, _, nl, off = planes[k]
                part = record[off // size: off // size + npoints * nl]
                assert np.array_equal(part.view(bits), want.ravel(order="F").view(bits)), (rec, name, op, "record")
                whole[rec].append(part.copy())
                k += 1
    return whole


@pytest.mark.parametrize("dtype", ["f8", "f4"])
def test_export_of_a_zoomed_schedule(mk, dtype):
    """window_export on zoomed schedules: the layout has the zoomed nlev and offsets that are multiples of 256; a plane
    equals window_record_fetch into an array pre-filled with land_value (narrowed for "f4"); the whole record agrees
    with the layout.  130 listed points, land among them (rows that are no multiple of the 64-row tile), 12 levels; and every
    point at one level (the column-per-thread path)."""
    A = mk.api
    ncol, nz = 300, 69
    h, kc, k3 = _start(mk, ncol, nz, grid="stretched")
    pts = np.random.default_rng(3).permutation(ncol)[:130]
    h.window_schedule_zoom(1, 1, 4, 3, FIELDS, _all_ops(A), points=pts, levels=(5, 12))
    h.window_schedule_zoom(2, 1, 4, 3, FIELDS, _all_ops(A), levels=(0, 1))
    h.window_export(1, dtype, 1e20)
    h.window_export(2, dtype, -3.5)
    h.run_forced(1, 12, 1)
    _check_export(A, h, kc, 1, range(3), 130, 12, dtype, 1e20)
    _check_export(A, h, kc, 2, range(3), ncol, 1, dtype, -3.5)
    h.close()


def test_three_shards_equal_the_single_context(mk):
    """Three shards on device 0 behind the multi handle: records and export planes equal the single context's, and the
    shards' ring_bytes add up to its figure."""
    A = mk.api
    ncol, nz, nsteps = 301, 69, 8
    pts = np.random.default_rng(7).permutation(ncol)[:100]
    outs = []
    for shards in (0, 3):
        h, kc, k3 = _start(mk, ncol, nz, grid="stretched", land_every=6, nsteps=nsteps, shards=shards)
        h.window_schedule_zoom(1, 1, 4, 2, FIELDS, _all_ops(A), points=pts, levels=(5, 12))
        h.window_schedule_zoom(2, 1, 4, 2, FIELDS, _all_ops(A), levels=(0, 1))
        h.window_export(1, "f4", 1e20)
        h.window_export(2, "f8", 1e20)
        h.run_forced(1, nsteps, 1)
        got = {"zoom": (h.window_zoom(1), h.window_zoom(2))}
        got["exp1"] = _check_export(A, h, kc, 1, range(2), 100, 12, "f4", 1e20)
        got["exp2"] = _check_export(A, h, kc, 2, range(2), ncol, 1, "f8", 1e20)
        for s, npoints, nlev in ((1, 100, 12), (2, ncol, 1)):
            for rec in range(2):
                for name in FIELDS:
                    for op in range(4):
                        got[s, rec, name, op] = _fetch_zoomed(h, kc, s, rec, name, op, npoints, nlev)
        if shards:
            per = [mk.api._lib().mckpp_hip_multi_ctx(h._h, d) for d in range(shards)]
            rb = []
            for x in per:
                b = C.c_int64()
                assert mk.api._lib().mckpp_hip_window_zoom(x, 1, None, None, None, C.byref(b)) == 0
                rb.append(b.value)
            assert sum(rb) == got["zoom"][0][3] and all(b > 0 for b in rb)
        h.close()
        outs.append(got)
    a, b = outs
    assert a.keys() == b.keys()
    assert a["zoom"] == b["zoom"] and a["zoom"][0][3] == _ring_bytes(kc, k3, pts, (5, 12), 2, 4)
    for key in a:
        if key == "zoom":
            continue
        if isinstance(key, str):
            for rec in a[key]:
                for pa, pb in zip(a[key][rec], b[key][rec]):
                    assert np.array_equal(pa.view(np.uint8), pb.view(np.uint8)), (key, rec)
        else:
            assert np.array_equal(a[key], b[key]), key


def test_a_refused_zoom_leaves_the_schedule_in_place(mk):
    """A duplicate point, a point equal to npts, lev0 + nlev > nzp1, a negative nlev and npoints = 0 with a list: each an
    error by name at the library (the wrapper refuses them before it), and afterwards the schedule that was in place
    still fetches its records."""
    A = mk.api
    ncol, nz = 200, 60
    h, kc, k3 = _start(mk, ncol, nz, land_every=5, forced=False)
    pts = np.array([3, 199, 17, 0, 42])
    h.window_schedule_zoom(1, 1, 2, 4, ("T", "hmix"), A.WIN_LAST | A.WIN_MEAN, points=pts, levels=(2, 9))
    h.step(1, 4)
    before = {(rec, n): _fetch_zoomed(h, kc, 1, rec, n, A.OP_MEAN, 5, 9) for rec in (0, 1) for n in ("T", "hmix")}
    lib = A._lib()
    f = np.array([A.OUT["T"]], dtype=np.int32)
    o = np.array([A.WIN_LAST], dtype=np.uint32)

    def refused(points, npoints, lev0, nlev, text):
        p = None if points is None else np.ascontiguousarray(points, dtype=np.int32)
        z = A._WinZoomC(None if p is None else p.ctypes.data_as(C.POINTER(C.c_int32)), npoints, lev0, nlev)
        rc = lib.mckpp_hip_window_schedule_zoom(h._h, 1, 1, 2, 4, f.ctypes.data_as(C.POINTER(C.c_int32)),
                                                o.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(z))
        assert rc != 0
        msg = lib.mckpp_hip_last_error().decode()
        assert msg.startswith("mckpp_hip_window_schedule_zoom: zoom: ") and text in msg, msg

    refused([5, 9, 11, 9], 4, 0, 0, "point 9 twice, at positions 1 and 3")
    refused([5, ncol], 2, 0, 0, f"point {ncol} at position 1 is outside 0..{ncol - 1}")
    refused(None, 0, 50, 12, "levels lev0=50 nlev=12")
    refused(None, 0, 3, -1, "levels lev0=3 nlev=-1")
    refused([5, 9], 0, 0, 0, "npoints=0 with a point list")
    for bad in (dict(points=[5, 9, 11, 9]), dict(points=[5, ncol]), dict(levels=(50, 12)), dict(levels=(3, -1)), dict(points=[])):
        with pytest.raises(ValueError, match="zoom: "):
            h.window_schedule_zoom(1, 1, 2, 4, ("T",), A.WIN_LAST, **bad)
    with pytest.raises(ValueError, match=r"is zoomed: a plane of T is out\(5, 9\)"):
        h.window_record_fetch(1, 0, "T", A.OP_MEAN, np.zeros((ncol, kc.nzp1), order="F"))
    assert h.window_zoom(1)[:3] == (5, 2, 9)
    for (rec, n), want in before.items():
        assert np.array_equal(_fetch_zoomed(h, kc, 1, rec, n, A.OP_MEAN, 5, 9), want), (rec, n)
    h.step(5, 2)   # ... and goes on
    assert h.window_records(1) == (0, 2)
    h.close()


def test_a_zoom_of_land_points_only_writes_nothing(mk):
    """A zoom that lists only land points is accepted; every fetch - a record's plane, the export's - leaves `out` as it
    was (the export: at land_value)."""
    A = mk.api
    ncol, nz = 200, 60
    h, kc, k3 = _start(mk, ncol, nz, forced=False)
    pts = np.array([14, 0, 196])
    assert not k3.run_physics[pts].any()
    h.window_schedule_zoom(1, 1, 2, 2, ("T", "hmix"), A.WIN_LAST | A.WIN_MEAN, points=pts, levels=(0, 4))
    h.window_export(1, "f8", 1e20)
    assert h.window_zoom(1) == (3, 0, 4, 0)
    h.step(1, 4)
    for n in ("T", "hmix"):
        for op in (A.OP_MEAN, A.OP_LAST):
            assert np.all(_fetch_zoomed(h, kc, 1, 1, n, op, 3, 4) == FILL)
            assert np.all(_fetch_zoomed(h, kc, 1, 1, n, op, 3, 4, fill=0, export=True) == 1e20)
    h.close()


def test_a_cancelled_zoom_leaves_the_steps_as_never_scheduled(mk):
    """A zoomed schedule set and then cancelled: the steps after it are bit-identical to a context never scheduled."""
    from test_window_schedule_gpu import _state_equal

    A = mk.api
    ncol, nz, nsteps = 400, 60, 6
    res = []
    for sched in (False, True):
        h, kc, k3 = _start(mk, ncol, nz, forced=False)
        if sched:
            h.window_schedule_zoom(1, 1, 2, 3, FIELDS, _all_ops(A), points=np.arange(0, ncol, 3)[::-1], levels=(0, 2))
            assert h.window_records(1) == (0, -1)
            h.window_schedule_zoom(1, 1, 1, 1, [], 0)
            with pytest.raises(mk.MckppHipError, match="schedule 1 is not set"):
                h.window_zoom(1)
        h.step(1, nsteps)
        h.download(k3)
        res.append(k3)
        h.close()
    _state_equal(res[1], res[0])
    for n in ("difs", "dift", "ghat", "wU", "wXNT", "Rig", "Shsq", "buoy", "cp"):
        assert np.array_equal(np.asarray(getattr(res[1], n)), np.asarray(getattr(res[0], n)), equal_nan=True), n


@pytest.mark.parametrize("shards,nz", [(0, 60), (2, 69)])
def test_fortran_forced_run_with_a_zoomed_schedule(built, tmp_path, shards, nz):
    """kpp_driver flags 256 + 32768: flag 256's schedule (mean hmix, maximum T over windows of two steps) zoomed to every
    third point in descending order and to levels 0..1, through mckpp_hip_all_window_schedule_zoom, on one device and on
    two shards - against the C-ABI run step by step, in the manner of tests/test_fortran_window_schedule_gpu.py."""
    import subprocess

    import mckpp_f90_amd as mk
    from test_fortran_host import DRIVER, _read_out, _write_case

    ncol, nsteps, period = 211, 4, 2
    nrec = nsteps // period
    pts = np.arange(ncol - 1, -1, -3)
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    _write_case(tmp_path / "case.bin", kc, k3, sf, nsteps, 0, flags=256 + 32768, shards=shards)
    r = subprocess.run([DRIVER, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    ocean = (k3.run_physics != 0)[pts]
    assert ocean.any() and not ocean.all()
    assert f"schedule 0 zoomed to {len(pts)} points, levels 0..1, {nrec * int(ocean.sum()) * (1 + 8) * 8} bytes" in r.stdout
    got = _read_out(tmp_path / "out.bin", kc, ncol)
    raw = (tmp_path / "out.bin").read_bytes()
    per_rec = len(pts) * (1 + 2)
    tail = np.frombuffer(raw[len(raw) - 8 * nrec * per_rec:], dtype=np.float64)
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    cm.set_forcing_3d(k3, sf)
    one = np.ones(ncol)
    hm, tmax = None, None
    for nt in range(1, nsteps + 1):
        ctx.fluxes(nt, 0.01 * one, 0 * one, 200 * one, 0 * one, -150 * one, 0 * one, 6e-5 * one, 0 * one)
        mk.mckpp_physics_driver(k3, kc, nt, new_forcing=False)
        first = (nt - 1) % period == 0
        hm = np.zeros(ncol) + k3.hmix if first else hm + k3.hmix
        tmax = k3.X[:, :, 0].copy() if first else np.maximum(tmax, k3.X[:, :, 0])
        if nt % period == 0:
            w = nt // period - 1
            blk = tail[w * per_rec:(w + 1) * per_rec]
            g_h, g_t = blk[:len(pts)], blk[len(pts):].reshape((len(pts), 2), order="F")
            assert np.array_equal(g_h[ocean], (hm / period)[pts][ocean]) and np.all(g_h[~ocean] == -1), w
            assert np.array_equal(g_t[ocean], tmax[pts][:, :2][ocean]) and np.all(g_t[~ocean] == -1), w
    for n in ("U", "X", "hmix", "kmix", "Tref", "difm", "rho"):
        assert np.array_equal(got[n], getattr(k3, n)), n
