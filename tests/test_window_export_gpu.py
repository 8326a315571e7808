"""The packed export of an output schedule's records (mckpp_hip_window_export): every step-launch call packs the records
it completed into export slots in the host's layout (k_record_pack), and a fetch is one copy behind the slot's event.
The reference is window_record_fetch in the same context - a code path the export does not touch - into an array
pre-filled with land_value: "f8" planes equal it bit for bit, "f4" planes equal its .astype(float32) compared as uint32,
and land points hold land_value converted likewise.  Everything is asserted to equality."""
import ctypes as C
import filecmp

import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401
from harness import shape as _shape

pytestmark = pytest.mark.gpu

LAST_FIELDS = ("T", "S", "hmix")
RED_FIELDS = ("T", "S", "hmix", "difm", "wT", "rho", "Rig", "solar_in")
LAND = 1e20
NP = {"f8": np.float64, "f4": np.float32}
BITS = {"f8": np.uint64, "f4": np.uint32}
ENV = ("MCKPP_MULTISTEP", "MCKPP_PS_FIXED_L", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT")


def _ops(mask):
    return [op for op in range(4) if (mask >> op) & 1]


def _start(mk, ncol, nz, grid="uniform", land_every=7, nsteps=12, forced=True, shards=0, switches=()):
    """A context (or a multi handle of `shards` shards on device 0) at the start of a run of nsteps steps."""
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, land_every=land_every)
    for s in switches:
        setattr(kc, s, 1)
    if "L_FCORR_WITHZ" in switches:
        z = np.arange(kc.nzp1)[None, :]
        k3.fcorr_withz[:, :] = 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, ncol)[:, None]
    h = mk.MckppHip(kc) if shards == 0 else mk.MckppHipMulti(kc, [0] * shards)
    h.upload(k3)
    h.init_ocean(0)
    if forced:
        h.set_flux_series(0, cm.synth.flux_series(ncol, 1, nsteps, kc.dto))
    else:
        cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
        h.set_forcing(k3.sflux)
    return h, kc, k3


def _schedule(mk, h, pl=3, pr=4, nrec=8, nrec_last=None, red=RED_FIELDS, last=LAST_FIELDS):
    A = mk.api
    h.window_schedule(0, 1, pl, nrec_last or nrec, last, A.WIN_LAST)
    h.window_schedule(1, 1, pr, nrec, red, A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX)
    return {0: (last, A.WIN_LAST), 1: (red, A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX)}


def _reference(h, kc, npts, sched, rec, name, op, dtype, land=LAND, bufs=None):
    """window_record_fetch into an array pre-filled with the land value, narrowed as the export narrows (bufs: arrays
    to use again, by shape - the result is then good until the next call)"""
    shape = _shape(kc, npts, name)
    out = np.full(shape, land, order="F") if bufs is None else bufs.setdefault(("ref", shape), np.zeros(shape, order="F"))
    out[...] = land
    h.window_record_fetch(sched, rec, name, op, out)
    return out.astype(NP[dtype], order="F") if dtype == "f4" else out


def _same_bits(got, want, dtype, tag):
    assert got.dtype == want.dtype == NP[dtype] and got.shape == want.shape, tag
    assert np.array_equal(got.view(BITS[dtype]), want.view(BITS[dtype])), tag


def _check(h, kc, npts, scheds, dtype, recs=None, land=LAND, ref=None, bufs=None):
    """every plane of every record (recs: {schedule: records}; default: all that can be fetched) through the export
    against the reference fetched from `ref` (default: the context itself)"""
    n = 0
    bufs = {} if bufs is None else bufs
    for s, (names, mask) in scheds.items():
        fk, lc = h.window_records(s)
        for rec in (recs[s] if recs is not None else range(fk, lc + 1)):
            for name in names:
                for op in _ops(mask):
                    shape = _shape(kc, npts, name)
                    out = bufs.setdefault(shape, np.zeros(shape, dtype=NP[dtype], order="F"))
                    out[...] = 0
                    h.window_export_fetch(s, rec, name, op, out)
                    _same_bits(out, _reference(ref or h, kc, npts, s, rec, name, op, dtype, land, bufs), dtype, (s, rec, name, op))
                    n += 1
    return n


@pytest.mark.parametrize("dtype", ["f8", "f4"])
@pytest.mark.parametrize("nz,grid,ncol", [(60, "uniform", 130), (69, "stretched", 70), (100, "uniform", 65), (40, "uniform", 40)])
def test_export_equals_record_fetch_where_the_tiles_can_go_wrong(mk, nz, grid, ncol, dtype):
    """12 steps in one run_forced under the two iodef-like schedules, land every 7th point: resident columns that are no
    multiple of the 64-column tile (130 points), nzp1 = 70 across a level tile with the interface fields on levels
    0..nz (69 stretched levels), two level tiles (100 levels), fewer points than one tile (40)."""
    h, kc, k3 = _start(mk, ncol, nz, grid)
    scheds = _schedule(mk, h)
    for s in scheds:
        h.window_export(s, dtype, LAND)
    h.run_forced(1, 12, 1)
    assert h.window_records(0) == (0, 3) and h.window_records(1) == (0, 2)
    assert _check(h, kc, ncol, scheds, dtype) == 4 * 3 + 3 * 8 * 3
    h.close()


def test_one_level_planes_of_more_than_256_columns_narrowed(mk):
    """321 points, every 40th land: 312 resident columns, 256 and a tail of 56.  The column-per-thread path of a
    two-dimensional field then takes two workgroups, the second with a tail in its last 64 columns; float32, which the
    shapes above reach with one workgroup only.  T beside it goes through the tile in five column tiles."""
    ncol = 321
    h, kc, k3 = _start(mk, ncol, 40, land_every=40)
    assert h.ncolumns == 312
    scheds = _schedule(mk, h, red=("hmix", "T"), last=("hmix", "solar_in"))
    for s in scheds:
        h.window_export(s, "f4", LAND)
    h.run_forced(1, 12, 1)
    assert _check(h, kc, ncol, scheds, "f4") == 4 * 2 + 3 * 2 * 3
    h.close()


def test_ring_wrap_and_records_cut_by_calls(mk):
    """Calls of 5 + 7 + 12 steps with releases between; the mean/min/max schedule (period 4) has nrec = 3, the "last"
    schedule (period 3) nrec = 4 - the last call completes four of its records, which a ring of three refuses.  A
    record begun in one call is completed in the next (steps 4..6, 5..8), one call completes several, the slots are
    reused, and the export is set only after the first call: its complete records are packed at once."""
    ncol = 130
    h, kc, k3 = _start(mk, ncol, 60, nsteps=24)
    scheds = _schedule(mk, h, nrec=3, nrec_last=4)
    h.run_forced(1, 5, 1)
    h.window_export(0, "f8", LAND)
    h.window_export(1, "f4", -3.5)
    assert h.window_records(0) == (0, 0) and h.window_records(1) == (0, 0)
    seen = 0
    for nt0, n, want0, want1 in ((0, 0, (0, 0), (0, 0)), (6, 7, (1, 3), (1, 2)), (13, 12, (4, 7), (3, 5))):
        if n:
            h.run_forced(nt0, n, 1)
        assert h.window_records(0) == want0 and h.window_records(1) == want1
        seen += _check(h, kc, ncol, {0: scheds[0]}, "f8")
        seen += _check(h, kc, ncol, {1: scheds[1]}, "f4", land=-3.5)
        h.window_record_release(0, want0[1])
        h.window_record_release(1, want1[1])
    assert seen == 8 * 3 + 6 * 8 * 3
    h.close()


@pytest.mark.parametrize("dtype", ["f8", "f4"])
def test_whole_record_fetch_and_layout(mk, dtype):
    """fetch_record equals the planes at the offsets window_export_layout reports; the planes come in the schedule's
    field order, within a field in bit order of its mask; every offset is a multiple of 256."""
    A = mk.api
    ncol, nz = 70, 69
    h, kc, k3 = _start(mk, ncol, nz, "stretched")
    masks = [A.WIN_MAX | A.WIN_MEAN, A.WIN_LAST, A.WIN_MIN | A.WIN_LAST | A.WIN_MEAN]
    h.window_schedule(2, 1, 4, 3, ("wT", "hmix", "S"), masks)
    h.window_export(2, dtype)
    h.run_forced(1, 12, 1)
    planes, rb = h.window_export_layout(2)
    assert [(f, op) for f, op, _, _ in planes] == [(A.OUT["wT"], 0), (A.OUT["wT"], 2), (A.OUT["hmix"], 3), (A.OUT["S"], 0),
                                                   (A.OUT["S"], 1), (A.OUT["S"], 3)]
    assert [nl for _, _, nl, _ in planes] == [70, 70, 1, 70, 70, 70]
    item = np.dtype(NP[dtype]).itemsize
    assert all(off % 256 == 0 for _, _, _, off in planes) and rb % 256 == 0
    ends = [off + ncol * nl * item for _, _, nl, off in planes]
    assert all(e <= o for e, (_, _, _, o) in zip(ends, planes[1:])) and ends[-1] <= rb   # (no plane over another)
    for rec in range(3):
        buf = np.zeros(rb // item, dtype=NP[dtype])
        h.window_export_fetch_record(2, rec, buf)
        for f, op, nl, off in planes:
            name = A.OUT_FIELDS[f]
            got = buf[off // item: off // item + ncol * nl].reshape(_shape(kc, ncol, name), order="F")
            _same_bits(np.asfortranarray(got), _reference(h, kc, ncol, 2, rec, name, op, dtype), dtype, (rec, name, op))
    h.close()


def test_records_are_fetched_while_later_launches_are_queued(mk):
    """run_forced(1, 12) and run_forced(13, 288) queued without a synchronise between: the first call's records are
    fetched at once, through events behind the first call's launches alone, and equal a twin context's after its
    synchronise.  Then synchronise and fetch the rest.  No assertion about time."""
    ncol, nz, nsteps = 1000, 60, 300
    twin, kc, _ = _start(mk, ncol, nz, nsteps=nsteps)
    scheds = _schedule(mk, twin, nrec=100)
    twin.run_forced(1, 12, 1)
    twin.run_forced(13, nsteps - 12, 1)
    twin.synchronize()
    h, _, _ = _start(mk, ncol, nz, nsteps=nsteps)
    _schedule(mk, h, nrec=100)
    for s in scheds:
        h.window_export(s, "f8")
    h.run_forced(1, 12, 1)
    h.run_forced(13, nsteps - 12, 1)
    bufs = {}
    first = {0: range(0, 4), 1: range(0, 3)}
    assert _check(h, kc, ncol, scheds, "f8", recs=first, ref=twin, bufs=bufs) == 4 * 3 + 3 * 8 * 3
    h.synchronize()
    assert h.window_records(0) == (0, 99) and h.window_records(1) == (0, 74)
    rest = {0: range(4, 100), 1: range(3, 75)}
    assert _check(h, kc, ncol, scheds, "f8", recs=rest, ref=twin, bufs=bufs) == 96 * 3 + 72 * 8 * 3
    h.close()
    twin.close()


@pytest.mark.parametrize("form", ["launch_per_step", "constant_forcing", "forced_views", "general_kernel"])
def test_launch_forms(mk, monkeypatch, form):
    """MCKPP_MULTISTEP=0 (a launch per step), constant-forcing step(nt, n) in two calls, workgroups in views throughout,
    and the kernels that take the level count at run time (MCKPP_PS_FIXED_L=0)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    env = {"launch_per_step": {"MCKPP_MULTISTEP": "0"}, "constant_forcing": {},
           "forced_views": {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}, "general_kernel": {"MCKPP_PS_FIXED_L": "0"}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ncol = 130
    forced = form in ("forced_views", "general_kernel")
    h, kc, k3 = _start(mk, ncol, 60, forced=forced)
    scheds = _schedule(mk, h)
    h.window_export(0, "f4")
    h.window_export(1, "f8")
    for nt0, n in ((1, 5), (6, 7)):
        if forced:
            h.run_forced(nt0, n, 1)
        else:
            h.step(nt0, n)
    assert _check(h, kc, ncol, {0: scheds[0]}, "f4") + _check(h, kc, ncol, {1: scheds[1]}, "f8") == 4 * 3 + 3 * 8 * 3
    h.close()


@pytest.mark.parametrize("dtype", ["f8", "f4"])
def test_optional_physics_fields_and_every_two_dimensional_field(mk, dtype):
    """An optional-physics context (L_FCORR_WITHZ, L_DAMP_CURR): tinc_fcorr and fcorr_z, and every two-dimensional field,
    the flags included."""
    A = mk.api
    ncol = 130
    two_d = ("hmix",) + A.OUT_FIELDS[A.OUT["fcorr"]:]
    assert len(two_d) == 11
    h, kc, k3 = _start(mk, ncol, 60, forced=False, switches=("L_FCORR_WITHZ", "L_DAMP_CURR"))
    mask = A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX | A.WIN_LAST
    scheds = {0: (("tinc_fcorr", "fcorr_z"), mask), 1: (two_d, mask)}
    for s, (names, m) in scheds.items():
        h.window_schedule(s, 1, 4, 2, names, m)
        h.window_export(s, dtype, -1e30)
    h.step(1, 8)
    assert _check(h, kc, ncol, scheds, dtype, land=-1e30) == 2 * 13 * 4
    h.close()


def test_beside_a_restart_schedule_a_step_log_and_an_ancillary_schedule(mk, tmp_path):
    """One forced run with a restart schedule, a step log and an ancillary schedule, with and without the export: the
    snapshot files, the log and the records of window_record_fetch are unchanged, and the export equals them."""
    A = mk.api
    ncol, nz, nsteps = 130, 60, 12
    res = []
    for export in (False, True):
        h, kc, k3 = _start(mk, ncol, nz, switches=("L_FCORR_WITHZ",))
        z = np.arange(kc.nzp1)[None, :, None]
        recs = np.stack([(1.0 + r) * np.exp(-z[0] / 10.0) * np.linspace(-1, 1, ncol)[None, :] for r in range(3)])
        h.set_ancillary_series(A.ANC_FCORR_WITHZ, 0, recs)
        h.ancillary_schedule(A.ANC_FCORR_WITHZ, 1, 4, [0, 1, 2])
        h.restart_schedule(1, 6, 2)
        h.step_log(nsteps * ncol, 1)
        scheds = _schedule(mk, h, red=("T", "tinc_fcorr", "fcorr_z", "hmix"))
        if export:
            for s in scheds:
                h.window_export(s, "f8")
        h.run_forced(1, nsteps, 1)
        files = []
        for s in range(2):
            files.append(tmp_path / f"snap{int(export)}_{s}")
            h.restart_snapshot_save(s, files[-1])
        got = {}
        for s, (names, mask) in scheds.items():
            for rec in range(h.window_records(s)[1] + 1):
                for name in names:
                    for op in _ops(mask):
                        got[s, rec, name, op] = _reference(h, kc, ncol, s, rec, name, op, "f8")
        if export:
            assert _check(h, kc, ncol, scheds, "f8") == len(got)
        res.append((files, h.step_log_count(), h.step_log_fetch(), got))
        h.close()
    (f0, c0, l0, g0), (f1, c1, l1, g1) = res
    for a, b in zip(f0, f1):
        assert filecmp.cmp(a, b, shallow=False), (a, b)
    assert c0 == c1 and c0[1] > 0
    for a, b in zip(l0, l1):
        assert np.array_equal(a, b)
    assert g0.keys() == g1.keys() and len(g0) == 4 * 3 + 3 * 4 * 3
    for k in g0:
        _same_bits(g1[k], g0[k], "f8", k)


def test_refusals_leave_the_context_as_it_was(mk):
    """No export set, a record that is incomplete or released, a field or op not kept, an out_bytes too small, an unset
    schedule, an unknown dtype: an error with a message, and a good fetch after each."""
    A = mk.api
    lib = A._lib()
    ncol = 130
    h, kc, k3 = _start(mk, ncol, 60)
    h.window_schedule(0, 1, 2, 2, ["T"], A.WIN_MEAN | A.WIN_LAST)
    out = np.zeros((ncol, kc.nzp1), order="F")
    outp = out.ctypes.data

    def good():
        out[...] = 0
        h.window_export_fetch(0, 1, "T", A.OP_MEAN, out)
        _same_bits(out, _reference(h, kc, ncol, 0, 1, "T", A.OP_MEAN, "f8"), "f8", "good fetch")

    def refused(rc, text):
        assert rc < 0 and text in lib.mckpp_hip_last_error(), lib.mckpp_hip_last_error()

    h.run_forced(1, 4, 1)   # records 0, 1 complete
    refused(lib.mckpp_hip_window_export_fetch(h._h, 0, 1, A.OUT["T"], 0, outp), b"schedule 0 has no export")
    refused(lib.mckpp_hip_window_export_fetch_record(h._h, 0, 1, outp, out.nbytes), b"schedule 0 has no export")
    refused(lib.mckpp_hip_window_export_layout(h._h, 0, None, None, None, None, None, None), b"schedule 0 has no export")
    with pytest.raises(ValueError, match="has no export"):
        h.window_export_fetch(0, 1, "T", A.OP_MEAN, out)
    refused(lib.mckpp_hip_window_export(h._h, 0, 3, 0.0), b"dtype 3")
    refused(lib.mckpp_hip_window_export(h._h, 1, A.EXP_F64, 0.0), b"schedule 1 is not set")
    h.window_export(0, "f8")
    good()
    with pytest.raises(mk.MckppHipError, match=r"window_export_fetch: record 2 of schedule 0 \(steps 5\.\.6\) is incomplete"):
        h.window_export_fetch(0, 2, "T", A.OP_LAST, out)
    good()
    h.window_record_release(0, 0)
    with pytest.raises(mk.MckppHipError, match=r"record 0 of schedule 0 \(steps 1\.\.2\) has been released"):
        h.window_export_fetch(0, 0, "T", A.OP_LAST, out)
    good()
    refused(lib.mckpp_hip_window_export_fetch(h._h, 0, 1, A.OUT["S"], 0, outp), b"field 5 is not in schedule 0")
    good()
    refused(lib.mckpp_hip_window_export_fetch(h._h, 0, 1, A.OUT["T"], A.OP_MAX, outp), b"keeps no op 2")
    good()
    _, rb = h.window_export_layout(0)
    refused(lib.mckpp_hip_window_export_fetch_record(h._h, 0, 1, outp, rb - 1), b"out_bytes")
    good()
    refused(lib.mckpp_hip_window_export_fetch(h._h, 1, 0, A.OUT["T"], 0, outp), b"schedule 1 is not set")
    good()
    with pytest.raises(ValueError, match="holds float64"):
        h.window_export_fetch(0, 1, "T", A.OP_MEAN, np.zeros((ncol, kc.nzp1), dtype=np.float32, order="F"))
    good()
    h.run_forced(5, 2, 1)   # the context goes on: record 2 complete, in the slot record 0 left
    h.window_export_fetch(0, 2, "T", A.OP_LAST, out)
    _same_bits(out, _reference(h, kc, ncol, 0, 2, "T", A.OP_LAST, "f8"), "f8", "record 2")
    h.close()


def test_cancelling(mk):
    """window_export(sched, None), re-scheduling and upload each drop the export; the schedule's records stay where
    window_record_fetch finds them (upload: the schedule goes too)."""
    A = mk.api
    lib = A._lib()
    ncol = 130
    h, kc, k3 = _start(mk, ncol, 60)
    h.window_schedule(0, 1, 2, 4, ["T", "hmix"], A.WIN_LAST)
    h.window_export(0, "f4")
    h.run_forced(1, 4, 1)
    out = np.zeros((ncol, kc.nzp1), order="F")
    assert _check(h, kc, ncol, {0: (("T", "hmix"), A.WIN_LAST)}, "f4") == 4
    h.window_export(0, None)
    assert lib.mckpp_hip_window_export_fetch(h._h, 0, 1, A.OUT["T"], 3, out.ctypes.data) < 0
    assert b"schedule 0 has no export" in lib.mckpp_hip_last_error()
    h.window_record_fetch(0, 1, "T", A.OP_LAST, out)   # the records themselves are untouched
    h.window_export(0, "f8")   # set again: records 0 and 1 are packed at once
    assert _check(h, kc, ncol, {0: (("T", "hmix"), A.WIN_LAST)}, "f8") == 4
    h.synchronize()
    h.window_schedule(0, 5, 2, 4, ["T"], A.WIN_LAST)   # a schedule set anew has no export
    h.run_forced(5, 2, 1)
    assert lib.mckpp_hip_window_export_fetch(h._h, 0, 0, A.OUT["T"], 3, out.ctypes.data) < 0
    assert b"schedule 0 has no export" in lib.mckpp_hip_last_error()
    with pytest.raises(ValueError, match="has no export"):
        h.window_export_fetch(0, 0, "T", A.OP_LAST, out)
    h.window_export(0, "f8")
    assert _check(h, kc, ncol, {0: (("T",), A.WIN_LAST)}, "f8") == 1
    h.download(k3)
    h.upload(k3)
    assert lib.mckpp_hip_window_export_fetch(h._h, 0, 0, A.OUT["T"], 3, out.ctypes.data) < 0
    assert b"schedule 0 is not set" in lib.mckpp_hip_last_error()
    h.close()


@pytest.mark.parametrize("dtype", ["f8", "f4"])
def test_three_shards_equal_the_single_context(mk, dtype):
    """Three shards on device 0 behind the multi handle, with land: planes and whole records equal the single context's,
    land points included."""
    ncol, nz, nsteps = 701, 69, 8
    item = np.dtype(NP[dtype]).itemsize
    outs = []
    for shards in (0, 3):
        h, kc, k3 = _start(mk, ncol, nz, "stretched", land_every=6, nsteps=nsteps, shards=shards)
        scheds = _schedule(mk, h, pl=2, pr=4, nrec=2)
        for s in scheds:
            h.window_export(s, dtype, LAND)
        got = {}
        for nt0 in (1, 5):
            h.run_forced(nt0, 4, 1)
            for s, (names, mask) in scheds.items():
                fk, lc = h.window_records(s)
                planes, rb = h.window_export_layout(s)
                for rec in range(fk, lc + 1):
                    for name in names:
                        for op in _ops(mask):
                            out = np.zeros(_shape(kc, ncol, name), dtype=NP[dtype], order="F")
                            got[s, rec, name, op] = h.window_export_fetch(s, rec, name, op, out)
                    buf = h.window_export_fetch_record(s, rec, np.zeros(rb // item, dtype=NP[dtype]))
                    got[s, rec, "planes"] = [buf[off // item: off // item + ncol * nl].copy() for _, _, nl, off in planes]
                    got[s, rec, "layout"] = (planes, rb)
                _check(h, kc, ncol, {s: scheds[s]}, dtype)   # (against the handle's own window_record_fetch)
                h.window_record_release(s, lc)
        if shards == 0:
            assert np.all(got[1, 1, "T", 0][~(k3.run_physics != 0)] == NP[dtype](LAND))
        h.close()
        outs.append(got)
    a, b = outs
    assert a.keys() == b.keys() and len(a) == (4 * 3 + 2 * 8 * 3) + 2 * 6
    for key in a:
        if key[2] == "layout":
            assert a[key] == b[key], key
        elif key[2] == "planes":
            for x, y in zip(a[key], b[key]):
                _same_bits(y, x, dtype, key)
        else:
            _same_bits(b[key], a[key], dtype, key)
