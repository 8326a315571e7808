"""Restart snapshots taken inside the step launches (mckpp_hip_restart_schedule): the column kernel copies each
column's restart set into a ring slot right after the column's scheduled step, so that a run with restart output can
take many steps in one launch.  Every snapshot file must be, byte for byte, what a second context run from the same
start writes with save_restart after a launch that ends at the snapshot's step."""
import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401

pytestmark = pytest.mark.gpu

NSTEPS, P = 36, 12


def _make(mk, ncol, nz, grid, nsteps=NSTEPS, land_every=7, diag=True, ext=False, shards=0):
    """A context (or a multi handle of `shards` shards on device 0) at the start of the forced run: uploaded,
    initialised, the flux records of every step resident."""
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, land_every=land_every)
    if ext:
        kc.L_NO_FREEZE = 1
        kc.L_RELAX_SST = 1
        k3.relax_sst[:] = 1.0 / (5.0 + np.arange(ncol) % 11)
        k3.SST0[:] = np.asarray(k3.X[:, 0, 0]) - 0.5
    h = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    h.set_flux_series(0, cm.synth.flux_series(ncol, 1, nsteps, kc.dto))
    if not diag:
        h.set_diagnostics(0)
    return h, kc, k3


def _reference_files(mk, tmp, tag, ndtocn, nsteps=NSTEPS, period=P, **case):
    """Context A: run_forced(nt, period) + save_restart, launch after launch; {step: file}."""
    a, _, _ = _make(mk, nsteps=nsteps, **case)
    files = {}
    for nt in range(1, nsteps + 1, period):
        a.run_forced(nt, period, ndtocn)
        files[nt + period - 1] = tmp / f"{tag}_A_step{nt + period - 1}"
        a.save_restart(files[nt + period - 1])
    a.close()
    return files


def _same_bytes(got, ref, what):
    g, r = open(got, "rb").read(), open(ref, "rb").read()
    assert len(g) == len(r) and len(g) > 64, (what, len(g), len(r))
    if g != r:
        first = next(i for i in range(len(g)) if g[i] != r[i])
        pytest.fail(f"{what}: the files differ from byte {first} of {len(g)}")


def _cs_records(path):
    """The cs records (ncol, MCKPP_CS) of a restart file: behind the header, the column map and the 16 rows."""
    raw = open(path, "rb").read()
    nz, ld, ncs, nci, nrows = np.frombuffer(raw, dtype=np.int32, count=5, offset=12)
    ncol = int(np.frombuffer(raw, dtype=np.int64, count=1, offset=40)[0])
    off = 48 + 4 * ncol + 8 * ncol * int(ld) * int(nrows)
    assert len(raw) == off + ncol * (8 * int(ncs) + 4 * int(nci)) and nrows == 16
    return np.frombuffer(raw, dtype=np.float64, count=ncol * int(ncs), offset=off).reshape(ncol, int(ncs))


CASES = [
    dict(ncol=2000, nz=40, grid="stretched"),
    dict(ncol=5000, nz=60, grid="stretched"),
    dict(ncol=3000, nz=69, grid="stretched"),
]


@pytest.mark.parametrize("ndtocn", [1, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['ncol']}x{c['nz']}")
def test_snapshots_of_one_forced_run_are_the_restart_files(mk, tmp_path, case, ndtocn):
    """36 steps as ONE run_forced under restart_schedule(1, 12, 3) against run_forced(nt, 12) + save_restart three
    times; with ndtocn = 4 a flux update lands between snapshots, so the flux slots of the column records differ from
    snapshot to snapshot."""
    ref = _reference_files(mk, tmp_path, "r", ndtocn, **case)
    b, _, _ = _make(mk, **case)
    b.restart_schedule(1, P, 3)
    assert b.restart_scheduled == (1, P, 3) and b.restart_snapshots() == (0, -1)
    b.run_forced(1, NSTEPS, ndtocn)
    assert b.last_launch_count() == 1
    assert b.restart_snapshots() == (0, 2)
    for s in range(3):
        b.restart_snapshot_save(s, tmp_path / f"B{s}")
        _same_bytes(tmp_path / f"B{s}", ref[(s + 1) * P], f"snapshot {s}")
    b.close()
    if ndtocn == 4:   # the comparison above has seen flux slots that differ from snapshot to snapshot
        flux = [_cs_records(ref[(s + 1) * P])[:, 5:11] for s in range(3)]   # CS_SFLUX1 .. CS_SFLUX6
        assert not np.array_equal(flux[0], flux[1]) and not np.array_equal(flux[1], flux[2])


@pytest.mark.parametrize("variant", ["diag_off", "ext", "launch_per_step"])
def test_snapshots_with_diagnostics_off_optional_physics_and_a_launch_per_step(mk, tmp_path, monkeypatch, variant):
    """The same byte identity with the diagnostics off (the snapshot still carries the rho and cp rows), in an
    optional-physics context (L_NO_FREEZE + L_RELAX_SST: the EXT kernel build), and under MCKPP_MULTISTEP=0 (a launch
    per step)."""
    monkeypatch.delenv("MCKPP_MULTISTEP", raising=False)
    case = dict(ncol=3000, nz=60, grid="stretched")
    if variant == "diag_off":
        case["diag"] = False
    if variant == "ext":
        case["ext"] = True
    if variant == "launch_per_step":
        monkeypatch.setenv("MCKPP_MULTISTEP", "0")
    ref = _reference_files(mk, tmp_path, "r", 4, **case)
    b, _, _ = _make(mk, **case)
    if variant == "ext":
        assert b.kernel_name == "k_column_ps<EXT>"
    b.restart_schedule(1, P, 3)
    b.run_forced(1, NSTEPS, 4)
    assert b.last_launch_count() == (NSTEPS if variant == "launch_per_step" else 1)
    for s in range(3):
        b.restart_snapshot_save(s, tmp_path / f"B{s}")
        _same_bytes(tmp_path / f"B{s}", ref[(s + 1) * P], f"{variant}: snapshot {s}")
    b.close()


def _all_fields(k3):
    return {n: np.array(v, copy=True) for n, v in vars(k3).items() if isinstance(v, np.ndarray)}


def test_a_run_continued_from_a_snapshot_ends_bit_for_bit_the_same(mk, tmp_path):
    """A fresh context loads snapshot 1 (the state after step 24), runs steps 25..36 and ends with the state of the
    one-launch run: every field of download(F_ALL), the status words and the pass counts."""
    case = dict(ncol=4000, nz=60, grid="stretched")
    b, _, k3b = _make(mk, **case)
    b.restart_schedule(1, P, 3)
    b.run_forced(1, NSTEPS, 4)
    b.restart_snapshot_save(1, tmp_path / "snap1")
    b.download(k3b)
    stb = b.status()
    c, _, k3c = _make(mk, **case)
    c.load_restart(tmp_path / "snap1", case["ncol"])
    c.run_forced(2 * P + 1, P, 4)
    c.download(k3c)
    stc = c.status()
    fb, fc = _all_fields(k3b), _all_fields(k3c)
    assert fb.keys() == fc.keys() and "Xs" in fb and "wX" in fb
    for n in fb:
        assert np.array_equal(fb[n], fc[n], equal_nan=True), n
    assert np.array_equal(stb[0], stc[0]) and stb[1] == stc[1] and np.array_equal(stb[2], stc[2])
    b.close()
    c.close()


def test_snapshots_are_saved_while_later_launches_are_queued(mk, tmp_path):
    """run_forced(1, 24) and run_forced(25, 12) queued without a synchronise between, snapshots 0 and 1 saved at once:
    the save waits for the first call's launch alone.  After a synchronise snapshot 2 is right as well."""
    case = dict(ncol=20000, nz=60, grid="stretched")
    ref = _reference_files(mk, tmp_path, "r", 4, **case)
    b, _, _ = _make(mk, **case)
    b.restart_schedule(1, P, 3)
    b.run_forced(1, 2 * P, 4)
    b.run_forced(2 * P + 1, P, 4)
    b.restart_snapshot_save(0, tmp_path / "B0")
    b.restart_snapshot_save(1, tmp_path / "B1")
    _same_bytes(tmp_path / "B0", ref[P], "snapshot 0")
    _same_bytes(tmp_path / "B1", ref[2 * P], "snapshot 1")
    b.synchronize()
    b.restart_snapshot_save(2, tmp_path / "B2")
    _same_bytes(tmp_path / "B2", ref[3 * P], "snapshot 2")
    b.close()


def test_the_ring_guards_its_slots(mk, tmp_path):
    """nslots = 2: a launch that reaches snapshot 2 before snapshot 0 is released is refused with nothing launched;
    released, incomplete and never-existing snapshots are refused by name of their step; upload cancels."""
    case = dict(ncol=2000, nz=40, grid="stretched")
    ref = _reference_files(mk, tmp_path, "r", 1, **case)
    b, _, k3 = _make(mk, **case)
    b.restart_schedule(1, P, 2)
    b.run_forced(1, 2 * P, 1)
    assert b.restart_snapshots() == (0, 1)
    b.download(k3)
    before = _all_fields(k3)
    with pytest.raises(mk.MckppHipError, match=r"reach restart snapshot 2 \(after step 36\).*ring of 2.*snapshot 0 \(after step 12\)"):
        b.run_forced(2 * P + 1, P, 1)
    b.synchronize()
    b.download(k3)
    for n, v in before.items():
        assert np.array_equal(np.asarray(getattr(k3, n)), v, equal_nan=True), n
    assert b.restart_snapshots() == (0, 1)
    with pytest.raises(mk.MckppHipError, match=r"snapshot 2 \(after step 36\) is incomplete"):
        b.restart_snapshot_save(2, tmp_path / "never")
    with pytest.raises(mk.MckppHipError, match=r"snapshot 2 \(after step 36\) is not complete"):
        b.restart_snapshot_release(2)
    with pytest.raises(mk.MckppHipError, match=r"follow on from one another"):
        b.run_forced(2 * P + 2, 1, 1)
    b.restart_snapshot_release(0)
    assert b.restart_snapshots() == (1, 1)
    b.run_forced(2 * P + 1, P, 1)
    assert b.restart_snapshots() == (1, 2)
    with pytest.raises(mk.MckppHipError, match=r"snapshot 0 \(after step 12\) has been released"):
        b.restart_snapshot_save(0, tmp_path / "never")
    assert not (tmp_path / "never").exists()
    for s in (1, 2):
        b.restart_snapshot_save(s, tmp_path / f"B{s}")
        _same_bytes(tmp_path / f"B{s}", ref[(s + 1) * P], f"snapshot {s}")
    b.upload(k3)   # cancels
    assert b.restart_scheduled is None
    with pytest.raises(mk.MckppHipError, match=r"no restart schedule is set"):
        b.restart_snapshots()
    b.close()
    # a schedule set after steps have run: the snapshot due before it does not exist
    b, _, _ = _make(mk, **case)
    b.run_forced(1, P, 1)
    b.restart_schedule(1, P, 2)
    b.run_forced(P + 1, P, 1)
    assert b.restart_snapshots() == (1, 1)
    with pytest.raises(mk.MckppHipError, match=r"snapshot 0 \(after step 12\) does not exist"):
        b.restart_snapshot_save(0, tmp_path / "never")
    b.restart_snapshot_save(1, tmp_path / "B1again")
    _same_bytes(tmp_path / "B1again", ref[2 * P], "snapshot 1 of a schedule set mid-run")
    # slots that cannot be allocated: an error, no schedule, the process goes on
    with pytest.raises(mk.MckppHipError, match=r"cannot allocate"):
        b.restart_schedule(1, P, 1 << 24)
    assert b.restart_scheduled is None
    with pytest.raises(mk.MckppHipError, match=r"no restart schedule is set"):
        b.restart_snapshots()
    b.run_forced(2 * P + 1, 1, 1)
    b.close()


def test_snapshots_and_output_windows_together(mk, tmp_path):
    """Two output schedules and the restart schedule in one forced run: every window record and every snapshot equals
    what each feature gives alone."""
    A = mk.api
    case = dict(ncol=3000, nz=69, grid="stretched")
    fields, ops = ("T", "hmix", "difm", "rho"), A.WIN_MEAN | A.WIN_MAX

    def run(windows, snaps, tag):
        h, kc, k3 = _make(mk, **case)
        if windows:
            h.window_schedule(0, 1, 3, 12, ("T", "S", "hmix"), A.WIN_LAST)
            h.window_schedule(1, 1, 4, 9, fields, ops)
        if snaps:
            h.restart_schedule(1, P, 3)
        h.run_forced(1, NSTEPS, 4)
        rec = {}
        if windows:
            for w in range(12):
                for n in ("T", "S", "hmix"):
                    shape = (case["ncol"],) if n == "hmix" else (case["ncol"], kc.nzp1)
                    rec[0, w, n] = h.window_record_fetch(0, w, n, A.OP_LAST, np.full(shape, -7.0, order="F")).copy()
            for w in range(9):
                for n in fields:
                    for op in (A.OP_MEAN, A.OP_MAX):
                        shape = (case["ncol"],) if n == "hmix" else (case["ncol"], kc.nzp1)
                        rec[1, w, n, op] = h.window_record_fetch(1, w, n, op, np.full(shape, -7.0, order="F")).copy()
        files = []
        if snaps:
            for s in range(3):
                files.append(tmp_path / f"{tag}{s}")
                h.restart_snapshot_save(s, files[-1])
        h.close()
        return rec, files

    rec_w, _ = run(True, False, "w")
    _, files_s = run(False, True, "s")
    rec_b, files_b = run(True, True, "b")
    assert rec_b.keys() == rec_w.keys() and len(rec_w) == 12 * 3 + 9 * 4 * 2
    for key in rec_w:
        assert np.array_equal(rec_b[key], rec_w[key], equal_nan=True), key
    for s in range(3):
        _same_bytes(files_b[s], files_s[s], f"snapshot {s} beside the output windows")


@pytest.mark.parametrize("shards", [2, 4])
def test_multi_handle_snapshots_are_the_shards_restart_files(mk, tmp_path, shards):
    """MckppHipMulti(kc, [0] * shards): the per-shard snapshot files equal multi_save_restart's at the same step, and
    multi_load_restart of them continues bit for bit."""
    case = dict(ncol=4001, nz=60, grid="stretched", shards=shards)
    a, _, _ = _make(mk, **case)
    for nt in range(1, NSTEPS + 1, P):
        a.run_forced(nt, P, 4)
        a.save_restart(tmp_path / f"A{nt + P - 1}")
    a.close()
    b, _, k3b = _make(mk, **case)
    b.restart_schedule(1, P, 3)
    b.run_forced(1, NSTEPS, 4)
    assert b.restart_snapshots() == (0, 2)
    for s in range(3):
        b.restart_snapshot_save(s, tmp_path / f"B{s}")
        for d in range(shards):
            _same_bytes(tmp_path / f"B{s}.{d}of{shards}", tmp_path / f"A{(s + 1) * P}.{d}of{shards}", f"snapshot {s}, shard {d}")
    b.restart_snapshot_release(2)
    assert b.restart_snapshots() == (3, 2)
    b.download(k3b)
    stb = b.status()
    c, _, k3c = _make(mk, **case)
    c.load_restart(tmp_path / "B1")
    c.run_forced(2 * P + 1, P, 4)
    c.download(k3c)
    stc = c.status()
    fb, fc = _all_fields(k3b), _all_fields(k3c)
    for n in fb:
        assert np.array_equal(fb[n], fc[n], equal_nan=True), n
    assert np.array_equal(stb[0], stc[0]) and stb[1] == stc[1] and np.array_equal(stb[2], stc[2])
    b.close()
    c.close()
