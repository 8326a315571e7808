"""The lifetime of a context's device and pinned memory: everything a context is given - two output schedules (one with
an export), a restart schedule, a step log, a bottom temperature (resident, or as an ancillary series with a schedule),
a flux series - is dropped by a second upload with another land mask (the state is allocated anew) and by close().

A cycle is: context, upload, set all of it, two run_forced calls, one record fetched and one snapshot saved; upload
again with another land mask - every schedule then reports itself unset -, set all of it again, run again, fetch and
save again, close.  What the second half fetched and saved equals, bit for bit, what a fresh context gives that is
handed the second half's inputs alone.  And device memory does not drain: the device's free memory is read after the
first cycle (code objects and scratch are loaded once), then two batches of four cycles run.  The figure is the whole
device's, which others may share, so the test fails only if free memory fell in EACH batch by at least 4 x half of what
one cycle allocates (computed below from the sizes asked for): a block of that size lost per cycle repeats in every
batch, another tenant's allocation does not."""
import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401

pytestmark = pytest.mark.gpu

NPTS, NZ, LD = 400, 20, 64          # 21 levels: rows of 64 doubles
LAND = (4, 5)                       # land every 4th point (300 columns), then every 5th (320)
NREC, NSLOTS, LOG_CAP = 64, 16, 1 << 20
LAST, RED = ("T", "S"), ("T", "difm")
STEPS = ((1, 3), (4, 3))            # two calls: steps 1..3, 4..6


def _half_bytes(ncol):
    """device memory one half of a cycle asks for, over the state's own: the rings, the export's slots, the snapshot
    slots, the log"""
    plane = ncol * LD * 8
    rings = NREC * plane * (len(LAST) * 1 + len(RED) * 3)
    export = NREC * len(LAST) * (NZ + 1) * NPTS * 8
    snaps = NSLOTS * 14 * plane   # (MCKPP_SNAP_ROWS whole rows; the per-column records beside them are small)
    return rings + export + snaps + LOG_CAP * 16


def _case(land_every):
    kc, k3 = cm.make_hip_case(NPTS, NZ, land_every=land_every)
    bt = np.asarray(k3.X[:, NZ, 0]) - 0.5 + 0.25 * np.sin(np.arange(NPTS))
    return kc, k3, bt, cm.synth.flux_series(NPTS, 1, 6, kc.dto)


def _half(mk, h, case, variant, path, unset=False):
    """upload, set everything, run, fetch one record and save one snapshot: (record planes, snapshot file's bytes)"""
    A = mk.api
    kc, k3, bt, series = case
    h.upload(k3)
    h.init_ocean(0)
    if unset:   # the first half's schedules are gone, with the messages a context gives that never had them
        for call, what in ((lambda: h.window_records(0), "schedule 0 is not set"),
                           (lambda: h.window_records(1), "schedule 1 is not set"),
                           (lambda: h.window_export_layout(0), "schedule 0 is not set"),
                           (h.restart_snapshots, "no restart schedule is set"),
                           (h.step_log_count, "no step log is set"),
                           (lambda: h.run_forced(1, 1, 1), "need flux records 0..0, resident are")):
            with pytest.raises(A.MckppHipError, match=what):
                call()
    # neither a resident bottom temperature nor a schedule of one has a query: the one-shot override is refused while
    # either is in place, so that it is accepted here says both are gone (every half applies it, the fresh context's too)
    h.bottomtemp(bt - 0.25)
    h.window_schedule(0, 1, 2, NREC, LAST, A.WIN_LAST)
    h.window_schedule(1, 1, 2, NREC, RED, A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX)
    h.window_export(0, "f8", 1e20)
    h.restart_schedule(1, 3, NSLOTS)
    h.step_log(LOG_CAP, 1)
    if variant == "resident":
        h.set_bottomtemp(bt)
    else:
        h.set_ancillary_series(A.ANC_BOTTOM_TEMP, 0, np.stack([bt, bt + 0.125]))
        h.ancillary_schedule(A.ANC_BOTTOM_TEMP, 1, 3, [0, 1])
    h.set_flux_series(0, series)
    for nt0, n in STEPS:
        h.run_forced(nt0, n, 1)
    assert h.window_records(0) == (0, 2) and h.restart_snapshots() == (0, 1)
    assert h.step_log_count()[0] == 6 * h.ncolumns
    exported = h.window_export_fetch(0, 2, "T", A.OP_LAST, np.zeros((NPTS, NZ + 1), order="F"))
    mean = h.window_record_fetch(1, 2, "difm", A.OP_MEAN, np.full((NPTS, NZ + 1), 1e20, order="F"))
    h.restart_snapshot_save(1, path)
    with open(path, "rb") as f:
        return exported.view(np.uint64).copy(), mean.view(np.uint64).copy(), f.read()


def _cycle(mk, cases, variant, path):
    h = mk.MckppHip(cases[0][0])
    _half(mk, h, cases[0], variant, path)
    got = _half(mk, h, cases[1], variant, path, unset=True)
    h.close()
    return got


@pytest.mark.parametrize("variant", ["resident", "series"])
def test_a_context_gives_back_what_it_was_given(mk, variant, tmp_path):
    import torch

    cases = [_case(e) for e in LAND]
    path = str(tmp_path / "snap.bin")
    fresh = mk.MckppHip(cases[1][0])
    want = _half(mk, fresh, cases[1], variant, path)
    fresh.close()
    got = _cycle(mk, cases, variant, path)
    for g, w, what in zip(got, want, ("exported record", "fetched mean", "snapshot file")):
        assert np.array_equal(g, w) if isinstance(g, np.ndarray) else g == w, what

    ncols = [int(np.count_nonzero(c[1].run_physics)) for c in cases]
    assert ncols == [300, 320]
    cycle = sum(_half_bytes(n) for n in ncols)
    assert cycle > 250 << 20   # (the blocks are large: the state itself and the code objects are small beside them)
    free = [torch.cuda.mem_get_info()[0]]
    for _ in range(2):
        for _ in range(4):
            _cycle(mk, cases, variant, path)
        free.append(torch.cuda.mem_get_info()[0])
    fell = [free[i] - free[i + 1] for i in range(2)]
    print(f"free device memory after the first cycle and after each batch of four cycles: {free}; a cycle asks for {cycle} bytes")
    # The bound is the loss of half a cycle's blocks in every cycle - what a state group that is not dropped gives.  It
    # is no detector of a single lost block: the step log alone (16 MB a half) or the snapshot slots alone (34 MB) pass.
    assert not all(f >= 4 * (cycle // 2) for f in fell), (fell, cycle)
