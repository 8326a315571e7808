"""Lean steps: inside a launch of several steps a column-step stores "what the last vmix leaves behind" (rho, cp, buoy,
talpha, sbeta, Rig, dbloc, Shsq, difm, difs, dift, ghat, wU, wX, wXNT) only if something can read it before the
column's next step overwrites it - the launch's last step, a snapshot step of the restart schedule, or every step when
an output schedule holds a diagnostic field or a bottom temperature is resident or scheduled.  What the host, the
records and the snapshots see must be what a launch per step leaves, bit for bit; MCKPP_LEAN_DIAG=0 stores every step's
diagnostics as before.

Every comparison is between two contexts built from the same host fields.  The host's diagnostic arrays are filled with
a sentinel before upload: upload does not carry diagnostics (the device rows start zeroed), so the sentinel guards the
host elements that no download writes, and an element of a device row that is stored in some steps only - an earlier
step of the per-step context writes it, the last one does not - shows as a difference against the one-launch context,
which still holds there what the spin-up left (or zero)."""
import numpy as np
import pytest

import common as cm
from harness import cleared, mk  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
SPINUP = 3
DIAG_ARRAYS = ("rho", "cp", "buoy", "difm", "difs", "dift", "wU", "wX", "wXNT", "ghat", "Rig", "Shsq", "dbloc")
ENV = ("MCKPP_MULTISTEP", "MCKPP_PS_FIXED_L", "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT", "MCKPP_L3_CAP")
_clean_env = cleared(ENV)


def _context(mk, ncol=2000, nz=40, physics="default", solver_mode=0, trap=False, spinup=SPINUP):
    """A context with the bench forcing mix and every seventh point land, after `spinup` steps in one launch; the next
    step is spinup + 1.  trap: no spin-up, and every seventh column (not a land one) starts with the currents that
    tests/test_parity_gpu.py uses to make the instability trap retry."""
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=7)
    if physics == "relax":   # optional physics: SST and salinity relaxation
        kc.L_RELAX_SST = 1
        kc.L_RELAX_SAL = 1
        k3.relax_sst[:] = 1.0 / (5.0 + np.arange(ncol) % 11)
        k3.SST0[:] = np.asarray(k3.X[:, 0, 0]) - 0.5
        k3.relax_sal[:] = 2.0 / (30 * 86400.0)
        k3.sal_clim[...] = np.asarray(k3.X[:, :, 1]) + 0.05
    if physics == "ldd":     # double diffusion, salt fingers under every other column
        kc.LDD = 1
        k3.X[::2, :, 1] = 0.4 - 0.8 * np.linspace(0, 1, kc.nzp1)[None, :]
    for n in DIAG_ARRAYS:
        getattr(k3, n)[...] = SENTINEL
    h = mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    if solver_mode:
        h.set_solver_mode(solver_mode)
    bad = np.arange(3, ncol, 7)
    if trap:
        h.download(k3)
        k3.U[bad, 0:4, 0] = 50.0
        h.upload(k3)
    cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
    h.set_forcing(k3.sflux)
    if trap:
        return h, kc, k3, 1
    if physics != "default":
        assert h.kernel_name == "k_column_ps<EXT>"
    h.step(1, spinup)
    return h, kc, k3, spinup + 1


def _end_state(h, k3):
    """every array of download(F_ALL), the status words and the pass counts"""
    h.download(k3)
    st, nf, npass = h.status()
    out = {n: np.array(v, copy=True) for n, v in vars(k3).items() if isinstance(v, np.ndarray)}
    out["status()"], out["npass()"], out["nflagged()"] = st.copy(), npass.copy(), np.array([nf])
    return out


def _same(a, b, what):
    assert a.keys() == b.keys() and "wX" in a and "Rig" in a and "Xs" in a
    bad = [n for n in a if not (a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes())]
    assert not bad, f"{what}: fields that differ: {bad}"


def _one_launch_against_a_launch_per_step(mk, n, **case):
    a, _, k3a, nt = _context(mk, **case)
    b, _, k3b, _ = _context(mk, **case)
    a.step(nt, n)
    assert a.last_launch_count() == 1
    first = None
    for i in range(n):
        b.step(nt + i, 1)
        if first is None:
            first = b.status()[0].copy()
    ea, eb = _end_state(a, k3a), _end_state(b, k3b)
    _same(ea, eb, f"step({nt}, {n}) against {n} launches of one step, {case}")
    # the diagnostics are there at all (not the sentinel, not all zero) and the sentinel survives where nothing downloads
    ocean = np.nonzero(k3a.run_physics)[0]
    assert np.all(ea["rho"][ocean, 1] > 1000.0) and np.any(ea["difm"][ocean, 1:5] > 0.0) and np.any(ea["wX"][ocean, 1, 0] != 0.0)
    assert np.all(ea["rho"][k3a.run_physics == 0] == SENTINEL)
    a.close()
    b.close()
    return first


@pytest.mark.parametrize("solver_mode", [0, 1])
@pytest.mark.parametrize("nz", [40, 60])
def test_identity_default_physics(mk, nz, solver_mode):
    """step(nt, 6) in one launch against six launches: every field of download(F_ALL), status() and the pass counts,
    bit for bit, sentinels included; 2,000 columns (more than the slots of the workgroups: refill rounds, hand-overs)."""
    _one_launch_against_a_launch_per_step(mk, 6, nz=nz, solver_mode=solver_mode)


@pytest.mark.parametrize("physics", ["relax", "ldd"])
def test_identity_optional_physics(mk, physics):
    """The EXT kernel build: SST and salinity relaxation on (rho cp enters the right-hand sides; the full equation of
    state runs whatever the step's kind), and double diffusion (alpha and beta feed the pass)."""
    _one_launch_against_a_launch_per_step(mk, 5, physics=physics)


def test_identity_general_kernels(mk, monkeypatch):
    """MCKPP_PS_FIXED_L=0: the kernels that take the level count at run time."""
    monkeypatch.setenv("MCKPP_PS_FIXED_L", "0")
    _one_launch_against_a_launch_per_step(mk, 5)


def test_identity_with_a_trap_retry(mk):
    """Columns that the instability trap retries in the first step of the launch (a lean step: the retry keeps the
    step's kind), with the start that tests/test_parity_gpu.py uses for the trap."""
    first = _one_launch_against_a_launch_per_step(mk, 5, trap=True)
    bad = np.arange(3, 2000, 7)
    assert np.all(first[bad] & 4 == 4), "the trap did not fire where it was set up"


def _fetch_all(h, A, ncol, nzp1, sched, nrec, fields, op):
    return {(w, n): h.window_record_fetch(sched, w, n, op, np.full((ncol, nzp1), -7.0, order="F")).copy()
            for w in range(nrec) for n in fields}


@pytest.mark.parametrize("fields", [("difm", "wT"), ("T",)], ids=["diagnostic_fields", "T_only"])
def test_window_records_equal_those_with_every_step_stored(mk, monkeypatch, fields):
    """Mean over windows of 3 steps in a launch of 7: a schedule with a diagnostic field makes every step of the launch
    a diagnostic step; one over T alone leaves the steps lean.  Either way the records, and the end state, are those of
    MCKPP_LEAN_DIAG=0."""
    A = mk.api
    got = {}
    for lean in ("1", "0"):
        monkeypatch.setenv("MCKPP_LEAN_DIAG", lean)
        h, kc, k3, nt = _context(mk)
        h.window_schedule(0, nt, 3, 3, fields, A.WIN_MEAN)
        h.step(nt, 7)
        assert h.last_launch_count() == 1 and h.window_records(0) == (0, 1)
        got[lean] = (_fetch_all(h, A, 2000, kc.nzp1, 0, 2, fields, A.OP_MEAN), _end_state(h, k3))
        h.close()
    assert got["1"][0].keys() == got["0"][0].keys() and len(got["1"][0]) == 2 * len(fields)
    for key in got["1"][0]:
        r1, r0 = got["1"][0][key], got["0"][0][key]
        assert r1.tobytes() == r0.tobytes(), key
        assert np.any(r1[np.nonzero(k3.run_physics)[0]] != -7.0), key
    _same(got["1"][1], got["0"][1], f"end state under a window schedule over {fields}")


def test_snapshots_whose_period_does_not_divide_the_launch(mk, monkeypatch, tmp_path):
    """restart_schedule(nt, 3, 2) under a launch of 7 steps: snapshots after the third and the sixth step, neither the
    launch's last; their files are byte for byte those of MCKPP_LEAN_DIAG=0 (the set carries the rho and cp rows)."""
    files = {}
    for lean in ("1", "0"):
        monkeypatch.setenv("MCKPP_LEAN_DIAG", lean)
        h, kc, k3, nt = _context(mk)
        h.restart_schedule(nt, 3, 2)
        h.step(nt, 7)
        assert h.last_launch_count() == 1 and h.restart_snapshots() == (0, 1)
        for s in range(2):
            files[lean, s] = tmp_path / f"snap{s}_lean{lean}"
            h.restart_snapshot_save(s, files[lean, s])
        files[lean, "end"] = _end_state(h, k3)
        h.close()
    for s in range(2):
        g, r = open(files["1", s], "rb").read(), open(files["0", s], "rb").read()
        assert len(g) > 64 and g == r, f"snapshot {s}"
    assert open(files["1", 0], "rb").read() != open(files["1", 1], "rb").read()
    _same(files["1", "end"], files["0", "end"], "end state under a restart schedule")


def test_resident_bottom_temperature(mk, monkeypatch):
    """The override reads rho and cp of each step's last vmix: with a bottom temperature resident every step of a
    5-step launch is a diagnostic step, and the end state is that of MCKPP_LEAN_DIAG=0 and of a launch per step."""
    end = {}
    for tag, lean, per_step in (("lean", "1", False), ("every", "0", False), ("per_step", "1", True)):
        monkeypatch.setenv("MCKPP_LEAN_DIAG", lean)
        h, kc, k3, nt = _context(mk)
        bt = np.asarray(k3.X[:, kc.nzp1 - 1, 0]) - 0.5 + 0.25 * np.sin(np.arange(2000))
        h.set_bottomtemp(bt)
        if per_step:
            for i in range(5):
                h.step(nt + i, 1)
        else:
            h.step(nt, 5)
        end[tag] = _end_state(h, k3)
        h.close()
    _same(end["lean"], end["every"], "bottom temperature, against MCKPP_LEAN_DIAG=0")
    _same(end["lean"], end["per_step"], "bottom temperature, against a launch per step")
    ocean = np.nonzero(k3.run_physics)[0]   # the override did act: T(nzp1) is the bottom temperature
    assert np.array_equal(end["lean"]["X"][ocean, kc.nzp1 - 1, 0], bt[ocean])


def test_switch(mk, monkeypatch):
    """MCKPP_LEAN_DIAG=0 against the default (unset, or any other value), the same launch of 6 steps: all fields
    identical."""
    end = {}
    for lean in (None, "0"):
        if lean is None:
            monkeypatch.delenv("MCKPP_LEAN_DIAG", raising=False)
        else:
            monkeypatch.setenv("MCKPP_LEAN_DIAG", lean)
        h, kc, k3, nt = _context(mk)
        h.step(nt, 6)
        assert h.last_launch_count() == 1
        end[lean] = _end_state(h, k3)
        h.close()
    _same(end[None], end["0"], "MCKPP_LEAN_DIAG=0 against the default")


def test_headline_sample(mk):
    """4,096 columns x 60 levels, 6 steps in one call after the 3 spin-up steps, against the per-step path."""
    _one_launch_against_a_launch_per_step(mk, 6, ncol=4096, nz=60)
