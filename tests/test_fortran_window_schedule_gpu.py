"""kpp_driver flag 256: the output of flag 32 (mean hmix, maximum T over windows of two steps) accumulated inside ONE
mckpp_hip_all_run_forced call under an output schedule (mckpp_hip_all_window_schedule), every record fetched with
mckpp_hip_all_window_record_fetch - on one device and on shards - against the C-ABI run step by step."""
import subprocess

import numpy as np
import pytest

import common as cm
from test_fortran_host import DRIVER, _read_out, _write_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shards,nz", [(0, 60), (2, 69), (3, 40)])
def test_fortran_forced_run_with_an_output_schedule(built, tmp_path, shards, nz):
    import mckpp_f90_amd as mk

    ncol, nsteps, period = 211, 4, 2
    nrec = nsteps // period
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    _write_case(tmp_path / "case.bin", kc, k3, sf, nsteps, 0, flags=256, shards=shards)
    r = subprocess.run([DRIVER, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    got = _read_out(tmp_path / "out.bin", kc, ncol)
    raw = (tmp_path / "out.bin").read_bytes()
    per_rec = ncol * (1 + kc.nzp1)
    tail = np.frombuffer(raw[len(raw) - 8 * nrec * per_rec:], dtype=np.float64)
    recs = []
    for w in range(nrec):
        blk = tail[w * per_rec:(w + 1) * per_rec]
        recs.append((blk[:ncol], blk[ncol:].reshape((ncol, kc.nzp1), order="F")))
    # the reference: the C-ABI, a step at a time, mckpp_fluxes with the forcing of the driver's flux record
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    cm.set_forcing_3d(k3, sf)
    one = np.ones(ncol)
    ocean = k3.run_physics != 0
    hm, tmax = None, None
    for nt in range(1, nsteps + 1):
        ctx.fluxes(nt, 0.01 * one, 0 * one, 200 * one, 0 * one, -150 * one, 0 * one, 6e-5 * one, 0 * one)
        mk.mckpp_physics_driver(k3, kc, nt, new_forcing=False)
        first = (nt - 1) % period == 0
        hm = np.zeros(ncol) + k3.hmix if first else hm + k3.hmix
        tmax = k3.X[:, :, 0].copy() if first else np.maximum(tmax, k3.X[:, :, 0])
        if nt % period == 0:
            w = nt // period - 1
            g_h, g_t = recs[w]
            assert np.array_equal(g_h[ocean], (hm / period)[ocean]) and np.all(g_h[~ocean] == -1), w
            assert np.array_equal(g_t[ocean], tmax[ocean]) and np.all(g_t[~ocean] == -1), w
    for n in ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "old", "new_", "difm", "ghat", "rho"):
        assert np.array_equal(got[n], getattr(k3, n)), n
