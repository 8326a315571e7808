"""kpp_driver with L_VARY_BOTTOM_TEMP (flag 2) and its time loop as ONE mckpp_hip_all_run_forced (flags 16, 512): the
session makes kpp_3d_fields%bottom_temp resident before the run, so that every step of the launch ends with
mckpp_physics_overrides_bottomtemp as the per-step mckpp_physics_driver's does.

The forced run's forcing is what mckpp_fluxes assembles from the driver's constant records, so the per-step run it is
held to is flags 2 + 1 (mckpp_fluxes every step, then mckpp_physics_driver with its override after the launch): flag 2
alone steps with the case file's own sflux, which is another forcing."""
import os

import numpy as np
import pytest

import common as cm
from harness import drive
from test_fortran_host import _read_out

pytestmark = pytest.mark.gpu

OUT = ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "old", "new_", "difm", "ghat", "rho")


@pytest.mark.parametrize("shards", [0, 3])
def test_one_forced_run_equals_the_per_step_driver(built, tmp_path, shards):
    ncol, nz, nsteps = 77, 40, 4
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    one = _read_out(drive(tmp_path, "one", kc, k3, sf, nsteps, 2 + 16, shards), kc, ncol)
    per_step = _read_out(drive(tmp_path, "per_step", kc, k3, sf, nsteps, 2 + 1, shards), kc, ncol)
    for n in OUT:
        assert np.array_equal(one[n], per_step[n]), n
    act = np.nonzero(k3.run_physics)[0]
    assert np.array_equal(one["X"][act, nz, 0], np.asarray(k3.X[act, nz, 0]) + 0.125)   # the driver's bottom_temp
    # ... and without the switch the same forced run ends elsewhere
    plain = _read_out(drive(tmp_path, "plain", kc, k3, sf, nsteps, 16, shards), kc, ncol)
    assert not np.array_equal(plain["X"], one["X"])


@pytest.mark.parametrize("shards", [0, 3])
def test_snapshots_carry_the_override(built, tmp_path, shards):
    """flags 2 + 512: every snapshot file equals the C-ABI's of the same run, byte for byte."""
    import mckpp_f90_amd as mk

    ncol, nz, nsteps = 77, 40, 4
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    out = drive(tmp_path, "snap", kc, k3, sf, nsteps, 2 + 512, shards)
    got = _read_out(out, kc, ncol)
    ndev, nsnap = max(1, shards), nsteps // 2
    bt = np.asarray(k3.X[:, nz, 0]) + 0.125
    h = mk.MckppHipMulti(kc, [0] * ndev)
    h.upload(k3)
    h.init_ocean(0)
    series = np.zeros((1, 8, ncol))   # the driver's constant records: taux, swf, lhf, rain
    series[0, 0], series[0, 2], series[0, 4], series[0, 6] = 0.01, 200.0, -150.0, 6e-5
    h.set_flux_series(0, series)
    h.restart_schedule(1, 2, nsnap)
    h.set_bottomtemp(bt)
    h.run_forced(1, nsteps, nsteps + 1)
    for s in range(nsnap):
        h.restart_snapshot_save(s, tmp_path / f"py.rst{s}")
        for d in range(ndev):
            f = f"{out}.rst{s}.{d}of{ndev}"
            assert os.path.exists(f), f
            a, b = open(f, "rb").read(), open(tmp_path / f"py.rst{s}.{d}of{ndev}", "rb").read()
            assert len(a) > 64 and a == b, (s, d, len(a), len(b))
    h.download(k3)
    h.close()
    for n in OUT:
        assert np.array_equal(got[n], getattr(k3, n)), n
    act = np.nonzero(k3.run_physics)[0]
    assert np.array_equal(got["X"][act, nz, 0], bt[act])
