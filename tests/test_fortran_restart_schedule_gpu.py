"""kpp_driver flag 512: the time loop as ONE mckpp_hip_all_run_forced under a restart schedule of period 2
(mckpp_hip_all_restart_schedule), every snapshot written through mckpp_hip_all_restart_snapshot_save afterwards.  The
snapshot files must equal, byte for byte, those of the same calls on the Python path, and the run's final state too."""
import os
import subprocess

import numpy as np
import pytest

import common as cm
from test_fortran_host import DRIVER, _read_out, _write_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ncol,nz,shards,nsteps", [(2000, 40, 0, 6), (3001, 60, 3, 8), (2500, 69, 2, 7)])
def test_fortran_driver_writes_the_snapshots_of_the_python_path(built, tmp_path, ncol, nz, shards, nsteps):
    import mckpp_f90_amd as mk

    kc, k3 = cm.make_hip_case(ncol, nz, grid="stretched", land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    _write_case(tmp_path / "case.bin", kc, k3, sf, nsteps, 0, flags=512, shards=shards)
    out = tmp_path / "out.bin"
    r = subprocess.run([DRIVER, str(tmp_path / "case.bin"), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    got = _read_out(out, kc, ncol)
    ndev, nsnap = max(1, shards), nsteps // 2
    h = mk.MckppHipMulti(kc, [0] * ndev)
    h.upload(k3)
    h.init_ocean(0)
    series = np.zeros((1, 8, ncol))   # the driver's constant records: taux, swf, lhf, rain
    series[0, 0], series[0, 2], series[0, 4], series[0, 6] = 0.01, 200.0, -150.0, 6e-5
    h.set_flux_series(0, series)
    h.restart_schedule(1, 2, nsnap)
    h.run_forced(1, nsteps, nsteps + 1)
    assert h.restart_snapshots() == (0, nsnap - 1)
    for s in range(nsnap):
        h.restart_snapshot_save(s, tmp_path / f"py.rst{s}")
        for d in range(ndev):
            f = f"{out}.rst{s}.{d}of{ndev}"
            assert os.path.exists(f), f
            a, b = open(f, "rb").read(), open(tmp_path / f"py.rst{s}.{d}of{ndev}", "rb").read()
            assert len(a) > 64 and a == b, (s, d, len(a), len(b))
    assert not os.path.exists(f"{out}.rst{nsnap}.0of{ndev}")
    h.download(k3)
    h.close()
    for n in ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "old", "new_", "difm", "ghat", "rho"):
        assert np.array_equal(got[n], getattr(k3, n)), n
