"""kpp_driver under ancillary schedules (flag 2048): L_RELAX_SST and L_RELAX_OCNT with SST0 changing every 3 steps and
ocnT_clim, interpolated between two records, every 2.  With flag 16 the time loop is ONE mckpp_hip_all_run_forced that
reads the fields from resident series (mckpp_hip_all_set_ancillary_series, mckpp_hip_all_ancillary_schedule); with flag
1 it is the per-step driver, which forms the same fields on the host and sends them with mckpp_hip_push_ancillaries at
those cadences.  The two are held to equality, on one device and on three shards."""
import numpy as np
import pytest

import common as cm
from harness import drive
from test_fortran_host import _read_out

pytestmark = pytest.mark.gpu

OUT = ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "old", "new_", "difm", "ghat", "rho")


@pytest.mark.parametrize("shards", [0, 3])
def test_one_forced_run_under_schedules_equals_the_per_step_driver(built, tmp_path, shards):
    ncol, nz, nsteps = 77, 40, 12
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    one = _read_out(drive(tmp_path, "one", kc, k3, sf, nsteps, 2048 + 16, shards), kc, ncol)
    per_step = _read_out(drive(tmp_path, "per_step", kc, k3, sf, nsteps, 2048 + 1, shards), kc, ncol)
    for n in OUT:
        assert np.array_equal(one[n], per_step[n]), n
    # reach: without the relaxations the same forced run ends elsewhere, on every ocean column
    plain = _read_out(drive(tmp_path, "plain", kc, k3, sf, nsteps, 16, shards), kc, ncol)
    act = np.nonzero(k3.run_physics)[0]
    assert np.all(np.any(plain["X"][act, :, 0] != one["X"][act, :, 0], axis=1))
