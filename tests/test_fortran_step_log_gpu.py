"""kpp_driver flag 1024: the time loop as ONE mckpp_hip_all_run_forced under a step log (mckpp_hip_all_step_log) of
ncol * nsteps records.  With itermax = 4 (flag 128) the run must write the reference's located warning for every
flagged column-step of the run - not only of its last step - in (time step, point) order; without the log the same
run writes none, as before."""
import re
import subprocess

import numpy as np
import pytest

import common as cm
from test_fortran_host import DRIVER, _read_out, _write_case

pytestmark = pytest.mark.gpu

NCOL, NZ, NSTEPS = 120, 40, 3


def _long_iteration_lines(stderr):
    """(step, point) of every "long iteration at timestep" warning, parsed as
    test_fortran_host.py::test_fortran_layer_writes_the_located_warnings parses them."""
    lines = [ln.strip() for ln in stderr.splitlines()]
    seen = []
    for i, ln in enumerate(lines):
        m = re.match(r"long iteration at timestep\s+(\d+)\s+location = \(\s*([-0-9.Ee+]+)\s*,\s*([-0-9.Ee+]+)\s*\)", ln)
        if m:
            assert lines[i - 1] == "Warning in MCKPP_PHYSICS_OCNSTEP:"
            ipt = round(float(m.group(2)) / 0.5)
            assert abs(float(m.group(3)) - (-60 + 0.25 * ipt)) < 1e-9
            assert re.search(r"passes =\s+\d+", lines[i + 2]) and re.search(rf"ipt =\s+{ipt}$", lines[i + 2])
            seen.append((int(m.group(1)), ipt))
    return seen


@pytest.fixture(scope="module")
def stepwise(built):
    """(step, point) of every flagged column-step, from a status read after each step of a step-by-step forced run on
    the driver's constant records, and the end state of that run."""
    import mckpp_f90_amd as mk

    kc, k3 = cm.make_hip_case(NCOL, NZ)
    kc.itermax = 4
    h = mk.MckppHip(kc)
    h.upload(k3)
    h.init_ocean(0)
    series = np.zeros((1, 8, NCOL))   # the driver's constant records: taux, swf, lhf, rain
    series[0, 0], series[0, 2], series[0, 4], series[0, 6] = 0.01, 200.0, -150.0, 6e-5
    h.set_flux_series(0, series)
    want = []
    for nt in range(1, NSTEPS + 1):
        h.run_forced(nt, 1, NSTEPS + 1)
        st, nf, npass = h.status()
        want += [(nt, int(i) + 1) for i in np.nonzero(st & 2)[0]]
    h.download(k3)
    h.close()
    assert any(nt < NSTEPS for nt, _ in want), "no column ran beyond itermax+1 passes before the last step"
    return want, k3


@pytest.mark.parametrize("shards", [0, 3])
def test_fortran_forced_run_writes_the_warnings_of_every_step(built, tmp_path, stepwise, shards):
    want, k3_end = stepwise
    kc, k3 = cm.make_hip_case(NCOL, NZ)
    _write_case(tmp_path / "case.bin", kc, k3, cm.synth.forcing(NCOL, "bench"), NSTEPS, 0, flags=128 + 16 + 1024, shards=shards)
    r = subprocess.run([DRIVER, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _long_iteration_lines(r.stderr) == want
    assert "were not recorded" not in r.stderr
    got = _read_out(tmp_path / "out.bin", kc, NCOL)
    for n in ("U", "X", "hmix", "kmix", "Tref"):
        assert np.array_equal(got[n], getattr(k3_end, n)), n


def test_fortran_forced_run_without_the_log_is_unchanged(built, tmp_path, stepwise):
    want, k3_end = stepwise
    kc, k3 = cm.make_hip_case(NCOL, NZ)
    _write_case(tmp_path / "case.bin", kc, k3, cm.synth.forcing(NCOL, "bench"), NSTEPS, 0, flags=128 + 16)
    r = subprocess.run([DRIVER, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _long_iteration_lines(r.stderr) == [] and "long iteration" not in r.stderr
    got = _read_out(tmp_path / "out.bin", kc, NCOL)
    for n in ("U", "X", "hmix", "kmix", "Tref"):
        assert np.array_equal(got[n], getattr(k3_end, n)), n
