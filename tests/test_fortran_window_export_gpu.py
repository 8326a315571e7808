"""kpp_driver flag 4096 with flag 256: the output schedule's records through its export (mckpp_hip_all_window_export,
mckpp_hip_all_window_export_fetch) - the steps as two forced runs, the second begun inside a window, the first run's
records fetched while the second is queued - must leave, byte for byte, the output file of flag 256 alone, whose records
come through mckpp_hip_all_window_record_fetch after one forced run.  On one device and on three shards."""
import subprocess

import pytest

import common as cm
from test_fortran_host import DRIVER, _write_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shards,nz", [(0, 60), (3, 69)])
def test_fortran_records_through_the_export_equal_the_record_fetch(built, tmp_path, shards, nz):
    ncol, nsteps = 211, 12
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    outs = []
    for name, flags in (("plain", 256 + 16), ("export", 256 + 16 + 4096)):
        case, out = tmp_path / f"{name}.case", tmp_path / f"{name}.out"
        _write_case(case, kc, k3, sf, nsteps, 0, flags=flags, shards=shards)
        r = subprocess.run([DRIVER, str(case), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        outs.append(out.read_bytes())
    # the state, then nsteps / 2 records of hmix(npts) and T(npts, nzp1)
    assert len(outs[0]) > 8 * (nsteps // 2) * ncol * (1 + kc.nzp1)
    assert outs[0] == outs[1]
