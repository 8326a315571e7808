"""kpp_driver flag 8192 (with 16): ndtocn = 2 and flux records that change with their number.  With flag 16384 the
records go through a flux ring of 2 slots (mckpp_hip_all_flux_ring, mckpp_hip_all_flux_ring_put) - two records put, the
forced run of their four steps, the next pair put while that run is queued - and must leave, byte for byte, the output
file of flag 8192 alone, whose records are all resident (mckpp_hip_all_set_flux_series) under one forced run.  On one
device and on three shards.  And the records do change the run: the output differs from that of flag 16 alone."""
import pytest

import common as cm
from harness import drive

pytestmark = pytest.mark.gpu


def _drive(tmp_path, name, kc, k3, sf, nsteps, flags, shards):
    return drive(tmp_path, name, kc, k3, sf, nsteps, flags, shards).read_bytes()


@pytest.mark.parametrize("shards,nz,nsteps", [(0, 60, 12), (3, 69, 10)])
def test_fortran_records_through_the_ring_equal_the_resident_series(built, tmp_path, shards, nz, nsteps):
    """12 steps: three pairs of records; 10 steps: the last call holds one record."""
    ncol = 211
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    series = _drive(tmp_path, "series", kc, k3, sf, nsteps, 16 + 8192, shards)
    ring = _drive(tmp_path, "ring", kc, k3, sf, nsteps, 16 + 8192 + 16384, shards)
    assert len(series) > 8 * ncol * kc.nzp1 * 4
    assert ring == series


def test_the_records_change_the_run(built, tmp_path):
    ncol, nz, nsteps = 211, 60, 12
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    sf = cm.synth.forcing(ncol, "bench")
    constant = _drive(tmp_path, "constant", kc, k3, sf, nsteps, 16, 0)
    changing = _drive(tmp_path, "changing", kc, k3, sf, nsteps, 16 + 8192, 0)
    assert len(constant) == len(changing) and constant != changing
