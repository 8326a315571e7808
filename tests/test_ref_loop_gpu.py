"""The HIP paths against the reference's OWN init, flux assembly and time loop, as recorded in
tests/golden/ref_loop.npz from the portable-exp build of the compiled reference (tests/ref_loop_cases.py,
tests/golden/make_ref_loop_golden.py) - bit for bit.  Reads the golden file only, never the reference.

What the record holds and no device call returns: tri(:,0:1,1) - the library's host side builds it for
KppConstFields, where it is checked (here, and without a GPU in tests/test_ref_loop_cpu.py).  Every other recorded
field comes back through mckpp_hip_download.  mckpp_initialize_fluxes has no device counterpart (the caller hands
over sflux = 1e-20 and zeroed flux arrays, as tests/common.py's make_hip_case does)."""
import numpy as np
import pytest

import ref_loop_cases as lc
from harness import assert_loop_step, flux_args, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401

pytestmark = pytest.mark.gpu


def _resident(mk, tag):
    """(context, KppConstFields, Kpp3dFields): the raw columns of the case uploaded and initialised on the device"""
    return resident(mk, lc.CASES[tag])


@pytest.mark.parametrize("tag", list(lc.CASES))
def test_init_fluxes_and_steps_one_by_one(mk, golden, tag):
    """mckpp_initialize_ocean_model, then per step mckpp_hip_fluxes at the update steps (record (nt-1)//ndtocn),
    mckpp_hip_step(nt, 1) and a download: every recorded field after init and after every step."""
    case = lc.CASES[tag]
    kc, k3 = lc.hip_raw(case)
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    bad = lc.mismatches(case, lc.INIT_FIELDS, golden.init_sha(tag, "pexp"), lc.hip_get(k3, kc, case.nz))
    assert not bad, f"{tag} after init: differs from the recorded reference: {bad}"
    rec = lc.flux_records(case)
    for nt in range(1, case.nsteps + 1):
        if (nt - 1) % case.ndtocn == 0:
            ctx.fluxes(nt, **dict(zip(lc.FLUX_NAMES, rec[(nt - 1) // case.ndtocn])), **flux_args(case))
        ctx.step(nt, 1)
        ctx.download(k3)
        assert_loop_step(golden, tag, nt, k3, kc, "fluxes + step")


@pytest.mark.parametrize("tag", list(lc.CASES))
def test_forced_run_in_one_launch(mk, golden, tag):
    """set_flux_series + run_forced(1, nsteps, ndtocn) as one launch: the state after the last step."""
    case = lc.CASES[tag]
    h, kc, k3 = _resident(mk, tag)
    h.set_flux_series(0, lc.flux_records(case))
    h.run_forced(1, case.nsteps, case.ndtocn, **flux_args(case))
    assert h.last_launch_count() == 1
    h.download(k3)
    assert_loop_step(golden, tag, case.nsteps, k3, kc, "one launch")


# cases with a step nd + 1 inside their second flux interval to split at; and, of those, the ones whose second call
# still has an update to make (from record 2 on)
SPLIT = [(t, False) for t, c in lc.CASES.items() if c.ndtocn > 1 and c.nsteps > c.ndtocn + 1]
SPLIT += [(t, True) for t, _ in SPLIT if lc.nrec(lc.CASES[t]) > 2]


@pytest.mark.parametrize("tag,later_records_only", SPLIT)
def test_forced_run_split_inside_a_flux_interval(mk, golden, tag, later_records_only):
    """The same in two calls whose boundary is not an update step: the sflux rows of the interval under way must
    stay put across the calls.  later_records_only: before the second call the series is replaced by the records
    that call still updates from (rec0 > 0) - the record of the interval under way is then not even resident."""
    case = lc.CASES[tag]
    nd = case.ndtocn
    first = nd + 1                                   # the second call starts at step nd + 2: (nd + 1) % nd != 0
    assert first < case.nsteps and first % nd != 0
    rec = lc.flux_records(case)
    h, kc, k3 = _resident(mk, tag)
    h.set_flux_series(0, rec)
    h.run_forced(1, first, nd, **flux_args(case))
    h.download(k3)
    assert_loop_step(golden, tag, first, k3, kc, "first of two calls")
    if later_records_only:
        rec0 = (first + nd - 1) // nd                # the first update of steps first+1 ..
        assert 0 < rec0 < len(rec)
        h.set_flux_series(rec0, rec[rec0:])
    h.run_forced(first + 1, case.nsteps - first, nd, **flux_args(case))
    h.download(k3)
    assert_loop_step(golden, tag, case.nsteps, k3, kc, "second of two calls")


def test_forced_run_through_the_multi_handle(mk, golden):
    """One case through MckppHipMulti with 3 shards on the one device (as tests/test_multi_gpu.py does)."""
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    kc, k3 = lc.hip_raw(case)
    m = mk.MckppHipMulti(kc, [0, 0, 0])
    m.upload(k3)
    m.init_ocean(0)
    m.download(k3)
    bad = lc.mismatches(case, lc.INIT_FIELDS, golden.init_sha(tag, "pexp"), lc.hip_get(k3, kc, case.nz))
    assert not bad, f"{tag} after init, 3 shards: differs from the recorded reference: {bad}"
    m.set_flux_series(0, lc.flux_records(case))
    m.run_forced(1, case.nsteps, case.ndtocn, **flux_args(case))
    m.synchronize()
    m.download(k3)
    assert_loop_step(golden, tag, case.nsteps, k3, kc, "3 shards")
    m.close()
