"""The oracle against the reference's OWN physics step (oracle/ref_step_shim.F90 over the reference's sources, built
by oracle/Makefile target `ref`): ocnstep with its label-45 iteration, trap and retries, vertical mixing (bldepth,
wscale, rimix, blmix, enhance, ddmix, kppmix), ocnint and the tridiagonal solver, check_profile and the overrides, on
the cases of tests/ref_step_cases.py - bit for bit, on every field after every step.

Against the recorded outputs (tests/golden/ref_step.npz) always, and against the live reference where
oracle/_ref/libmckpp_ref_step*.so were built: exp_mode=0 against the libm build, exp_mode=1 against the
portable-exp build."""
import numpy as np
import pytest

import ref_step_cases as rc
from oracle import orc

BUILDS = {"libm": 0, "pexp": 1}


@pytest.fixture(scope="module")
def golden(built):
    return rc.Golden()


def _batch_get(ob, nz):
    return lambda name: rc.field_of(ob, name, nz)


def test_every_case_is_recorded(golden):
    assert golden.cases() == sorted(rc.CASES)
    for tag, case in rc.CASES.items():
        for b in BUILDS:
            assert golden.digests(tag, b).shape == (case.nsteps, len(rc.STEP_FIELDS), 32), (tag, b)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tag", list(rc.CASES))
def test_oracle_matches_the_reference_step(golden, tag, build):
    case, em = rc.CASES[tag], BUILDS[build]
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=em)
    assert np.array_equal(rc.input_digest(ob), golden.input_sha(tag, build)), \
        f"{tag}: the seeded starting state is not the recorded one (tests/common.py or synth changed?)"
    live = rc.run_reference(case, oc, ob, em) if orc.have_ref_step() else None
    values = golden.values(tag) if build == "pexp" else {}
    for nt in rc.run_oracle(case, oc, ob):
        bad = rc.mismatches(case, golden.digests(tag, build), values, nt, _batch_get(ob, case.nz))
        assert not bad, f"{tag} ({build} exp) step {nt}: oracle differs from the recorded reference: {bad}"
        if live is not None:
            r = live[nt - 1]
            for name in rc.STEP_FIELDS:
                a = rc.canonical(rc.field_of(ob, name, case.nz))[rc.active_columns(case)]
                b = rc.canonical(rc.field_of(r, name, case.nz))[rc.active_columns(case)]
                assert np.array_equal(a.view(np.int64), b.view(np.int64)), \
                    f"{tag} ({build} exp) step {nt}: {name} differs from the live reference"


def test_the_cases_reach_what_they_are_for(golden):
    """The recorded cases take the paths they are named after (else a bit-exact match proves less than it says)."""
    def last(tag):
        case = rc.CASES[tag]
        oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
        ob.most_passes, ob.status_seen = 0, np.zeros(case.ncol, dtype=np.int32)
        for _ in rc.run_oracle(case, oc, ob):
            ob.most_passes = max(ob.most_passes, int(ob["npasses"].max()))
            ob.status_seen |= ob["status"]
        return ob

    ob = last("nz40_diurnal_itermax")
    assert ob.most_passes >= rc.CASES["nz40_diurnal_itermax"].switches["itermax"]
    ob = last("nz40_trap_retry")
    assert (ob.status_seen & orc.ST_RETRIED).any()
    ob = last("nz40_trap_clim_reset")
    assert (ob.status_seen & orc.ST_FAILED).any()
    ob = last("nofreeze_isotherm_clim")
    assert (ob["freeze_flag"] > 0).any() and (ob["reset_flag"] != 0).any()
    ob = last("damp_curr")
    assert ((ob["dampu_flag"] != 0) | (ob["dampv_flag"] != 0)).any()
    ob = last("relax_sst")
    assert (ob["fcorr"] != 0).any()
