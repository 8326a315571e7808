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
    for tag in rc.REGIME_CASES:
        _regime_case_reaches_what_it_is_for(tag)



def _through(tag):
    """The oracle through a regime case: (paths of the last step, paths OR-ed over the steps, status of each step,
    the batch after the last step), over the ocean columns; T, S, U, V finite after every step."""
    case = rc.CASES[tag]
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
    act = rc.active_columns(case)
    seen, status = np.zeros(len(act), dtype=np.int32), []
    for nt in rc.run_oracle(case, oc, ob):
        for name in "TSUV":
            assert np.isfinite(rc.field_of(ob, name, case.nz)[act]).all(), f"{tag} step {nt}: {name} is not finite"
        assert not (ob["status"][act] & orc.ST_ZERO_PIVOT).any(), f"{tag} step {nt}: a zero pivot (the reference stops)"
        seen |= ob["paths"][act]
        status.append(ob["status"][act].copy())
    return ob["paths"][act], seen, status, ob, act


def _regime_case_reaches_what_it_is_for(tag):
    """The oracle's `paths` word (which branch a column took, OR-ed over its passes and retries) on the regime cases:
    conditions on the inputs, so that a bit-exact match on a case proves what the case's name says.  Where one is
    missed it is the case's inputs that change (denser ramp, shallower bathymetry), never the condition."""
    P = orc.PATHS
    case = rc.CASES[tag]
    last, seen, status, ob, act = _through(tag)
    n = len(act)

    def has(word, *names):
        return (word & sum(P[k] for k in names)) != 0

    if tag.startswith("seafloor_"):
        floor = has(last, "HBL_SEAFLOOR")
        assert floor.sum() >= 0.1 * n, f"{tag}: the sea floor clamps {floor.sum()} of {n} columns"
        assert np.array_equal(ob["hmix"][act][floor], -ob["ocdepth"][act][floor])
    if tag == "seafloor_edges_nz40":
        d = -ob["ocdepth"][act]
        for edge in rc.SEAFLOOR_EDGES:      # every edge value clamps at least one column
            assert has(last, "HBL_SEAFLOOR")[d == edge].any(), edge
        assert (ob["kmix"][act][d < 2.5] == 2).all() and has(seen, "HBL_SECOND_MIN").any()
    if "fulldepth" in tag:
        bottom = has(last, "HBL_NO_HIT") & (ob["kmix"][act] >= case.nz)
        assert bottom.sum() >= 0.1 * n, f"{tag}: {bottom.sum()} of {n} columns mix down to the last level"
    if tag.startswith("tjump_"):
        assert (has(seen, "TRAP_TJUMP") & ~has(seen, "TRAP_U")).sum() >= 5
        want = orc.ST_RETRIED | orc.ST_FAILED
        assert ((status[0] & want) == want).sum() >= 5
    if tag == "rms_retry_thin_grid":
        rms = has(seen, "TRAP_RMS_U", "TRAP_RMS_V", "TRAP_RMS_T", "TRAP_RMS_S")
        assert (rms & ~has(seen, "TRAP_U", "TRAP_TJUMP")).sum() >= 5
        assert sum(bool(has(seen, k).any()) for k in ("TRAP_RMS_U", "TRAP_RMS_V", "TRAP_RMS_T", "TRAP_RMS_S")) >= 2
        assert any((((st & orc.ST_RETRIED) != 0) & ((st & orc.ST_FAILED) == 0)).any() for st in status), \
            "no column is retried and then accepted"
    if tag == "ssref0_nz40":
        assert np.array_equal(ob["Ssurf"][act], (ob["S"][:, 1] + ob["Sref"])[act])
        assert not np.array_equal(ob["Ssurf"][act], ob["SSref"][act])
    if tag == "ldd_diffconv_nz40":
        assert has(last, "DD_DIFFCONV").sum() >= 0.1 * n and has(seen, "DD_FINGER").any()
    if tag == "regime_sweep_nz60":
        missing = [k for k in P if not has(seen, k).any()]
        assert not missing, f"the sweep never takes {missing}"
