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
from harness import step_golden as golden  # noqa: F401
from oracle import orc

BUILDS = {"libm": 0, "pexp": 1}


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
    _advection_cases_reach_what_they_are_for(golden)
    _precedence_and_trap_v_cases_reach_what_they_are_for()


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


@pytest.mark.parametrize("grid", ["uniform_90", "thin"])
def test_oracle_mode_4_without_a_level_below_100_m_adds_nothing(built, grid):
    """Mode 4's search for the first level below 100 m has no bound in the reference (solvers.F90:258-259): on a grid
    without such a level it has no defined behaviour, and no such input is recorded.  The oracle stops at nzp1, as the
    column kernel does: the range is empty, the step is that of a column without advection."""
    import common as cm

    ncol, nz = 12, 12
    out = []
    for adv in (True, False):
        oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid)
        assert oc.zm[nz + 1] >= -100.0
        if adv:
            rc._apply_batch(ob, nz + 1, rc.advection_inputs(ncol, lambda c: ((4, 4), 2)))
        orc.init_ocean(oc, ob, 0)
        ob["sflux"] = cm.synth.forcing(ncol, "bench")
        for nt in (1, 2):
            orc.physics_driver(oc, ob, nt)
        out.append(ob)
    for name in rc.STEP_FIELDS:
        assert np.array_equal(rc.canonical(rc.field_of(out[0], name, nz)), rc.canonical(rc.field_of(out[1], name, nz)), equal_nan=True), name


def advection_range(mode, km, nz, zm, hm, dm):
    """What rhsmod (src/mckpp_physics_solvers.F90:223-331) does with `mode` when the mixed layer ends in level km, in
    plain Python on the Fortran-indexed grid: (n1, n2, met, depth) - the levels n1 .. n2 the term is spread over (n1 >
    n2: none) and, for modes 6 and 7, whether the running depth met dmax (else the loop ran to nzi = nz) and that depth
    as the loop left it; for mode 4, n1 is the first level below 100 m."""
    if mode == 1:
        return 1, 1, None, None
    if mode == 2:
        return 1, km - 1, None, None
    if mode == 3:
        return 1, nz, None, None
    if mode == 4:
        n1 = 1
        while zm[n1] >= -100.0:
            n1 += 1                      # (no case has mode 4 on a grid where this leaves zm(1:nz+1))
        return n1, nz - 1, None, None
    if mode == 5:
        return nz, nz, None, None
    if mode == 6:
        n1, depth, dmax = 1, hm[1], dm[km] - 0.5 * (hm[km] + hm[km - 1])
    else:
        assert mode == 7
        n1, depth, dmax = km - 1, dm[km] - 0.5 * hm[km], 100.0
    for n in range(n1, nz + 1):
        depth = depth + hm[n + 1]
        if depth >= dmax:
            return n1, n, True, depth
    return n1, nz, False, depth


def _advection_ranges(tag):
    """[(step, column, slot, mode, km, n1, n2, met, depth)] of the live slots with a positive mode on the ocean columns of an
    advection case, km being the recorded kmix after the step; and the grid."""
    case = rc.CASES[tag]
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
    nz = case.nz
    assert oc.zm[nz + 1] < -100.0 or not (ob["modeadv"][:, 1, :] == 4).any(), f"{tag}: mode 4 with no level below 100 m"
    out = []
    for nt in rc.run_oracle(case, oc, ob):
        for c in rc.active_columns(case):
            km = int(ob["kmix"][c])
            assert 2 <= km <= nz, f"{tag}: kmix = {km}: dm(km), hm(km-1) would lie outside the reference's arrays"
            for j in range(int(ob["nmodeadv"][c, 1])):
                mode = int(ob["modeadv"][c, 1, j])
                if mode > 0:
                    assert ob["advection"][c, 1, j] != 0.0
                    n1, n2, met, depth = advection_range(mode, km, nz, oc.zm, oc.hm, oc.dm)
                    assert 1 <= n1 and n2 <= nz, (tag, mode, km, n1, n2)       # rhs(n1:n2) inside rhs(1:nz+1)
                    out.append((nt, int(c), j, mode, km, n1, n2, met, depth))
    return out, oc, ob


def _advection_cases_reach_what_they_are_for(golden):
    """Every mode, slot pattern and level-range edge the advection cases are named after really occurs on a column
    the reference steps, the ranges recomputed in plain Python from the recorded kmix and the grid."""
    for tag in ("adv_modes_nz40", "adv_modes_nz60", "adv_modes_nz60_index1", "adv_modes_nz69_stretched"):
        r, oc, ob = _advection_ranges(tag)
        case = rc.CASES[tag]
        act = rc.active_columns(case)
        assert {x[3] for x in r} == set(range(1, 8)), f"{tag}: modes {sorted({x[3] for x in r})}"
        for mode in (2, 6, 7):        # the ranges that follow the mixed layer differ between columns and move in time
            assert len({(x[5], x[6]) for x in r if x[3] == mode}) >= 4, (tag, mode)
            per_col = {}
            for x in r:
                if x[3] == mode:
                    per_col.setdefault((x[1], x[2]), set()).add((x[5], x[6]))
            assert sum(len(v) > 1 for v in per_col.values()) >= 3, f"{tag}: mode {mode} keeps its range on every column"
        nm, mo, ad = ob["nmodeadv"][act, 1], ob["modeadv"][act, 1, :], ob["advection"][act, 1, :]
        if tag == "adv_modes_nz40":
            assert (nm == 1).all() and (ad[:, 0] > 0).any() and (ad[:, 0] < 0).any()
            continue
        assert {int(c) % 7 for c in act} == set(range(7)), f"{tag}: a slot pattern lies on land columns only"
        assert (nm == 6).any() and ((nm == 6) & (mo > 0).all(axis=1)).any()                  # all six slots live
        assert any(n >= 2 and len(set(m[:n][m[:n] > 0])) < (m[:n] > 0).sum() for n, m in zip(nm, mo))   # a mode twice
        holes = [m[:n] for n, m in zip(nm, mo) if n >= 3]
        assert any((m[1:-1] == 0).any() and m[-1] > 0 for m in holes)                        # mode 0 between live ones
        assert any((m[1:-1] < 0).any() and m[-1] > 0 for m in holes)                         # a negative one likewise
        assert ((nm == 0) & (mo[:, 0] > 0) & (ad[:, 0] != 0)).any()                          # nothing live, values behind
        assert any(0 < n < 6 and m[n] > 0 and a[n] != 0 for n, m, a in zip(nm, mo, ad))      # live ones, values behind
    # index 1 (temperature) holds live-looking values in the twin and zeros in the other: the reference never reads it
    a, b = (rc.oracle_start(rc.CASES[t], exp_mode=1)[1] for t in ("adv_modes_nz60", "adv_modes_nz60_index1"))
    for k in ("nmodeadv", "modeadv", "advection"):
        assert not a[k][:, 0].any() and b[k][:, 0].all() and np.array_equal(a[k][:, 1], b[k][:, 1]), k
    for build in BUILDS:
        assert not np.array_equal(golden.input_sha("adv_modes_nz60", build), golden.input_sha("adv_modes_nz60_index1", build))
        assert np.array_equal(golden.digests("adv_modes_nz60", build), golden.digests("adv_modes_nz60_index1", build)), \
            f"{build}: the reference's step depends on index 1 of the advection arrays"
    # the advection term and sinc_fcorr in one right-hand side
    sw = rc.CASES["adv_modes_nz69_stretched"].switches
    assert sw["L_SFCORR_WITHZ"] and sw["L_RELAX_SAL"] and (ob["sinc_fcorr"][act] != 0).any()

    r, oc, ob = _advection_ranges("adv_edges_nz40")
    nz = 40

    def some(mode, cond):
        return any(x[3] == mode and cond(*x[4:8]) for x in r)

    assert some(2, lambda km, n1, n2, met: km == 2 and (n1, n2) == (1, 1))                  # mode 2 over one level
    assert some(7, lambda km, n1, n2, met: km == 2 and n1 == 1)                             # mode 7 from level 1
    above = lambda km: -oc.zm[km] < 100.0 and -oc.zm[km + 1] > 100.0      # noqa: E731  (the last centre above 100 m)
    below = lambda km: -oc.zm[km] > 100.0 and -oc.zm[km - 1] < 100.0      # noqa: E731  (the first one below)
    assert some(7, lambda km, n1, n2, met: above(km) and met and n2 == n1)                  # `depth >= dmax` at once
    assert some(7, lambda km, n1, n2, met: below(km) and met and n2 == n1)
    assert some(7, lambda km, n1, n2, met: met and n2 - n1 >= 5)                            # ... after several levels
    assert some(6, lambda km, n1, n2, met: met and n2 == 1)                                 # dmax on the first level
    assert some(6, lambda km, n1, n2, met: met and n2 >= 25)                                # ... and deep
    assert some(6, lambda km, n1, n2, met: km == nz and met) and some(7, lambda km, n1, n2, met: km == nz)
    assert some(2, lambda km, n1, n2, met: km == nz)                                        # full-depth mixed layer
    assert not some(6, lambda km, n1, n2, met: not met)       # (mode 6 cannot run to nzi: see tests/ref_step_cases.py)

    for tag, want in (("adv_edges_120m", lambda nz, n1: n1 == nz - 1),       # mode 4 over the one level nz - 1
                      ("adv_edges_105m", lambda nz, n1: n1 == nz),           # n1 > nzend: none
                      ("adv_edges_102m", lambda nz, n1: n1 == nz + 1)):      # the 100 m level is the last grid point
        r, oc, ob = _advection_ranges(tag)
        four = [x for x in r if x[3] == 4]
        assert four and all(want(rc.CASES[tag].nz, x[5]) for x in four), (tag, four[:2])
        assert {x[3] for x in r} == set(range(1, 8)), tag
    r, oc, ob = _advection_ranges("adv_edges_128m")     # the two comparisons at equality
    assert oc.zm[13] == -100.0 and all(x[5] == 14 for x in r if x[3] == 4) and any(x[3] == 4 for x in r)
    assert any(x[3] == 7 and x[7] and x[8] == 100.0 for x in r)
    r, oc, ob = _advection_ranges("adv_edges_90m")
    assert oc.zm[13] >= -100.0 and not any(x[3] == 4 for x in r)
    assert {x[3] for x in r} == {1, 2, 3, 5, 6, 7}
    assert any(x[3] == 7 and x[7] is False and x[6] == 12 for x in r)        # mode 7 runs to nzi without meeting 100 m
    assert all(x[7] for x in r if x[3] == 6)


def _precedence_and_trap_v_cases_reach_what_they_are_for():
    """The switch pairs: both members' inputs are non-zero, and the diagnostics show which of them ocnint applied
    (fcorr is what L_RELAX_SST computes, tinc_fcorr / ocnTcorr what L_FCORR_WITHZ and L_RELAX_OCNT add, sinc_fcorr /
    scorr what L_SFCORR_WITHZ adds; L_FCORR leaves no diagnostic: that it is ignored is the bit-exact match with the
    reference).  trap_v: the trap fires on |V| >= 10 at levels where |U| < 10."""
    def through(tag):
        case = rc.CASES[tag]
        oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
        seen = np.zeros(case.ncol, dtype=np.int32)
        status = np.zeros(case.ncol, dtype=np.int32)
        for _ in rc.run_oracle(case, oc, ob):
            seen |= ob["paths"]
            status |= ob["status"]
        return ob, seen, status

    def zero(ob, *names):
        return all(not rc.field_of(ob, n, ob.nz).any() for n in names)

    ob, _, _ = through("prec_relax_sst_fcorr_withz")         # relaxation ignored, the correction with depth applied
    assert (ob["relax_sst"] > 1e-10).any() and ob["fcorr_withz"].any()
    assert zero(ob, "fcorr") and rc.field_of(ob, "tinc_fcorr", ob.nz).any()
    ob, _, _ = through("prec_relax_sst_fcorr")               # each excludes the other: neither applied
    assert (ob["relax_sst"] > 1e-10).any() and ob["fcorr_twod"].any() and zero(ob, "fcorr", "tinc_fcorr", "ocnTcorr")
    ob, _, _ = through("prec_fcorr_fcorr_withz")             # likewise: neither applied
    assert ob["fcorr_twod"].any() and ob["fcorr_withz"].any() and zero(ob, "fcorr", "tinc_fcorr", "ocnTcorr")
    ob, _, _ = through("prec_sfcorr_sfcorr_withz")           # the salinity correction with depth ignored
    assert ob["sfcorr_withz"].any() and zero(ob, "sinc_fcorr", "scorr")
    ob, _, _ = through("prec_relax_sst_fcorr_withz_relax_ocnt")
    assert zero(ob, "fcorr") and ob["fcorr_withz"].any() and (ob["relax_ocnT"] > 0).all()
    both = rc.field_of(ob, "tinc_fcorr", ob.nz)
    only = rc.field_of(through("prec_relax_sst_fcorr_withz")[0], "tinc_fcorr", ob.nz)
    assert both.any() and not np.array_equal(both, only)      # the relaxation to the climatology adds to the correction
    for tag in ("trap_v_nz40", "trap_v_clim_nz40"):
        case = rc.CASES[tag]
        start = rc.oracle_start(case, exp_mode=1)[1]
        hit = np.arange(0, case.ncol, 4)
        assert (np.abs(start["V"][hit, 1:5]) >= 10).all() and np.abs(start["U"]).max() < 1.0
        ob, seen, status = through(tag)
        assert ((seen[hit] & orc.PATH_TRAP_V_ALONE) != 0).all() and ((status[hit] & orc.ST_RETRIED) != 0).all()
        assert not (seen & orc.PATHS["TRAP_TJUMP"]).any()
        if case.switches.get("clim_present"):
            assert ((status[hit] & orc.ST_FAILED) != 0).any()
