"""The oracle against the reference's OWN init, flux assembly and time loop (oracle/ref_step_shim.F90 over the
reference's sources and the in-memory flux file of oracle/netcdf_standin.F90, built by oracle/Makefile target `ref`):
mckpp_initialize_ocean_model with the tridiagonal factors it computes, mckpp_initialize_fluxes, mckpp_fluxes through
the reference's reader - the record of a step chosen by its own mckpp_get_update_time -, mckpp_fluxes_ntflux /
_swdk under the reference's own ntime, and mckpp_physics_driver, on the cases of tests/ref_loop_cases.py - bit for
bit, on every recorded field after init and after every step.

Against the recorded outputs (tests/golden/ref_loop.npz) always, and against the live reference where
oracle/_ref/libmckpp_ref_step*.so were built: exp_mode=0 against the libm build, exp_mode=1 against the portable-exp
build.  The oracle is driven as the loop by ref_loop_cases.run_oracle: orc.fluxes at the steps with
(nt-1) % ndtocn == 0 only, with record (nt-1)//ndtocn; the reference picks its own, and that they agree is asserted.

Single edits that test_oracle_loop_matches_the_recorded_reference was checked to catch, with the first line of its
failure, and whether the suite before these tests noticed the edit:
  orc_swdk alone given 7.8 for type III's a2   "every_step_nz40 (libm exp) after init: ... {'swdk_opt': 'digest differs'}"
      before: only through the compiler-convention vectors (test_compiler_conventions_intrinsics_golden)
  calm-point taux 1e-10 -> 1e-11               "every_step_nz40 (libm exp) step 1: ... {'U': ..., 'V': ..., 'T': ..."
      before: test_fluxes_assembly, against the same constant written again in the test
  record index nt // ndtocn                    "every_step_nz40 (libm exp) step 1: ... {'U': ..., 'V': ..., 'T': ..."
      before: no test (the forced-run tests compare the device with an oracle driven by the same index)
  the next record at steps without an update   "diurnal_nz60_nd3 (libm exp) step 2: ... {'U': ..., 'V': ..., 'T': ..."
      before: no test
  deltaz of init's wX taken as hm(k)           "every_step_nz40 (libm exp) after init: ... {'wU1': ..., 'wX1': ..., 'wX2':
      ..., 'wX3': ...}"; before: as a drift of the step record's starting state only (its input digest)
  tri(k,0,1) from dzb(k)                       "every_step_nz40 (libm exp) after init: ... {'tri0': 'digest differs'}"
      before: test_step_invariants (a conservation property), not against the reference"""
import numpy as np
import pytest

import ref_loop_cases as lc
from harness import loop_golden as golden  # noqa: F401
from oracle import orc

BUILDS = lc.BUILDS


def test_every_case_is_recorded(golden):
    assert golden.cases() == sorted(lc.CASES)
    for tag, case in lc.CASES.items():
        for b in BUILDS:
            assert golden.init_sha(tag, b).shape == (len(lc.INIT_FIELDS), 32), (tag, b)
            assert golden.sha(tag, b).shape == (case.nsteps, len(lc.LOOP_FIELDS), 32), (tag, b)
        assert sorted(golden.values(tag, "pexp")) == (sorted(lc.CORE) if case.full else []), tag


def _check_recorded(golden, tag, build, nt, oc, ob):
    case = lc.CASES[tag]
    if nt == 0:
        bad = lc.mismatches(case, lc.INIT_FIELDS, golden.init_sha(tag, build),
                            lc.batch_get(ob, case.nz, (oc.tri0, oc.tri1)))
    else:
        values = golden.values(tag, build) if nt == case.nsteps else None
        bad = lc.mismatches(case, lc.LOOP_FIELDS, golden.sha(tag, build)[nt - 1], lc.batch_get(ob, case.nz), values)
    where = "after init" if nt == 0 else f"step {nt}"
    assert not bad, f"{tag} ({build} exp) {where}: the oracle differs from the recorded reference: {bad}"


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tag", list(lc.CASES))
def test_oracle_loop_matches_the_recorded_reference(golden, tag, build):
    case, em = lc.CASES[tag], BUILDS[build]
    _, raw, _ = lc.oracle_raw(case, em)
    assert np.array_equal(lc.input_digest(case, raw, lc.flux_records(case)), golden.input_sha(tag, build)), \
        f"{tag}: the seeded inputs are not the recorded ones (tests/common.py, synth or the case changed?)"
    for nt, oc, ob in lc.run_oracle(case, em):
        _check_recorded(golden, tag, build, nt, oc, ob)


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("tag", list(lc.CASES))
def test_oracle_loop_matches_the_live_reference(golden, tag, build):
    """... and the libraries built here give the committed record (the generator would write the same digests)."""
    if not orc.have_ref_step():
        pytest.skip("the reference's libraries are not built here (oracle/_ref)")
    case, em = lc.CASES[tag], BUILDS[build]
    (ib, t0, t1), steps = lc.run_reference(case, em)
    rec = lc.record(case, (ib, t0, t1), steps)
    assert np.array_equal(rec["init_sha"], golden.init_sha(tag, build)), f"{tag} ({build}): init is not the recorded one"
    assert np.array_equal(rec["sha"], golden.sha(tag, build)), f"{tag} ({build}): the steps are not the recorded ones"
    for nt, oc, ob in lc.run_oracle(case, em):
        names = lc.INIT_FIELDS if nt == 0 else lc.LOOP_FIELDS
        ref = lc.batch_get(ib, case.nz, (t0, t1)) if nt == 0 else lc.batch_get(steps[nt - 1], case.nz)
        got = lc.batch_get(ob, case.nz, (oc.tri0, oc.tri1))
        for name in names:
            d = lc.first_difference(case, name, lc._over_columns(case, name, got(name)),
                                    lc._over_columns(case, name, ref(name)))
            assert d is None, (f"{tag} ({build} exp) {'after init' if nt == 0 else f'step {nt}'}: {name} differs "
                               f"from the live reference, {d}")


@pytest.mark.parametrize("tag", list(lc.CASES))
def test_host_tri_matches_the_reference_init(golden, tag):
    """tri(:,0:1,1) as the library's host side builds it for KppConstFields (the C ABI takes it from there; no
    device call returns it) against what the reference's init computed."""
    import mckpp_f90_amd as mk

    case = lc.CASES[tag]
    zm, hm, dm = lc.cm.grid_for(case.nz, case.grid)
    kc = mk.KppConstFields(case.nz, dto=case.dto, zm=zm[1:case.nz + 2], hm=hm[1:case.nz + 2], dm=dm)
    sha = golden.init_sha(tag, "pexp")
    for i in (0, 1):
        assert np.array_equal(lc.digest(kc.tri[0:case.nz + 1, i, 0]), sha[lc.INIT_FIELDS.index(f"tri{i}")]), \
            f"{tag}: tri(:,{i},1) of KppConstFields is not the reference's"


def _assembled(case, rec):
    """sflux rows 1, 2, 3, 4, 6 that mckpp_fluxes assembles from a record (row 5 is a constant), [5, ncol]"""
    taux = np.where((rec[0] == 0.0) & (rec[1] == 0.0), 1e-10, rec[0])
    return np.array([taux, rec[1], rec[2], rec[3] + rec[4] + rec[5] - rec[7] * lc.FLSN, rec[6] + rec[7] + rec[4] / lc.EL])


def test_the_cases_reach_what_they_are_for(golden):
    """Each case has what it is named after - from the inputs and the recorded reference results alone (else a
    bit-exact match proves less than it says)."""
    counts = {}
    for tag, case in lc.CASES.items():
        rec, oce, act = lc.flux_records(case), lc.ocean(case).astype(bool), lc.active_columns(case)
        n_calm = sum(int(((rec[r, 0] == 0.0) & (rec[r, 1] == 0.0) & oce).sum()) for r in range(len(rec)))
        counts[tag] = dict(land=int((~oce).sum()), calm=n_calm, jerlov=sorted(set(lc.jerlov(case)[act])),
                           zero_swf_records=int(sum(bool((rec[r, 2][act] == 0.0).all()) for r in range(len(rec)))))
        assert counts[tag]["jerlov"] == [1, 2, 3, 4, 5], tag
        if case.ndtocn > 1 and case.flux_file and not case.l_rest:
            # a step without an update whose record differs from both neighbours in every assembled row on every
            # ocean column: a loop that took a neighbouring record there, or refreshed sflux, could not go unseen
            told_apart = []
            for nt in range(1, case.nsteps + 1):
                r = (nt - 1) // case.ndtocn
                if (nt - 1) % case.ndtocn == 0 or r + 1 >= len(rec):
                    continue
                near = [q for q in (r - 1, r + 1) if 0 <= q < len(rec)]
                if all((_assembled(case, rec[r])[:, act] != _assembled(case, rec[q])[:, act]).all() for q in near):
                    told_apart.append(nt)
            assert told_apart, f"{tag}: no step without an update at which successive records differ everywhere"
            counts[tag]["steps_told_apart"] = told_apart
    print(counts)
    c = counts["every_step_nz40"]
    assert c["land"] == 10 and c["calm"] > 0 and lc.CASES["every_step_nz40"].ndtocn == 1
    assert counts["diurnal_nz60_nd3"]["zero_swf_records"] >= 1 and counts["diurnal_nz60_nd3"]["calm"] > 0
    assert lc.CASES["diurnal_nz60_nd3"].ndtocn == 3 and counts["diurnal_nz60_nd3"]["steps_told_apart"]
    nl = lc.CASES["namelist_nz69_nd2"]
    assert (nl.nz, nl.grid, nl.dto, nl.ndtocn) == (69, "stretched", 1200.0, 2)
    assert abs(counts["namelist_nz69_nd2"]["land"] / nl.ncol - 1 / 3) < 0.05
    assert lc.CASES["deep_nz100_nd4"].nz == 100 and lc.CASES["deep_nz100_nd4"].ndtocn == 4
    assert lc.CASES["startt_nd3"].startt % 1.0 != 0.0 and lc.CASES["startt_nd3"].ndtocn == 3
    for tag in ("sweep_nd1", "sweep_nd3"):
        assert lc.CASES[tag].ncol * lc.CASES[tag].nsteps >= 2000 * 24 and counts[tag]["calm"] > 0 \
            and counts[tag]["land"] > 0 and counts[tag]["zero_swf_records"] >= 1
    assert {lc.CASES["sweep_nd1"].ndtocn, lc.CASES["sweep_nd3"].ndtocn} == {1, 3}
    # the recorded reference: calm points came out as taux = 1e-10, l_rest and the constants as the reference has
    # them, the last step's short wave reached wXNT1, and the boundary layer of init differs across columns
    for tag in ("every_step_nz40", "diurnal_nz60_nd3", "startt_nd3"):
        case, v = lc.CASES[tag], golden.values(tag, "pexp")
        last = lc.flux_records(case)[lc.nrec(case) - 1][:, lc.active_columns(case)]
        calm = (last[0] == 0.0) & (last[1] == 0.0)
        assert calm.any() and (v["sflux1"][calm] == 1e-10).all() and (v["sflux1"][~calm] == last[0][~calm]).all(), tag
        assert np.array_equal(v["sflux3"], last[2]), tag
    v = golden.values("l_rest", "pexp")
    assert (v["sflux1"] == 1e-10).all() and (v["sflux3"] == 300.0).all() and (v["sflux4"] == -300.0).all()
    v = golden.values("no_flux_file", "pexp")
    assert (v["sflux1"] == 0.01).all() and (v["sflux3"] == 200.0).all() and (v["sflux6"] == 6e-5 - 150.0 / lc.EL).all()
    assert (golden.values("every_step_nz40", "pexp")["wXNT1"] != 0).any()
    for tag, case in lc.CASES.items():      # hmix after init, from the oracle run that the record has just confirmed
        _, _, ob = next(iter(lc.run_oracle(case, 1)))
        assert len(set(ob["hmix"][lc.active_columns(case)])) > 1, f"{tag}: one hmix on every column after init"
    case = lc.CASES["ldd_nz60"]
    _, _, ob = next(iter(lc.run_oracle(case, 1)))
    assert (ob["dift"][:, 1:case.nz] != ob["difs"][:, 1:case.nz]).any(), "ldd_nz60: dift never differs from difs"
