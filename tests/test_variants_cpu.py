"""What can be settled about tests/variant_cases.py without a GPU, on the oracle alone: the matrix names every
instantiation the launcher's tables name and takes each through the forms it has to meet; the column mix reaches what
it is for under every switch set, at the shapes the matrix uses; and every switch of every set changes the result - a
switch that ocnint's precedence silences, or that the mix never feeds, would sit in the matrix and test nothing."""
import numpy as np
import pytest

import variant_cases as vc

ORACLE_KEYS = sorted({c.oracle_key for c in vc.MATRIX})


# ---------------------------------------------------------------------------------------------------------------
# the matrix is complete
# ---------------------------------------------------------------------------------------------------------------
def test_the_matrix_names_the_instantiations_the_launcher_names():
    """A nineteenth k_column_ps<...> in mckpp_kernels_ps.hip fails here until the matrix has it."""
    compiled = vc.compiled_instantiations()
    assert len(compiled) == 18, sorted(compiled)
    assert {c.instantiation for c in vc.MATRIX} == compiled


def test_every_variant_and_solver_meets_every_form():
    for xv, names in vc.SETS_OF_XV.items():
        for sm in (0, 1):
            met = {c.form for c in vc.MATRIX if c.instantiation[:2] == (xv, sm)}
            assert met == set(vc.FORMS), (xv, sm, sorted(set(vc.FORMS) - met))
        for name in names:       # ... and every switch set, under one solver or the other
            met = {c.form for c in vc.MATRIX if c.set_name == name}
            assert met == set(vc.FORMS), (name, sorted(set(vc.FORMS) - met))


def test_every_instantiation_meets_one_call_plain_and_with_views():
    for inst in vc.compiled_instantiations():
        met = {c.form for c in vc.MATRIX if c.instantiation == inst}
        want = {"F2", "F5"} | ({"F1"} if inst[2] else set())
        assert want <= met, (inst, sorted(want - met))


def test_the_cases_are_what_they_say():
    ids = [c.id for c in vc.MATRIX]
    assert len(set(ids)) == len(ids)
    for c in vc.MATRIX:
        assert set(c.env) <= set(vc.ENV), c.id          # whatever a case sets, the GPU module clears
        assert vc.instantiation(c.switches, c.solver, c.nz, {})[0] == {"default": 0, "relaxed": 1, "corrected": 1,
                                                                          "relaxed_dd": 2, "corrected_dd": 2}[c.set_name]
        assert (c.grid, c.dto) == (("stretched", 1200.0) if c.nz == 69 else ("uniform", 3600.0)), c.id
        assert c.ncol == {"F13": 300}.get(c.form, 1024 if c.nz == 100 else 2048), c.id
    assert all(vc.FORMS[f].nsteps == 3 for f in vc.FORMS if f != "F13")
    assert (vc.FORMS["F13"].nsteps, vc.FORMS["F13"].runs) == (10, 2)


@pytest.mark.parametrize("name", list(vc.SETS))
def test_the_sets_are_live_under_the_precedence_of_ocnint(name):
    """src/mckpp_physics_ocnint_mod.F90:97, :134, :190"""
    sw = vc.SETS[name]
    if sw.get("L_RELAX_SST"):
        assert not sw.get("L_FCORR_WITHZ") and not sw.get("L_FCORR")
    if sw.get("L_FCORR_WITHZ"):
        assert not sw.get("L_FCORR")
    if sw.get("L_SFCORR_WITHZ"):
        assert not sw.get("L_SFCORR")
    if sw.get("L_NO_ISOTHERM"):
        assert sw.get("clim_present") and (sw["iso_bot"], sw["iso_thresh"]) == (20, 0.002)


@pytest.mark.parametrize("nz", [60, 69, 100])
@pytest.mark.parametrize("xv", [0, 1, 2])
def test_the_most_slots_are_the_most_that_fit(xv, nz):
    """F11's geometry from ps_lds_bytes restated: it fits in 160 KiB, one slot more does not (or is more than
    ps_geometry takes), and the waves cover the items or are all sixteen."""
    w = vc.most_slots(nz, xv)
    assert vc.lds_bytes(nz + 3, w, xv) <= vc.LDS_LIMIT
    assert w == vc.MOST_SLOTS or vc.lds_bytes(nz + 3, w + 1, xv) > vc.LDS_LIMIT
    slots, waves, per_cu = (int(x) for x in vc.most_slots_geometry(nz, xv).split("x"))
    assert slots == w and per_cu == 1 and 1 <= waves <= vc.MOST_WAVES
    assert waves == vc.MOST_WAVES or 64 * waves >= w * (nz + 3)
    if nz == 60:
        assert w < vc.MOST_SLOTS if xv == 2 else w == vc.MOST_SLOTS    # the double-diffusion rows cost slots at 60 levels


# ---------------------------------------------------------------------------------------------------------------
# the mix reaches what it is for
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ORACLE_KEYS, ids=["-".join(str(x) for x in k) for k in ORACLE_KEYS])
def test_the_mix_reaches_what_it_is_for(key):
    """Conditions, not measurements (variant_cases.reach): in every step at least 5 % of the active columns are
    trapped (status & 12 == 12 after 66 passes or more: the stragglers) and at least 5 % clamped by the sea floor -
    the figures of test_regimes_through_the_launch_forms - and at least 2 % show each thing the set's switches exist
    for.  As measured (profiles/coverage/kernel_variants.md): trapped 8.3 %, clamped 8.3 % and more, the others 8 % and
    more."""
    set_name, solver, nz, grid, dto, ncol, nsteps = key
    run = vc.oracle_run(*key)
    assert len(run.steps) == nsteps and len(run.active) >= 0.95 * ncol
    short = {k: (bound, got) for k, (bound, got) in vc.reach(run, set_name, nz).items() if got < bound}
    assert not short, f"{key}: (bound, reached) {short}"
    if nz >= 69:
        assert any(np.any(ob["kmix"][run.active] > 64) for ob in run.steps)     # some column mixes past the first wave


@pytest.mark.parametrize("name", ["corrected", "corrected_dd"])
@pytest.mark.parametrize("ncol", [vc.NCOL, vc.QUEUE_NCOL])
def test_every_advection_mode_is_on_some_column(name, ncol):
    oc, ob, land = vc.start(name, 0, 60, "uniform", 3600.0, ncol)
    active = np.setdiff1d(np.arange(ncol), land)
    assert (ob["nmodeadv"][active, 1] == 2).all()
    for slot in (0, 1):
        modes, count = np.unique(ob["modeadv"][active, 1, slot], return_counts=True)
        assert modes.tolist() == [1, 2, 3, 4, 5, 6, 7] and count.min() >= vc.REACHED_AT_LEAST * len(active)
    assert (ob["advection"][active, 1, 0:2] != 0).all()


# ---------------------------------------------------------------------------------------------------------------
# every switch counts
# ---------------------------------------------------------------------------------------------------------------
SWITCHES = [(name, sw) for name in vc.SETS for sw in vc.switches_of(name)]


@pytest.mark.parametrize("name,switch", SWITCHES, ids=[f"{n}-{s}" for n, s in SWITCHES])
def test_every_switch_counts(name, switch):
    """The oracle again with that one switch off: some field of rc.STEP_FIELDS differs in some bit on at least 1 % of
    the active columns after the last step.  Under LDD the salinity itself: a kernel that gave S the factorisation
    of T would be seen."""
    key = (name, 0, *vc.UNIFORM, vc.NCOL, vc.NSTEPS)
    full, less = vc.oracle_run(*key), vc.oracle_run(*key, without=switch)
    d = vc.columns_differing(full.steps[-1], less.steps[-1], full.active)
    field, most = max(d.items(), key=lambda kv: kv[1])
    assert most >= vc.SWITCH_AT_LEAST, f"{name} without {switch}: at most {most:.4f} of the columns differ ({field})"
    if switch == "LDD":
        assert d["S"] >= vc.SWITCH_AT_LEAST, f"{name} without LDD: S differs on {d['S']:.4f} of the columns"
