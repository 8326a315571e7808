"""GPU parity AT the comparisons of the step (tests/ref_step_cases.py, "the edge cases";
profiles/coverage/oracle_boundaries.md): every edge case holds columns on which a `<`, `<=`, `>` or `>=` of the physics
is evaluated with both sides equal, next to columns one ulp to either side.  The column kernel states each of these
comparisons separately from the oracle, several of them more than once, so a `<=` for a `<` in one place passes every
other test.

Bar everywhere: bit-exact on every field of rc.STEP_FIELDS, the status words and the pass counts - against the
recorded reference and the oracle for the cases, against the oracle stepped one step at a time for the launch forms
that change which code states a comparison or who executes it.  That the cases still sit on their equalities is
asserted on the CPU (tests/test_boundaries_cpu.py)."""
import numpy as np
import pytest

import common as cm
import ref_step_cases as rc
from harness import assert_equal_to_oracle, differing, mk  # noqa: F401
from harness import step_golden as golden  # noqa: F401

pytestmark = pytest.mark.gpu

VMIX_FIELDS = ["hmix", "kmix", "uref", "vref", "rho", "cp", "buoy", "difm", "difs", "dift", "ghat", "Rig", "dbloc",
               "Shsq", "wXNT1"]


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("tag", rc.EDGE_CASES)
def test_edge_case_matches_reference_and_oracle(mk, golden, tag, solver):
    """Solver mode 0: the recorded reference and the oracle; solver mode 1 (two-ended elimination): the oracle's
    restatement of that mode."""
    case = rc.CASES[tag]
    act = rc.active_columns(case)
    got = rc.run_hip(mk, tag, golden, solver_mode=solver)
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=1, solver_mode=solver)
    for (nt, hip), _ in zip(got, rc.run_oracle(case, oc, ob)):
        if solver == 0:
            bad = rc.mismatches(case, golden.digests(tag, "pexp"), golden.values(tag), nt, hip.__getitem__)
            assert not bad, f"{tag} step {nt}: HIP differs from the reference's own step: {bad}"
        assert np.array_equal(hip["status"][act], ob["status"][act]), f"{tag} solver {solver} step {nt}: status words"
        assert np.array_equal(hip["npasses"][act], ob["npasses"][act]), f"{tag} solver {solver} step {nt}: pass counts"
        bad = [n for n in rc.STEP_FIELDS if not np.array_equal(
            rc.canonical(hip[n])[act].view(np.int64), rc.canonical(rc.field_of(ob, n, case.nz))[act].view(np.int64))]
        assert not bad, f"{tag} solver {solver} step {nt}: HIP differs from the oracle in {bad}"


# (environment, several steps in one call, the tags it runs on: None = all)
LITERAL_DEPTHS = [t for t in rc.EDGE_CASES if rc.CASES[t].nz in (60, 69)]
FORMS = [
    ({}, True, None),
    ({"MCKPP_MULTISTEP": "0"}, True, None),
    ({"MCKPP_PS_FIXED_L": "0"}, False, LITERAL_DEPTHS),
    ({"MCKPP_PS_FIXED_L": "1"}, True, LITERAL_DEPTHS),
    ({"MCKPP_L2PRE": "0"}, False, None),
    ({"MCKPP_L2PRE": "1"}, False, None),
    ({"MCKPP_PS": "1x1x1"}, False, None),
]
FORM_CASES = [(tag, env, one_call) for env, one_call, tags in FORMS for tag in (tags or rc.EDGE_CASES)]


@pytest.mark.parametrize("tag,env,one_call", FORM_CASES,
                         ids=[f"{t}-{'-'.join(f'{k[6:]}={v}' for k, v in e.items()) or 'default'}-"
                              f"{'one_call' if o else 'call_per_step'}" for t, e, o in FORM_CASES])
def test_edges_through_the_launch_forms(mk, golden, monkeypatch, tag, env, one_call):
    """The edge columns under the forcing of step 1 held for all steps: every step in one launch, with and without the
    multi-step kernel, the kernels with and without the level count as a literal (60 and 69 levels), the
    reference-level sums both ways, a single slot - each against the oracle stepped one step at a time."""
    from oracle import orc

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = rc.CASES[tag]
    act = rc.active_columns(case)
    kc, k3, ctx, oc, ob = rc.start_hip(mk, tag, golden)
    sf = rc.forcing(case, 1)
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    ctx.set_forcing(k3.sflux)
    what = f"{tag} {env} one_call={one_call}"
    if one_call:
        ctx.step(1, case.nsteps)
    for nt in range(1, case.nsteps + 1):
        orc.physics_driver(oc, ob, nt)
        if not one_call:
            ctx.step(nt, 1)
            assert_equal_to_oracle(ctx, k3, ob, case.nz, act, f"{what} step {nt}")
    assert_equal_to_oracle(ctx, k3, ob, case.nz, act, what)
    if "MCKPP_PS" in env:
        assert ctx.kernel_residency()[2] == 64 * int(env["MCKPP_PS"].split("x")[1])
    ctx.close()


@pytest.mark.parametrize("tag", rc.EDGE_CASES)
def test_verticalmixing_alone_on_the_edges(mk, golden, tag):
    """mckpp_hip_vmix_only after the case's steps (bldepth, wscale, rimix and ddmix without the solver around them):
    hmixn / kmixn and the diagnostics of vmix as the oracle's mckpp_physics_verticalmixing gives them, the state left
    alone."""
    from oracle import orc

    case = rc.CASES[tag]
    act = rc.active_columns(case)
    kc, k3, ctx, oc, ob = rc.start_hip(mk, tag, golden)
    for nt in range(1, case.nsteps + 1):
        sf = rc.forcing(case, nt)
        ob["sflux"] = sf
        cm.set_forcing_3d(k3, sf)
        ctx.set_forcing(k3.sflux)
        ctx.step(nt, 1)
        orc.physics_driver(oc, ob, nt)
    assert_equal_to_oracle(ctx, k3, ob, case.nz, act, f"{tag} before vmix_only")
    before = {n: np.array(getattr(k3, n), copy=True) for n in ("U", "X", "Us", "Xs", "hmixd", "Tref", "Ssurf")}
    ctx.vmix_only(case.nsteps + 1)
    orc.vmix_only(oc, ob, case.nsteps + 1)
    ctx.download(k3)
    ctx.close()
    bad = differing(k3, ob, case.nz, act, VMIX_FIELDS)
    assert not bad, f"vmix only on {tag}: {bad}"
    for n, v in before.items():
        assert np.array_equal(getattr(k3, n), v, equal_nan=True), n
