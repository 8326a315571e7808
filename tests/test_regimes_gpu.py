"""GPU parity in the physics regimes the synthetic generators never reach by themselves (tests/ref_step_cases.py,
"the regimes"): the sea floor clamping the boundary layer (bldepth_mod.F90:161,175), columns mixing down
to the last level of the grid, the instability trap fired by a temperature jump and by the rms change of a step
(ocnstep_mod.F90:200-227), columns retried and then accepted, L_SSref = .FALSE., and ddmix's diffusive convection.

Bar everywhere: bit-exact on every field of rc.STEP_FIELDS, the status words and the pass counts - against the
recorded reference and the oracle for the cases, against the oracle stepped one step at a time for the launch forms.
That the cases take the branches they are named after is asserted on the CPU (tests/test_ref_step_cpu.py,
test_the_cases_reach_what_they_are_for).  All inputs are seeds and closed forms; all of it is finite
arithmetic the reference and the oracle ran on the CPU.

Not covered here: invalid `old`/`new` indices (ST_DODGY_OLDNEW).  Before an out-of-range index is fed to a device it
has to be shown by reading that every consumer of it sanitises it first."""
import numpy as np
import pytest

import common as cm
import ref_step_cases as rc
from harness import assert_equal_to_oracle, differing, mk  # noqa: F401

pytestmark = pytest.mark.gpu

VIEWS_FORCED = {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}


def _start(mk, ncol, nz, grid="uniform", dto=3600.0, solver=0, switches=None, hook=rc.regime_mix, land=None, shards=0):
    """Oracle (const, batch) and HIP (const, fields, context) from the same start: the generators' columns with `hook`
    on top, `land` columns masked out, initialised on both sides and compared, the bench forcing set.  shards > 0:
    an MckppHipMulti of that many shards in place of the single context."""
    from oracle import orc

    switches = switches or {}
    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid, dto=dto, solver_mode=solver, **switches)
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, dto=dto)
    for k, v in switches.items():
        setattr(kc, k, v)
    rc.apply_both(ob, k3, nz + 1, hook(ncol, nz + 1, ob))
    if land is not None:
        k3.run_physics[land] = 0
        k3.l_ocean[land] = 0
    ctx = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    ctx.set_solver_mode(solver)
    ctx.upload(k3)
    ctx.init_ocean(0)
    ctx.download(k3)
    orc.init_ocean(oc, ob, 0)
    active = np.nonzero(k3.run_physics)[0]
    bad = differing(k3, ob, nz, active)
    assert not bad, f"init: {bad}"
    sf = cm.synth.forcing(ncol, "bench")
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    ctx.set_forcing(k3.sflux)
    return oc, ob, kc, k3, ctx, active


# ---------------------------------------------------------------------------------------------------------------
# the recorded cases: against the reference's own step and, with status words and pass counts, the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("tag", rc.REGIME_CASES)
def test_regime_case_matches_reference_and_oracle(mk, tag, solver):
    """Solver mode 0: the recorded reference and the oracle; solver mode 1 (two-ended elimination): the oracle's
    restatement of that mode."""
    golden = rc.Golden()
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


# ---------------------------------------------------------------------------------------------------------------
# the launch forms that reorder WHO does the work, on the regimes side by side
# ---------------------------------------------------------------------------------------------------------------
FORMS = [  # (nz, grid, dto, environment, several steps in one call)
    (60, "uniform", 3600.0, {}, True),
    (60, "uniform", 3600.0, {"MCKPP_MULTISTEP": "0"}, True),
    (60, "uniform", 3600.0, VIEWS_FORCED, False),
    (60, "uniform", 3600.0, VIEWS_FORCED, True),
    (100, "uniform", 3600.0, VIEWS_FORCED, True),
    (60, "uniform", 3600.0, {"MCKPP_PS_FIXED_L": "0"}, False),
    (60, "uniform", 3600.0, {"MCKPP_PS_FIXED_L": "1"}, False),
    (69, "stretched", 1200.0, {"MCKPP_PS_FIXED_L": "0"}, True),
    (69, "stretched", 1200.0, {"MCKPP_PS_FIXED_L": "1"}, True),
    (100, "uniform", 3600.0, {"MCKPP_PS_FIXED_L": "0"}, True),
    (100, "uniform", 3600.0, {"MCKPP_PS_FIXED_L": "1"}, False),
    (60, "uniform", 3600.0, {"MCKPP_L2PRE": "0"}, False),
    (60, "uniform", 3600.0, {"MCKPP_L2PRE": "1"}, False),
    (69, "stretched", 1200.0, {"MCKPP_L2PRE": "0"}, False),
    (69, "stretched", 1200.0, {"MCKPP_L2PRE": "1"}, False),
    (60, "uniform", 3600.0, {"MCKPP_PS": "1x1x1"}, False),
    (60, "uniform", 3600.0, {"MCKPP_PS": "5x8x2"}, True),
]


@pytest.mark.parametrize("nz,grid,dto,env,one_call", FORMS,
                         ids=[f"nz{f[0]}-{'-'.join(f'{k[6:]}={v}' for k, v in f[3].items()) or 'default'}-"
                              f"{'one_call' if f[4] else 'call_per_step'}" for f in FORMS])
def test_regimes_through_the_launch_forms(mk, monkeypatch, nz, grid, dto, env, one_call):
    """2048 columns of rc.regime_mix (clamped by the sea floor, mixing to the last level, trapped on a temperature
    jump - 66 passes a step, the stragglers the views exist for - and plain ones, side by side in every workgroup),
    three steps: several steps in one launch, a launch per step, the forced views, the kernels with and without the
    level count as a literal, the reference-level sums both ways, forced geometries down to a single slot - each
    against the oracle stepped one step at a time, every column."""
    from oracle import orc

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ncol, nsteps = 2048, 3
    oc, ob, kc, k3, ctx, active = _start(mk, ncol, nz, grid=grid, dto=dto, land=np.arange(5, ncol, 23))
    what = f"nz={nz} {env} one_call={one_call}"
    if one_call:
        ctx.step(1, nsteps)
    for nt in range(1, nsteps + 1):
        orc.physics_driver(oc, ob, nt)
        if not one_call:
            ctx.step(nt, 1)
            assert_equal_to_oracle(ctx, k3, ob, nz, active, f"{what} step {nt}")
    assert_equal_to_oracle(ctx, k3, ob, nz, active, what)
    if "MCKPP_PS" in env:
        assert ctx.kernel_residency()[2] == 64 * int(env["MCKPP_PS"].split("x")[1])
    ctx.close()
    trapped = active[active % 8 == 3]
    assert (ob["status"][trapped] & 12 == 12).all() and (ob["npasses"][trapped] >= 66).all()
    assert (ob["hmix"][active] == -ob["ocdepth"][active]).sum() >= 0.05 * len(active)
    assert (ob["kmix"][active] >= nz).sum() >= 0.03 * len(active)


# ---------------------------------------------------------------------------------------------------------------
# vertical mixing by itself (bldepth lives there) over bathymetry
# ---------------------------------------------------------------------------------------------------------------
VMIX_FIELDS = ["hmix", "kmix", "uref", "vref", "rho", "cp", "buoy", "difm", "difs", "dift", "ghat", "Rig", "dbloc",
               "Shsq", "wXNT1"]


@pytest.mark.parametrize("nz,grid", [(40, "uniform"), (60, "uniform"), (69, "stretched"), (100, "uniform")])
def test_verticalmixing_alone_over_bathymetry(mk, nz, grid):
    """mckpp_hip_vmix_only after two steps of the regime mix: hmixn / kmixn and the diagnostics of vmix as the
    oracle's mckpp_physics_verticalmixing gives them, the state left alone."""
    from oracle import orc

    ncol = 640
    oc, ob, kc, k3, ctx, active = _start(mk, ncol, nz, grid=grid, land=np.arange(3, ncol, 17))
    for nt in (1, 2):
        ctx.step(nt, 1)
        orc.physics_driver(oc, ob, nt)
    assert_equal_to_oracle(ctx, k3, ob, nz, active, f"nz={nz} before vmix_only")
    before = {n: np.array(getattr(k3, n), copy=True) for n in ("U", "X", "Us", "Xs", "hmixd", "Tref", "Ssurf", "old", "new_")}
    ctx.vmix_only(3)
    orc.vmix_only(oc, ob, 3)
    ctx.download(k3)
    ctx.close()
    bad = differing(k3, ob, nz, active, VMIX_FIELDS)
    assert not bad, f"vmix only nz={nz}: {bad}"
    for n, v in before.items():
        assert np.array_equal(getattr(k3, n), v), n
    assert (ob["hmix"][active] == -ob["ocdepth"][active]).sum() >= 0.05 * len(active)


@pytest.mark.parametrize("nz,grid", [(40, "uniform"), (60, "uniform"), (69, "stretched")])
def test_kppmix_tridiag_pass_over_bathymetry(mk, nz, grid):
    """mckpp_hip_vmix_pass (one vmix + ocnint pass from the raw profiles) on the regime mix, against orc.vmix_batch."""
    from oracle import orc

    ncol = 1000
    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid)
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid)
    rc.apply_both(ob, k3, nz + 1, rc.regime_mix(ncol, nz + 1, ob))
    sf = cm.synth.forcing(ncol, "bench")
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.vmix_pass(1)
    ctx.download(k3)
    ctx.close()
    orc.vmix_batch(oc, ob, 1)
    bad = differing(k3, ob, nz, None, ["U", "V", "T", "S"] + VMIX_FIELDS)
    assert not bad, f"vmix pass nz={nz}: {bad}"
    assert (ob["hmix"] == -ob["ocdepth"]).sum() >= 0.05 * ncol


# ---------------------------------------------------------------------------------------------------------------
# a model day of the forced run over a coast: scattered land, bathymetry shoaling towards it
# ---------------------------------------------------------------------------------------------------------------
def _coast(ncol, seed=20261017):
    """(land columns, hook): a seeded scatter of land points over a tenth of the columns; the sea floor rises from
    150 m, five columns from the nearest land point and beyond, to 1 m next to it"""
    land = np.sort(np.random.default_rng(seed).choice(ncol, ncol // 10, replace=False))
    dist = np.abs(np.arange(ncol)[:, None] - land[None, :]).min(axis=1)
    depth = np.interp(dist, [1, 2, 3, 4, 5], [1.0, 4.0, 12.0, 40.0, 150.0])

    def hook(n, nzp1, ob):
        return {"ocdepth": -depth, "jerlov": (1 + (np.arange(n) % 5)).astype(np.int32)}
    return land, hook


@pytest.mark.parametrize("shards", [0, 3])
def test_forced_day_over_a_coast(mk, shards):
    """mckpp_hip_run_forced over a model day (72 steps of 1200 s, diurnal flux records resident on the device) on the
    69-level stretched grid with a scattered land mask and a sea floor that shoals towards the land points - the
    picture of BASELINE configs[4] - against the oracle driven the same way; through one context (shards = 0) and
    through MckppHipMulti with three shards."""
    from oracle import orc

    ncol, nz, dto, nsteps, ndtocn = 600, 69, 1200.0, 72, 3
    land, hook = _coast(ncol)
    oc, ob, kc, k3, ctx, active = _start(mk, ncol, nz, grid="stretched", dto=dto, hook=hook, land=land, shards=shards)
    series = cm.synth.flux_series(ncol, 1, nsteps, dto)[::ndtocn]
    ctx.set_flux_series(0, series)
    half = 31                                          # the second call starts in the middle of a forcing interval
    ctx.run_forced(1, half, ndtocn)
    ctx.run_forced(half + 1, nsteps - half, ndtocn)
    if shards:
        ctx.synchronize()
    clamped = np.zeros(ncol, dtype=bool)
    for nt in range(1, nsteps + 1):
        if (nt - 1) % ndtocn == 0:
            orc.fluxes(oc, ob, nt, **dict(zip(cm.synth.FLUX_NAMES, series[(nt - 1) // ndtocn])))
        orc.physics_driver(oc, ob, nt)
        clamped |= ob["hmix"] == -ob["ocdepth"]
    assert_equal_to_oracle(ctx, k3, ob, nz, active, f"forced day, shards={shards}")
    assert np.array_equal(k3.sflux[active, 0:6, 4, 0], ob["sflux"][active])
    ctx.close()
    assert clamped[active].sum() >= 0.1 * len(active), "the sea floor clamps too few columns of the coast"


# ---------------------------------------------------------------------------------------------------------------
# L_SSref = .FALSE.: Ssurf = S(1) + Sref (ocnstep_mod.F90:309-313)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,switches", [(40, dict(L_SSref=0)), (60, dict(L_SSref=0)),
                                         (40, dict(L_SSref=0, L_DAMP_CURR=1, dt_uvdamp=360)),
                                         (60, dict(L_SSref=0, L_DAMP_CURR=1, dt_uvdamp=360))])
def test_surface_salinity_follows_the_column(mk, nz, switches):
    """On the default kernel and on an optional-physics one, over the regime mix: Ssurf feeds the fresh-water flux of
    the next step, so three steps."""
    from oracle import orc

    ncol = 512
    oc, ob, kc, k3, ctx, active = _start(mk, ncol, nz, switches=switches)
    for nt in (1, 2, 3):
        ctx.step(nt, 1)
        orc.physics_driver(oc, ob, nt)
        assert_equal_to_oracle(ctx, k3, ob, nz, active, f"{switches} nz={nz} step {nt}")
    ctx.close()
    assert np.array_equal(k3.Ssurf, k3.X[:, 0, 1] + k3.Sref) and not np.array_equal(k3.Ssurf, k3.SSref)


# ---------------------------------------------------------------------------------------------------------------
# a property that needs no oracle
# ---------------------------------------------------------------------------------------------------------------
def test_boundary_layer_never_below_the_sea_floor_1e5x60(mk):
    """bldepth takes hbl from min(hri, hmonob, hekman, -ocdepth) at the level that hits (bldepth_mod.F90:161-183), and
    a sea floor at D inside the grid makes some level hit: hmix <= D after every step, on every column of 1e5 x 60
    with D from 0.5 m to the grid's own depth; and the clamp binds on a good part of them."""
    ncol, nz = 100_000, 60
    kc, k3 = cm.make_hip_case(ncol, nz)
    D = np.resize(np.linspace(0.5, -kc.zm[nz - 1], 997), ncol)         # down to the last level that can hit
    k3.ocdepth[:] = -D
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(ncol, "bench"))
    ctx.set_forcing(k3.sflux)
    for nt in (1, 2, 3):
        ctx.step(nt, 1)
        ctx.download(k3, mk.api.F_RESTART)
        assert np.all(k3.hmix <= D) and np.all(k3.hmix > 0), f"step {nt}: {(k3.hmix > D).sum()} columns mix below their sea floor"
        assert np.all(np.isfinite(k3.X)) and np.all(np.isfinite(k3.U))
        assert (k3.hmix == D).sum() >= 0.05 * ncol      # (the oracle on every 25th of these columns: 6.4 ... 7.7 %)
    ctx.close()
