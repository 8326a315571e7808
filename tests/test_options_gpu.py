"""the optional physics switches of ocnint / ocnstep / check_profile on the device
(src/mckpp_physics_ocnint_mod.F90:97-215, src/mckpp_physics_solvers.F90:176-335,
src/mckpp_physics_verticalmixing_ddmix_mod.F90, src/mckpp_physics_ocnstep_mod.F90:317-340,
src/mckpp_physics_overrides.F90:42-125).  Every switch combination is compared bit for bit with the
oracle's restatement on identical inputs."""
import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401

pytestmark = pytest.mark.gpu

FIELDS = cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["hmixd0", "hmixd1"] + list(cm.DIAG_FIELDS.keys()) + cm.EXT_SCALARS


def _case(mk, ncol, nz, switches, prep, nsteps=2, grid="uniform"):
    """switches: dict of kpp_const switch -> value (same names on both sides);
    prep(k3, ob, col_T, col_S): fill the optional input fields identically on both sides."""
    from oracle import orc

    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid, **switches)
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid)
    for k, v in switches.items():
        setattr(kc, k, v)
    prep(k3, ob)
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    orc.init_ocean(oc, ob, 0)
    sf = cm.synth.forcing(ncol, "bench")
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    for nt in range(1, nsteps + 1):
        ctx = mk.mckpp_physics_driver(k3, kc, nt)
        orc.physics_driver(oc, ob, nt)
        st, nf, npass = ctx.status()
        assert np.array_equal(st, ob["status"]) and np.array_equal(npass, ob["npasses"])
        res = cm.compare(k3, ob, nz, FIELDS)
        bad = {k: v for k, v in res.items() if v[2] != 0}
        assert not bad, f"{switches} step {nt}: {bad}"
    return k3, ob


def _set2(k3, ob, name, arr):
    """same (ncol, nzp1) profile field on both sides"""
    nzp1 = arr.shape[1]
    getattr(k3, name)[:, :] = arr
    ob.a[name][:, 1:nzp1 + 1] = arr


def test_relax_sst_and_calconly(mk):
    def prep(k3, ob):
        n = k3.npts
        r = np.full(n, 1.0 / (5 * 86400.0)); r[::4] = 0.0        # some columns not relaxed
        k3.relax_sst[:] = r; ob["relax_sst"] = r
        sst = k3.X[:, 0, 0] + 1.5
        k3.SST0[:] = sst; ob["SST0"] = sst
    k3, ob = _case(mk, 96, 40, dict(L_RELAX_SST=1), prep)
    assert np.any(k3.fcorr != 0) and np.all(k3.fcorr[::4] == 0)
    _case(mk, 32, 40, dict(L_RELAX_SST=1, L_RELAX_CALCONLY=1), prep)


def test_fcorr_twod_and_withz(mk):
    def prep2(k3, ob):
        v = np.linspace(-80.0, 80.0, k3.npts)
        k3.fcorr_twod[:] = v; ob["fcorr_twod"] = v
    _case(mk, 64, 40, dict(L_FCORR=1), prep2)

    def prepz(k3, ob):
        nzp1 = k3.X.shape[1]
        z = np.arange(nzp1)[None, :]
        _set2(k3, ob, "fcorr_withz", 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, k3.npts)[:, None])
        _set2(k3, ob, "sfcorr_withz", 1e-7 * np.cos(z / 7.0) * np.ones((k3.npts, 1)))
    k3, ob = _case(mk, 64, 40, dict(L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1), prepz)
    assert np.any(k3.tinc_fcorr != 0) and np.any(k3.scorr != 0)


def test_relax_ocnt_and_sal(mk):
    def prep(k3, ob):
        n = k3.npts
        _set2(k3, ob, "ocnT_clim", np.asarray(k3.X[:, :, 0]) - 0.3)
        _set2(k3, ob, "sal_clim", np.asarray(k3.X[:, :, 1]) + 0.05)
        r = np.full(n, 1.0 / (30 * 86400.0))
        k3.relax_ocnT[:] = r; ob["relax_ocnT"] = r
        k3.relax_sal[:] = 2 * r; ob["relax_sal"] = 2 * r
    k3, ob = _case(mk, 64, 60, dict(L_RELAX_OCNT=1, L_RELAX_SAL=1), prep)
    assert np.any(k3.ocnTcorr != 0) and np.any(k3.sinc_fcorr != 0)


def test_double_diffusion(mk):
    def prep(k3, ob):
        # salt-fingering favourable stratification on half of the columns: warm salty over cold fresh
        nzp1 = k3.X.shape[1]
        z = np.linspace(0, 1, nzp1)[None, :]
        S = np.asarray(k3.X[:, :, 1]).copy()
        S[::2] = 0.4 - 0.8 * z
        k3.X[:, :, 1] = S
        ob.a["S"][:, 1:nzp1 + 1] = S
    _case(mk, 64, 40, dict(LDD=1), prep, nsteps=3)


def test_double_diffusion_with_the_most_slots_a_workgroup_takes(mk, monkeypatch):
    """21 slots x 3 species = 63 lanes of the manager wave in M3 (hbl, blmix scalars: one lane per (slot, species));
    the launcher's own choice for this depth has fewer"""
    monkeypatch.setenv("MCKPP_PS", "21x4x1")

    def prep(k3, ob):
        nzp1 = k3.X.shape[1]
        z = np.linspace(0, 1, nzp1)[None, :]
        S = np.asarray(k3.X[:, :, 1]).copy()
        S[::2] = 0.4 - 0.8 * z
        k3.X[:, :, 1] = S
        ob.a["S"][:, 1:nzp1 + 1] = S
    _case(mk, 150, 20, dict(LDD=1), prep, nsteps=3)


def test_current_damping(mk):
    _case(mk, 64, 40, dict(L_DAMP_CURR=1, dt_uvdamp=360), lambda k3, ob: None)


def test_no_freeze_and_isotherm_and_clim_reset(mk):
    def prep(k3, ob):
        nzp1 = k3.X.shape[1]
        T = np.asarray(k3.X[:, :, 0]).copy()
        T[::3, :] = -2.2                       # below -1.8 everywhere: clamped, freeze_flag counts levels
        T[1::3, :] = 12.0                      # isothermal columns: reset to climatology
        k3.X[:, :, 0] = T
        ob.a["T"][:, 1:nzp1 + 1] = T
        _set2(k3, ob, "ocnT_clim", 8.0 + 10.0 * np.exp(-np.arange(nzp1) / 15.0)[None, :] * np.ones((k3.npts, 1)))
        _set2(k3, ob, "sal_clim", np.asarray(k3.X[:, :, 1]) * 0.5)
        k3.U[2::3, 0:3, 0] = 40.0              # absurd currents: trap -> climatology + U_init
        ob.a["U"][2::3, 1:4] = 40.0
    sw = dict(L_NO_FREEZE=1, L_NO_ISOTHERM=1, clim_present=1, iso_bot=20, iso_thresh=0.002)
    k3, ob = _case(mk, 60, 40, sw, prep, nsteps=1)
    # frozen columns clamped, isothermal columns reset (negative count), trapped columns reset to climatology
    assert np.any(k3.freeze_flag > 0) and np.any(k3.reset_flag < 0) and np.any(np.abs(k3.reset_flag) == 999)
    _case(mk, 60, 40, sw, prep, nsteps=3)


@pytest.mark.parametrize("nz", [40, 69])
def test_climatology_reset_alone_runs_on_the_default_kernel(mk, nz):
    """The shipped namelist names T and S climatology files (ocnT_file, sal_file /= 'none') and switches nothing
    else on: check_profile then resets a failed column's T and S to the climatology instead of leaving them
    (src/mckpp_physics_overrides.F90:57-78).  That needs the two input fields but none of the optional-physics
    kernel code, so such a context runs the default build."""
    def prep(k3, ob):
        nzp1 = k3.X.shape[1]
        _set2(k3, ob, "ocnT_clim", 8.0 + 10.0 * np.exp(-np.arange(nzp1) / 15.0)[None, :] * np.ones((k3.npts, 1)))
        _set2(k3, ob, "sal_clim", np.asarray(k3.X[:, :, 1]) * 0.5)
        k3.U[2::3, 0:3, 0] = 40.0              # absurd currents: trap, ten retries, reset to climatology + U_init
        ob.a["U"][2::3, 1:4] = 40.0
    k3, ob = _case(mk, 60, nz, dict(clim_present=1), prep, nsteps=1, grid="stretched" if nz == 69 else "uniform")
    clim = 8.0 + 10.0 * np.exp(-np.arange(nz + 1) / 15.0)
    assert np.array_equal(np.asarray(k3.X[2, :, 0]), clim)      # a failed column came back as the climatology
    kc = mk.KppConstFields(nz)
    kc.clim_present = 1
    mk.mckpp_physics_lookup(kc)
    ctx = mk.MckppHip(kc)
    assert ctx.kernel_name == "k_column_ps"
    ctx.close()
    _case(mk, 60, nz, dict(clim_present=1), prep, nsteps=3, grid="stretched" if nz == 69 else "uniform")


@pytest.mark.parametrize("grid", ["uniform", "stretched"])
def test_prescribed_advection_modes(mk, grid):
    def prep(k3, ob):
        n = k3.npts
        for c in range(n):
            mode = 1 + (c % 7)
            k3.nmodeadv[c, 1] = 2
            k3.modeadv[c, 0, 1] = mode
            k3.modeadv[c, 1, 1] = 1 + ((c + 3) % 7)
            k3.advection[c, 0, 1] = 1e-6 * (1 + c % 5)
            k3.advection[c, 1, 1] = -5e-7
        ob["nmodeadv"][:, 1] = k3.nmodeadv[:, 1]
        ob["modeadv"][:, 1, :] = k3.modeadv[:, :, 1]
        ob["advection"][:, 1, :] = k3.advection[:, :, 1]
    nz = 60 if grid == "uniform" else 69
    _case(mk, 70, nz, dict(L_ADVECT=1), prep, grid=grid)


@pytest.mark.parametrize("nz,switches", [(40, {}), (69, {}), (40, dict(L_FCORR_WITHZ=1))])
def test_vary_bottom_temp(mk, nz, switches):
    """L_VARY_BOTTOM_TEMP: mckpp_physics_overrides_bottomtemp after the column loop
    (src/mckpp_physics_driver_mod.F90:67-71, src/mckpp_physics_overrides.F90:12-24), on the default
    kernels (which carry no correction rows of their own) and next to an ocnint correction switch."""
    from oracle import orc

    ncol = 77
    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, **switches)
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=6)
    for k, v in switches.items():
        setattr(kc, k, v)
    kc.L_VARY_BOTTOM_TEMP = 1
    if switches:
        z = np.arange(nz + 1)[None, :]
        _set2(k3, ob, "fcorr_withz", 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, ncol)[:, None])
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    orc.init_ocean(oc, ob, 0)
    active = np.nonzero(k3.run_physics)[0]
    sf = cm.synth.forcing(ncol, "bench")
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    for nt in (1, 2, 3):
        bt = np.asarray(k3.X[:, nz, 0]) + 0.25 * np.sin(np.arange(ncol) + nt)
        k3.bottom_temp[:] = bt
        ctx = mk.mckpp_physics_driver(k3, kc, nt)
        orc.physics_driver(oc, ob, nt)
        orc.bottomtemp(oc, ob, bt)
        res = cm.compare(k3, ob, nz, FIELDS, active)
        bad = {k: v for k, v in res.items() if v[2] != 0}
        assert not bad, f"bottomtemp {switches} step {nt}: {bad}"
        assert np.array_equal(k3.X[active, nz, 0], bt[active])
        assert np.any(k3.ocnTcorr[active, nz] != 0)
    land = np.nonzero(k3.run_physics == 0)[0]
    assert np.all(k3.tinc_fcorr[land] == 0)
    ctx.set_diagnostics(0)
    with pytest.raises(mk.MckppHipError):
        ctx.bottomtemp(k3.bottom_temp)


@pytest.mark.parametrize("nz", [30, 69, 100, 150, 200, 509])
def test_options_on_other_depths(mk, nz):
    """The optional physics where a slot's items span one to three wavefronts (k_column_ps<EXT>): the level
    counts of check_profile (damped levels, frozen levels), the isotherm sums and the double-diffusion
    neighbours cross wave boundaries here."""
    nzp1 = nz + 1
    z = np.arange(nzp1)[None, :]

    def check_kernel(k3, ob):
        pass

    # double diffusion: fingering-favourable salinity on half of the columns, all the way down
    def prep_ldd(k3, ob):
        S = np.asarray(k3.X[:, :, 1]).copy()
        S[::2] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
        k3.X[:, :, 1] = S
        ob.a["S"][:, 1:nzp1 + 1] = S
    _case(mk, 40, nz, dict(LDD=1), prep_ldd, nsteps=2)

    # current damping with strong deep currents (levels beyond the first wave are damped too)
    def prep_damp(k3, ob):
        k3.U[::2, min(60, nz - 8):, 0] = 3.0
        k3.U[1::4, min(66, nz - 4):, 1] = -2.5
        ob.a["U"][:, 1:nzp1 + 1] = k3.U[:, :, 0]
        ob.a["V"][:, 1:nzp1 + 1] = k3.U[:, :, 1]
    k3, ob = _case(mk, 40, nz, dict(L_DAMP_CURR=1, dt_uvdamp=360), prep_damp, nsteps=2)
    assert np.any(k3.dampu_flag > 0) or np.any(k3.dampv_flag > 0)

    # freeze clamp over the whole depth, isotherm check over 80 levels, climatology reset after a trap
    def prep_frz(k3, ob):
        T = np.asarray(k3.X[:, :, 0]).copy()
        T[::3, :] = -2.2
        T[1::3, :] = 12.0
        k3.X[:, :, 0] = T
        ob.a["T"][:, 1:nzp1 + 1] = T
        _set2(k3, ob, "ocnT_clim", 8.0 + 10.0 * np.exp(-np.arange(nzp1) / 15.0)[None, :] * np.ones((k3.npts, 1)))
        _set2(k3, ob, "sal_clim", np.asarray(k3.X[:, :, 1]) * 0.5)
        k3.U[2::3, 0:3, 0] = 40.0
        ob.a["U"][2::3, 1:4] = 40.0
    sw = dict(L_NO_FREEZE=1, L_NO_ISOTHERM=1, clim_present=1, iso_bot=min(80, nz - 2), iso_thresh=0.002)
    k3, ob = _case(mk, 42, nz, sw, prep_frz, nsteps=1)
    assert np.any(k3.freeze_flag > 0.99) and np.any(k3.reset_flag < 0) and np.any(np.abs(k3.reset_flag) == 999)
    _case(mk, 42, nz, sw, prep_frz, nsteps=3)

    # relaxation and flux corrections with depth
    def prep_rel(k3, ob):
        n = k3.npts
        _set2(k3, ob, "ocnT_clim", np.asarray(k3.X[:, :, 0]) - 0.3)
        _set2(k3, ob, "sal_clim", np.asarray(k3.X[:, :, 1]) + 0.05)
        r = np.full(n, 1.0 / (30 * 86400.0))
        k3.relax_ocnT[:] = r; ob["relax_ocnT"] = r
        k3.relax_sal[:] = 2 * r; ob["relax_sal"] = 2 * r
        _set2(k3, ob, "fcorr_withz", 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, n)[:, None])
        _set2(k3, ob, "sfcorr_withz", 1e-7 * np.cos(z / 7.0) * np.ones((n, 1)))
    k3, ob = _case(mk, 40, nz, dict(L_RELAX_OCNT=1, L_RELAX_SAL=1, L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1), prep_rel)
    assert np.any(k3.ocnTcorr[:, min(64, nz - 2):] != 0) and np.any(k3.scorr[:, min(64, nz - 2):] != 0)

    # prescribed advection, all seven modes
    def prep_adv(k3, ob):
        for c in range(k3.npts):
            k3.nmodeadv[c, 1] = 2
            k3.modeadv[c, 0, 1] = 1 + (c % 7)
            k3.modeadv[c, 1, 1] = 1 + ((c + 3) % 7)
            k3.advection[c, 0, 1] = 1e-6 * (1 + c % 5)
            k3.advection[c, 1, 1] = -5e-7
        ob["nmodeadv"][:, 1] = k3.nmodeadv[:, 1]
        ob["modeadv"][:, 1, :] = k3.modeadv[:, :, 1]
        ob["advection"][:, 1, :] = k3.advection[:, :, 1]
    _case(mk, 42, nz, dict(L_ADVECT=1), prep_adv, grid="stretched" if nz == 69 else "uniform")


@pytest.mark.parametrize("nz,sw", [(40, dict(LRI=0)), (69, dict(LRI=0)), (60, dict(LRI=0, LDD=1)), (40, dict(LRI=0, L_DAMP_CURR=1, dt_uvdamp=360))])
def test_without_the_richardson_mixing(mk, nz, sw):
    """LRI=.FALSE. (src/mckpp_physics_verticalmixing_kppmix_mod.F90:65-74): rimix is not called, the interior
    diffusivities stay at the zeros kppmix starts from (double diffusion adds to those), Rig is not formed; the
    boundary-layer scheme and the solves run on that.  Default and optional-physics builds."""
    def prep(k3, ob):
        if sw.get("LDD"):
            S = np.asarray(k3.X[:, :, 1]).copy()
            S[::2] = 0.4 - 0.8 * np.linspace(0, 1, nz + 1)[None, :]
            k3.X[:, :, 1] = S
            ob.a["S"][:, 1:nz + 2] = S
    k3, ob = _case(mk, 60, nz, sw, prep, nsteps=3, grid="stretched" if nz == 69 else "uniform")
    assert np.all(np.asarray(k3.Rig) == 0.0)          # never written
    assert np.any(np.asarray(k3.difm)[:, 1:nz] == 0.0)   # below the boundary layer


def test_lkpp_false_is_refused_with_the_reason(mk):
    kc = mk.KppConstFields(40)
    kc.LKPP = 0
    mk.mckpp_physics_lookup(kc)
    with pytest.raises(mk.MckppHipError, match="unassigned in the reference"):
        mk.MckppHip(kc)


def test_optional_physics_kernel_selection(mk):
    for nz, want in [(40, "k_column_ps<EXT>"), (60, "k_column_ps<EXT>"), (69, "k_column_ps<EXT>"), (150, "k_column_ps<EXT>")]:
        kc = mk.KppConstFields(nz)
        kc.L_DAMP_CURR = 1
        mk.mckpp_physics_lookup(kc)
        ctx = mk.MckppHip(kc)
        assert ctx.kernel_name == want, (nz, ctx.kernel_name)
        ctx.close()


def test_restart_and_ancillary_update_on_optional_physics_context(mk, tmp_path):
    """A restart file loaded into a fresh optional-physics context: stepping is refused until the
    relaxation inputs are resident (mckpp_hip_update_ancillaries), then continues bit-identically;
    a changed ancillary (SST0 / climatology, what mckpp_boundary_update rewrites between steps,
    src/mckpp_ocean_model_3D.F90:51-55) reaches the device without touching the prognostic state."""
    from oracle import orc

    ncol, nz = 96, 40
    sw = dict(L_RELAX_SST=1, L_RELAX_OCNT=1)

    def fill(k3, ob, dT):
        n = k3.npts
        r = np.full(n, 1.0 / (5 * 86400.0))
        k3.relax_sst[:] = r
        k3.relax_ocnT[:] = r / 6
        k3.SST0[:] = T0[:, 0] + dT
        k3.ocnT_clim[:, :] = T0 - 0.3 + dT
        if ob is not None:
            ob["relax_sst"] = r; ob["relax_ocnT"] = r / 6; ob["SST0"] = T0[:, 0] + dT
            ob.a["ocnT_clim"][:, 1:nz + 2] = T0 - 0.3 + dT

    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, **sw)
    kc, k3 = cm.make_hip_case(ncol, nz, land_every=7)
    for k, v in sw.items():
        setattr(kc, k, v)
    T0 = np.asarray(k3.X[:, :, 0]).copy()
    fill(k3, ob, 1.5)
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    orc.init_ocean(oc, ob, 0)
    sf = cm.synth.forcing(ncol, "bench")
    ob["sflux"] = sf
    cm.set_forcing_3d(k3, sf)
    ctx.set_forcing(k3.sflux)
    ctx.step(1, 2)
    for nt in (1, 2):
        orc.physics_driver(oc, ob, nt)
    rst = tmp_path / "ext.restart"
    ctx.save_restart(rst)

    # (a) ancillaries change on the host between steps: only they are re-uploaded
    fill(k3, ob, 0.4)
    ctx.update_ancillaries(k3)
    ctx.step(3, 1)
    orc.physics_driver(oc, ob, 3)
    ctx.download(k3)
    ocean = np.flatnonzero(k3.run_physics)
    res = cm.compare(k3, ob, nz, cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["fcorr", "tinc_fcorr", "ocnTcorr"], active=ocean)
    assert not {k: v for k, v in res.items() if v[2] != 0}, res

    # (b) fresh optional-physics context + restart file
    kc2, k3b = cm.make_hip_case(ncol, nz, land_every=7)
    for k, v in sw.items():
        setattr(kc2, k, v)
    ctx2 = mk.MckppHip(kc2)
    ctx2.load_restart(rst, ncol)
    with pytest.raises(mk.MckppHipError, match="update_ancillaries"):
        ctx2.step(3, 1)
    fill(k3b, None, 0.4)
    ctx2.update_ancillaries(k3b)
    cm.set_forcing_3d(k3b, sf)
    ctx2.step(3, 1)
    ctx2.download(k3b)
    for n in ("U", "X", "Us", "Xs", "hmix", "kmix", "Tref", "fcorr", "tinc_fcorr", "ocnTcorr"):
        assert np.array_equal(getattr(k3, n)[ocean], getattr(k3b, n)[ocean]), n

    # (c) a file with a corrupt column map or a truncated tail is refused and the resident state survives
    raw = bytearray(rst.read_bytes())
    hdr = 8 + 6 * 4 + 2 * 8
    bad = bytearray(raw)
    bad[hdr:hdr + 4] = (10 ** 6).to_bytes(4, "little")          # ipt[0] far outside npts
    (tmp_path / "badmap").write_bytes(bad)
    with pytest.raises(mk.MckppHipError, match="column map"):
        ctx2.load_restart(tmp_path / "badmap", ncol)
    (tmp_path / "short").write_bytes(raw[:len(raw) // 2])
    with pytest.raises(mk.MckppHipError, match="truncated"):
        ctx2.load_restart(tmp_path / "short", ncol)
    k3c = cm.make_hip_case(ncol, nz, land_every=7)[1]
    ctx2.download(k3c)
    assert np.array_equal(k3c.X[ocean], k3b.X[ocean]) and np.array_equal(k3c.hmix[ocean], k3b.hmix[ocean])
    ctx2.close()


# the switch families pinned to the reference's own physics step (tests/ref_step_cases.py, recorded outputs of the
# portable-exp build in tests/golden/ref_step.npz): bit for bit on every field after every step
_REF_STEP_SWITCH_CASES = [t for t, c in __import__("ref_step_cases").CASES.items()
                          if (c.switches or c.bottom_temp) and not t.startswith("nz40_")]


@pytest.mark.parametrize("tag", _REF_STEP_SWITCH_CASES)
def test_switches_match_the_reference_step(mk, tag):
    import ref_step_cases as rc

    golden = rc.Golden()
    case = rc.CASES[tag]
    for nt, got in rc.run_hip(mk, tag, golden):
        bad = rc.mismatches(case, golden.digests(tag, "pexp"), golden.values(tag), nt, got.__getitem__)
        assert not bad, f"{tag} step {nt}: HIP differs from the reference's own step: {bad}"


# ---------------------------------------------------------------------------------------------------------------
# prescribed advection (tests/ref_step_cases.py, "prescribed advection"): the recorded cases through the other launch
# forms, the ancillary update, and the two inputs the reference has no defined behaviour for
# ---------------------------------------------------------------------------------------------------------------
_VIEWS_FORCED = {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}
_ADVECTION_FORMS = (
    [(t, {}) for t in __import__("ref_step_cases").ADVECTION_CASES]           # all steps in one call
    + [("adv_modes_nz40", {"MCKPP_MULTISTEP": "0"}),
       ("adv_modes_nz60", {"MCKPP_PS_FIXED_L": "0"}),                         # the general kernel at 60 levels
       ("adv_modes_nz69_stretched", {"MCKPP_PS_FIXED_L": "0"}),
       ("adv_modes_nz60", _VIEWS_FORCED), ("adv_modes_nz69_stretched", _VIEWS_FORCED), ("adv_edges_nz40", _VIEWS_FORCED),
       ("adv_edges_120m", {"MCKPP_PS": "21x4x1"}), ("adv_edges_90m", {"MCKPP_PS": "21x4x1"})])   # the most slots


@pytest.mark.parametrize("tag,env", _ADVECTION_FORMS,
                         ids=[f"{t}-{'-'.join(f'{k[6:]}={v}' for k, v in e.items()) or 'default'}" for t, e in _ADVECTION_FORMS])
def test_advection_cases_through_the_launch_forms(mk, monkeypatch, tag, env):
    """All steps of an advection case in ONE call - km = kmix moves between the steps inside the launch, and the
    per-item range tests of the kernel's rhsmod have to follow it - against the reference's recorded last step: the
    launcher's own choice, the general kernel where the depth has one with the level count as a literal, the forced
    views, and a forced workgroup geometry of 21 slots."""
    import ref_step_cases as rc

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    golden = rc.Golden()
    case = rc.CASES[tag]
    kc, k3, ctx, oc, ob = rc.start_hip(mk, tag, golden)
    cm.set_forcing_3d(k3, rc.forcing(case, 1))      # (the advection cases' forcing is the same at every step)
    ctx.set_forcing(k3.sflux)
    ctx.step(1, case.nsteps)
    ctx.download(k3)
    got = rc.hip_fields(k3, ctx, case.nz)
    if "MCKPP_PS" in env:
        assert ctx.kernel_residency()[2] == 64 * int(env["MCKPP_PS"].split("x")[1])
    bad = rc.mismatches(case, golden.digests(tag, "pexp"), golden.values(tag), case.nsteps, got.__getitem__)
    assert not bad, f"{tag} {env}: HIP differs from the reference's own step {case.nsteps}: {bad}"


@pytest.mark.parametrize("tag", ["adv_modes_nz40", "adv_modes_nz60", "adv_edges_nz40"])
def test_advection_with_the_two_ended_solver(mk, tag):
    """Solver mode 1 on the advection cases: within rounding of the recorded reference (the same mixed-layer index,
    T and hmix as test_two_ended_solver_within_rounding_of_the_reference_step asks), and bit for bit the oracle's
    restatement of that mode on every field, S among them."""
    import ref_step_cases as rc

    golden = rc.Golden()
    case, ref = rc.CASES[tag], golden.values(tag)
    act = rc.active_columns(case)
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=1, solver_mode=1)
    for (nt, got), _ in zip(rc.run_hip(mk, tag, golden, solver_mode=1), rc.run_oracle(case, oc, ob)):
        bad = [n for n in rc.STEP_FIELDS if not np.array_equal(
            rc.canonical(got[n])[act].view(np.int64), rc.canonical(rc.field_of(ob, n, case.nz))[act].view(np.int64))]
        assert not bad, f"{tag} solver 1 step {nt}: HIP differs from the oracle in {bad}"
        assert np.array_equal(got["status"][act], ob["status"][act]) and np.array_equal(got["npasses"][act], ob["npasses"][act])
    assert np.array_equal(got["kmix"][act], ref["kmix"])
    assert np.allclose(got["hmix"][act], ref["hmix"], rtol=1e-10, atol=0)
    assert np.abs(got["T"][act] - ref["T"]).max() <= 1e-10 * np.abs(ref["T"]).max()


def _advection_prep(hook):
    """prep(k3, ob) for _case: a hook of tests/ref_step_cases.py on both sides"""
    import ref_step_cases as rc

    def prep(k3, ob):
        rc.apply_both(ob, k3, ob.nzp1, hook(k3.npts, ob.nzp1, ob))
    return prep


@pytest.mark.parametrize("nz", [150, 200])
def test_advection_slot_patterns_where_a_slot_spans_several_wavefronts(mk, nz):
    """The slot patterns of the recorded cases (all six slots, a mode twice, holes, dead slots) at depths where a
    slot's items span two and three wavefronts, three steps against the oracle."""
    import ref_step_cases as rc

    k3, ob = _case(mk, 42, nz, dict(L_ADVECT=1), _advection_prep(rc._adv_patterns), nsteps=3)
    assert len(set(ob["kmix"].tolist())) >= 3


def test_update_ancillaries_with_other_advection_modes(mk):
    """Modes and magnitudes change on the host between two steps (what an ancillary reader does): after
    update_ancillaries the next step uses the new ones, bit for bit with the oracle, and the prognostic state is
    untouched by the update itself."""
    import ref_step_cases as rc
    from oracle import orc

    tag = "adv_modes_nz60"
    golden = rc.Golden()
    case = rc.CASES[tag]
    act = rc.active_columns(case)
    kc, k3, ctx, oc, ob = rc.start_hip(mk, tag, golden)
    sf = rc.forcing(case, 1)
    cm.set_forcing_3d(k3, sf)
    ob["sflux"] = sf
    ctx.set_forcing(k3.sflux)
    ctx.step(1, 1)
    orc.physics_driver(oc, ob, 1)
    ctx.download(k3)
    state = ("U", "X", "Us", "Xs", "hmix", "kmix", "hmixd", "Tref", "Ssurf", "old", "new_")
    before = {n: np.array(getattr(k3, n), copy=True) for n in state}
    new = rc.advection_inputs(case.ncol, lambda c: rc.ADV_PATTERNS[(c + 3) % 7])
    new["advection"] = -1.5 * new["advection"]
    rc.apply_both(ob, k3, case.nz + 1, new)
    ctx.update_ancillaries(k3)
    ctx.download(k3)
    for n, v in before.items():
        assert np.array_equal(getattr(k3, n), v), f"update_ancillaries changed {n}"
    ctx.step(2, 1)
    orc.physics_driver(oc, ob, 2)
    ctx.download(k3)
    st, _, npass = ctx.status()
    assert np.array_equal(st[act], ob["status"][act]) and np.array_equal(npass[act], ob["npasses"][act])
    bad = {k: v for k, v in cm.compare(k3, ob, case.nz, rc.STEP_FIELDS, act).items() if v[2] != 0}
    assert not bad, f"step 2 after the update: {bad}"
    got = rc.hip_fields(k3, ctx, case.nz)
    assert "S" in rc.mismatches(case, golden.digests(tag, "pexp"), {}, 2, got.__getitem__), \
        "step 2 is the recorded one of the old modes: the update never reached the kernel"


@pytest.mark.parametrize("grid", ["uniform_90", "thin"])
def test_mode_4_on_a_grid_shallower_than_100_m_is_a_no_op(mk, grid):
    """rhsmod's mode 4 looks for the first level below 100 m without a bound (solvers.F90:258-259): on a grid that has
    none, the reference reads past zm - it has NO DEFINED BEHAVIOUR for this input, and no such column is recorded.
    The column kernel stops the search at nzp1 and adds nothing; the oracle has the same guard.  Device against
    oracle, and against an oracle that was given no advection at all on the columns that have mode 4 alone."""
    import ref_step_cases as rc
    from oracle import orc

    ncol, nz = 28, 12

    def hook(n, nzp1, ob):       # mode 4 alone on the even columns, beside each of the others on the odd ones
        return rc.advection_inputs(n, lambda c: ((4,), 1) if c % 2 == 0 else ((4, 1 + c % 7, 4), 3))
    k3, ob = _case(mk, ncol, nz, dict(L_ADVECT=1), _advection_prep(hook), nsteps=2, grid=grid)
    oc, plain = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid)
    orc.init_ocean(oc, plain, 0)
    plain["sflux"] = cm.synth.forcing(ncol, "bench")
    for nt in (1, 2):
        orc.physics_driver(oc, plain, nt)
    assert np.array_equal(np.asarray(k3.X)[0::2, :, 1], plain["S"][0::2, 1:nz + 2])
    assert not np.array_equal(np.asarray(k3.X)[1::2, :, 1], plain["S"][1::2, 1:nz + 2])


def test_an_advection_mode_above_7_is_refused(mk):
    """The reference aborts on a live slot whose mode is above 7 (solvers.F90:320-323); the kernel would skip it in
    silence.  The upload and update_ancillaries refuse it, naming the point and the slot; a slot behind nmodeadv may
    hold anything; a good upload afterwards runs to the recorded state."""
    import ref_step_cases as rc

    tag = "adv_edges_120m"
    golden = rc.Golden()
    case = rc.CASES[tag]
    kc, k3, ctx, oc, ob = rc.start_hip(mk, tag, golden)
    good = np.array(k3.modeadv, copy=True)
    k3.modeadv[5, 1, 1] = 8                      # point 6, slot 2 of nmodeadv(6,2) = 2
    with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_upload: modeadv\(6,2,2\)=8 "):
        ctx.upload(k3)
    with pytest.raises(mk.MckppHipError, match=r"mckpp_hip_update_ancillaries: modeadv\(6,2,2\)=8 "):
        ctx.update_ancillaries(k3)
    k3.modeadv[...] = good
    k3.modeadv[5, 2, 1] = 8                      # behind the live slots: ignored by the reference, accepted here
    ctx.upload(k3)
    for nt in range(1, case.nsteps + 1):
        cm.set_forcing_3d(k3, rc.forcing(case, nt))
        ctx.set_forcing(k3.sflux)
        ctx.step(nt, 1)
        ctx.download(k3)
        bad = rc.mismatches(case, golden.digests(tag, "pexp"), golden.values(tag), nt,
                            rc.hip_fields(k3, ctx, case.nz).__getitem__)
        assert not bad, f"{tag} step {nt} after the refused uploads: {bad}"
