"""The reference-pinned step cases: seeded starting states, built by tests/common.py's generators and the oracle's
init_ocean (which the HIP init matches bit for bit), on which the compiled reference's own physics step is recorded
(tests/golden/make_ref_step_golden.py -> tests/golden/ref_step.npz) and against which the oracle
(tests/test_ref_step_cpu.py) and the HIP kernel (tests/test_parity_gpu.py, tests/test_options_gpu.py) are asserted bit
for bit.

A case is a name -> Case.  `pre` fills optional inputs before init_ocean, `post` perturbs the state after it (the
instability trap); both return {batch field: array} so the same values go to the oracle batch and to the HIP
Kpp3dFields (`apply_hip`)."""
import hashlib
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

import common as cm
from oracle import orc

# every field the reference's kpp_3d_fields carries and the suite compares (tests/test_parity_gpu.py: ALL_FIELDS,
# plus the option outputs and the step bookkeeping)
STEP_FIELDS = (cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["hmixd0", "hmixd1"] + list(cm.DIAG_FIELDS.keys())
               + cm.EXT_SCALARS)
INPUT_FIELDS = list(orc.LEVEL_FIELDS) + list(orc.SCALAR_FIELDS) + ["old", "newi", "jerlov", "l_initflag", "l_ocean",
                                                                    "hmixd", "nmodeadv", "modeadv", "advection"]


@dataclass
class Case:
    ncol: int
    nz: int
    nsteps: int
    grid: str = "uniform"
    dto: float = 3600.0
    switches: dict = field(default_factory=dict)
    pre: Optional[Callable] = None          # (ncol, nzp1, ob) -> {field: array}, before init_ocean
    post: Optional[Callable] = None         # (ncol, nzp1, ob) -> {field: array}, after init_ocean
    stress: Optional[Callable] = None       # (ncol) -> (taux, tauy) in place of the bench mix's wind stress
    land_every: int = 0                     # run_physics = l_ocean = 0 on every land_every-th column
    jerlov_mix: bool = False
    diurnal: bool = False                   # short-wave follows the sun, step by step
    bottom_temp: bool = False               # L_VARY_BOTTOM_TEMP with a bottom temperature 0.5 K below the deepest level
    full: bool = True                       # record T, hmix, kmix of the last step in full too (else: digests only)


def _relax_sst(ncol, nzp1, ob):
    r = np.full(ncol, 1.0 / (5 * 86400.0))
    r[::4] = 0.0
    return {"relax_sst": r, "SST0": ob["T"][:, 1] + 1.5}


def _fcorr_twod(ncol, nzp1, ob):
    return {"fcorr_twod": np.linspace(-80.0, 80.0, ncol)}


def _fcorr_withz(ncol, nzp1, ob):
    z = np.arange(nzp1)[None, :]
    return {"fcorr_withz": 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, ncol)[:, None],
            "sfcorr_withz": 1e-7 * np.cos(z / 7.0) * np.ones((ncol, 1))}


def _relax_ocnt_sal(ncol, nzp1, ob):
    r = np.full(ncol, 1.0 / (30 * 86400.0))
    return {"ocnT_clim": ob["T"][:, 1:nzp1 + 1] - 0.3, "sal_clim": ob["S"][:, 1:nzp1 + 1] + 0.05,
            "relax_ocnT": r, "relax_sal": 2 * r}


def _salt_fingers(ncol, nzp1, ob):
    S = ob["S"][:, 1:nzp1 + 1].copy()
    S[::2] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
    return {"S": S}


def _freeze_isotherm(ncol, nzp1, ob):
    T = ob["T"][:, 1:nzp1 + 1].copy()
    T[::3, :] = -2.2
    T[1::3, :] = 12.0
    return {"T": T, "ocnT_clim": 8.0 + 10.0 * np.exp(-np.arange(nzp1) / 15.0)[None, :] * np.ones((ncol, 1)),
            "sal_clim": ob["S"][:, 1:nzp1 + 1] * 0.5}


def _trap(ncol, nzp1, ob):
    U = ob["U"][:, 1:nzp1 + 1].copy()
    U[::4, 0:4] = 50.0
    return {"U": U}


def _trap_clim(ncol, nzp1, ob):
    d = _trap(ncol, nzp1, ob)
    d["ocnT_clim"] = ob["T"][:, 1:nzp1 + 1] - 0.25
    d["sal_clim"] = ob["S"][:, 1:nzp1 + 1] + 0.01
    return d


# ---------------------------------------------------------------------------------------------------------------
# the physics regimes the generators of tests/common.py never reach by themselves ("Regimes"): each hook
# below is a closed form of the column index; test_the_cases_reach_what_they_are_for asserts through the oracle's
# `paths` word that the branch a case is named after is really taken
# ---------------------------------------------------------------------------------------------------------------
def bathymetry(ncol, shallow, deep, every=1):
    """ocdepth = -linspace(shallow, deep) on every `every`-th column (from column every-1), -10000 elsewhere"""
    d = np.full(ncol, -10000.0)
    sel = np.arange(every - 1, ncol, every)
    d[sel] = -np.linspace(shallow, deep, len(sel))
    return d


def _bathymetry(shallow, deep):
    return lambda ncol, nzp1, ob: {"ocdepth": bathymetry(ncol, shallow, deep)}


# -ocdepth on level centres of the 40-level grid (2.5, 7.5: `hmin < -zm(k)` is strict), on an interface (10), just
# past a centre (2.6) and above the first centre (0.01 ... 2: hbl shallower than level 1, kbl = 2, blmix with kn = 1)
SEAFLOOR_EDGES = (2.5, 7.5, 10.0, 2.6, 0.01, 0.5, 1.0, 2.0)


def _seafloor_edges(ncol, nzp1, ob):
    return {"ocdepth": -np.resize(np.array(SEAFLOOR_EDGES), ncol)}


def isothermal(T, S):
    """T(k) = T(1) - 1e-4 k, S = 0: nothing but the surface forcing decides how deep a column mixes"""
    return T[:, 0:1] - 1e-4 * np.arange(T.shape[1])[None, :], np.zeros_like(S)


def tjump(T):
    """a 12 K step down between levels 9 and 10: |T(k) - T(k+1)| >= 10 on every retry"""
    T = T.copy()
    T[:, 9:] -= 12.0
    return T


def _profiles(ob, nzp1):
    return (ob[k][:, 1:nzp1 + 1].copy() for k in "TSUV")


def _isothermal(ncol, nzp1, ob):
    T, S, _, _ = _profiles(ob, nzp1)
    T, S = isothermal(T, S)
    return {"T": T, "S": S}


def _isothermal_bathymetry(ncol, nzp1, ob):
    d = _isothermal(ncol, nzp1, ob)
    d["ocdepth"] = bathymetry(ncol, 3.0, 260.0, every=2)       # the deepest lie below the 200 m grid
    return d


def _tjump(ncol, nzp1, ob):
    T, _, _, _ = _profiles(ob, nzp1)
    T[::3] = tjump(T[::3])
    return {"T": T}


def _tjump_clim(ncol, nzp1, ob):
    d = _tjump(ncol, nzp1, ob)
    d["ocnT_clim"] = ob["T"][:, 1:nzp1 + 1] - 0.25
    d["sal_clim"] = ob["S"][:, 1:nzp1 + 1] + 0.01
    return d


def _stress_ramp(ncol):
    """a wind stress from 0.5 to 6 N/m2 across the columns, eastward on the even and northward on the odd ones: on the
    10 m grid the rms change of U (of V) over a step crosses its threshold of 1 m/s inside the ramp, while no level
    reaches 10 m/s"""
    ramp = np.linspace(0.5, 6.0, ncol)
    even = np.arange(ncol) % 2 == 0
    return np.where(even, ramp, 1e-3), np.where(even, 0.0, ramp)


def _moving(ncol, nzp1, ob):
    """2 m/s in U and V at every level: the Coriolis term is a good part of a step's change, so that the retries'
    f * 1.01 moves the rms change - columns just past the threshold are retried and then accepted"""
    return {"U": np.full((ncol, nzp1), 2.0), "V": np.full((ncol, nzp1), 2.0)}


def diffconv(T, S):
    """cold fresh water over warm salty water, the warmth outweighing the salt (alphaDT < betaDS < 0: what the
    reference's ddmix takes for diffusive convection, ddmix_mod.F90:39)"""
    k = np.linspace(0.0, 1.0, T.shape[1])[None, :]
    return 4.0 + 8.0 * k + 0 * T, -0.25 + 0.5 * k + 0 * S


def _diffconv(ncol, nzp1, ob):
    T, S, _, _ = _profiles(ob, nzp1)
    T[::2], S[::2] = diffconv(T[::2], S[::2])
    S[1::2] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]       # salt fingers on the others
    return {"T": T, "S": S}


SWEEP_SEED, LID = 20261016, 4
SWEEP_REGIMES = ("plain", "seafloor", "isothermal", "isothermal_seafloor", "tjump", "diffconv", "fingers", "spun_up",
                 "cold_lid", "salty_lid", "trap_u")


def sweep_regimes(ncol):
    """regime name -> the columns of the seeded sweep that have it (a shuffled, even deal of SWEEP_REGIMES)"""
    reg = np.random.default_rng(SWEEP_SEED).permutation(np.arange(ncol) % len(SWEEP_REGIMES))
    return {name: np.nonzero(reg == i)[0] for i, name in enumerate(SWEEP_REGIMES)}


def _sweep(ncol, nzp1, ob):
    """every regime above side by side in one batch, dealt over the columns by a seeded shuffle; and three that only
    the sweep has: a column moving at 7 m/s at every level (Coriolis turns it by more than 1 m/s rms in a step:
    the rms check on U and V), and a lid of four levels 9.5 K colder / 8 psu saltier than the water below it (convection
    changes T / S by more than 1 rms over the column in a step: the rms check on T and S)"""
    reg = sweep_regimes(ncol)
    T, S, U, V = _profiles(ob, nzp1)
    d = np.full(ncol, -10000.0)
    d[reg["seafloor"]] = -np.linspace(0.5, 40.0, len(reg["seafloor"]))
    iso = np.concatenate([reg["isothermal"], reg["isothermal_seafloor"]])
    T[iso], S[iso] = isothermal(T[iso], S[iso])
    d[reg["isothermal_seafloor"]] = -np.linspace(3.0, 260.0, len(reg["isothermal_seafloor"]))
    T[reg["tjump"]] = tjump(T[reg["tjump"]])
    T[reg["diffconv"]], S[reg["diffconv"]] = diffconv(T[reg["diffconv"]], S[reg["diffconv"]])
    S[reg["fingers"]] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
    U[reg["spun_up"]], V[reg["spun_up"]] = 7.0, 7.0
    T[reg["cold_lid"], :LID] -= 9.5
    S[reg["salty_lid"], :LID] += 8.0
    return {"T": T, "S": S, "U": U, "V": V, "ocdepth": d}


def regime_mix(ncol, nzp1, ob):
    """The sea-floor, full-depth and T-jump regimes side by side, by column index modulo 8 (so that the workgroups of
    a large batch hold columns of different regimes next to each other, at every latitude): 0, 4 the plain
    stratified start; 1, 5 shallow bathymetry (0.5 ... 40 m); 2 near-isothermal; 6 near-isothermal over bathymetry
    from 3 m to below the grid; 3 the 12 K temperature step (trapped: 11 tries of 6 passes, every step); 7 the
    stratified start over bathymetry between 20 and 150 m."""
    T, S, _, _ = _profiles(ob, nzp1)
    i = np.arange(ncol)
    d = np.full(ncol, -10000.0)
    for r, (lo, hi) in {1: (0.5, 40.0), 5: (40.0, 0.5), 6: (3.0, 260.0), 7: (20.0, 150.0)}.items():
        d[i % 8 == r] = -np.linspace(lo, hi, int((i % 8 == r).sum()))
    iso = (i % 8 == 2) | (i % 8 == 6)
    T[iso], S[iso] = isothermal(T[iso], S[iso])
    T[i % 8 == 3] = tjump(T[i % 8 == 3])
    return {"T": T, "S": S, "ocdepth": d}


def apply_both(ob, k3, nzp1, d):
    """{batch field: array} on an oracle batch and on the HIP Kpp3dFields"""
    _apply_batch(ob, nzp1, d)
    apply_hip(k3, d)


def _sweep_trap(ncol, nzp1, ob):
    U = ob["U"][:, 1:nzp1 + 1].copy()
    U[sweep_regimes(ncol)["trap_u"], 0:4] = 50.0
    return {"U": U}


CASES = {
    "nz40": Case(32, 40, 3),
    "nz60_land_jerlov": Case(30, 60, 2, land_every=4, jerlov_mix=True),
    "nz69_stretched": Case(24, 69, 2, grid="stretched"),
    "nz100": Case(48, 100, 2, full=False),
    "nz40_dto600": Case(24, 40, 3, dto=600.0),
    "nz40_diurnal_itermax": Case(45, 40, 6, switches=dict(itermax=4), diurnal=True),
    "nz40_trap_retry": Case(24, 40, 2, post=_trap),
    "nz40_trap_clim_reset": Case(24, 40, 2, switches=dict(clim_present=1), post=_trap_clim),
    "relax_sst": Case(24, 40, 2, switches=dict(L_RELAX_SST=1), pre=_relax_sst),
    "relax_sst_calconly": Case(16, 40, 2, switches=dict(L_RELAX_SST=1, L_RELAX_CALCONLY=1), pre=_relax_sst),
    "fcorr_twod": Case(24, 40, 2, switches=dict(L_FCORR=1), pre=_fcorr_twod),
    "fcorr_withz": Case(24, 40, 2, switches=dict(L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1), pre=_fcorr_withz),
    "relax_ocnt_sal": Case(24, 60, 2, switches=dict(L_RELAX_OCNT=1, L_RELAX_SAL=1), pre=_relax_ocnt_sal),
    "ldd": Case(24, 40, 3, switches=dict(LDD=1), pre=_salt_fingers),
    "lri0": Case(24, 40, 2, switches=dict(LRI=0)),
    "damp_curr": Case(24, 40, 2, switches=dict(L_DAMP_CURR=1, dt_uvdamp=360)),
    "nofreeze_isotherm_clim": Case(24, 40, 2, switches=dict(L_NO_FREEZE=1, L_NO_ISOTHERM=1, clim_present=1),
                                   pre=_freeze_isotherm),
    "bottom_temp": Case(24, 40, 2, bottom_temp=True),
    # the seeded sweep: a model day of a sunlit, mixed-Jerlov 2000-column batch
    "sweep_2000x24": Case(2000, 60, 24, jerlov_mix=True, diurnal=True, full=False),
    # the regimes: the sea floor clamps the boundary layer ...
    "seafloor_nz40": Case(60, 40, 3, pre=_bathymetry(3.0, 40.0)),
    "seafloor_nz69_stretched": Case(60, 69, 3, grid="stretched", dto=1200.0, pre=_bathymetry(3.0, 40.0), land_every=5,
                                    jerlov_mix=True, diurnal=True),
    "seafloor_edges_nz40": Case(24, 40, 3, pre=_seafloor_edges),
    # ... columns mix down to the last level of the grid ...
    "seafloor_fulldepth_nz60": Case(96, 60, 3, pre=_isothermal_bathymetry),
    "fulldepth_nz100": Case(48, 100, 3, pre=_isothermal),
    # ... the instability trap fires on a temperature jump, and on the rms change of a step ...
    "tjump_trap_nz40": Case(60, 40, 2, pre=_tjump),
    "tjump_trap_clim_nz40": Case(30, 40, 2, switches=dict(clim_present=1), pre=_tjump_clim),
    "rms_retry_thin_grid": Case(96, 12, 2, grid="thin", pre=_moving, stress=_stress_ramp),
    # ... the surface salinity follows the column, double diffusion takes its diffusive-convection arm ...
    "ssref0_nz40": Case(24, 40, 3, switches=dict(L_SSref=0)),
    "ldd_diffconv_nz40": Case(24, 40, 3, switches=dict(LDD=1), pre=_diffconv),
    # ... and all of them side by side, seeded, under the bench forcing
    "regime_sweep_nz60": Case(400, 60, 4, switches=dict(LDD=1), pre=_sweep, post=_sweep_trap, jerlov_mix=True, full=False),
}


REGIME_CASES = [t for t in CASES if t.startswith(("seafloor_", "fulldepth_", "tjump_", "rms_retry_", "ssref0_",
                                                  "ldd_diffconv_", "regime_sweep_"))]


def _apply_batch(ob, nzp1, d):
    for k, v in d.items():
        if ob.a[k].ndim == 2 and k not in ("sflux", "hmixd"):
            ob.a[k][:, 1:nzp1 + 1] = v
        else:
            ob[k] = v


def apply_hip(k3, d):
    """The same {batch field: array} on the HIP Kpp3dFields."""
    m = {"U": ("U", 0), "V": ("U", 1), "T": ("X", 0), "S": ("X", 1)}
    for k, v in d.items():
        if k in m:
            a, l = m[k]
            getattr(k3, a)[:, :, l] = v
        elif k == "jerlov":
            k3.jerlov[:] = v
        else:
            getattr(k3, k)[...] = v


def forcing(case, step):
    """sflux(1:6) of model step `step` (1-based)"""
    t = step * case.dto if case.diurnal else None
    sf = cm.synth.forcing(case.ncol, "bench", t_seconds=t)
    if case.stress:
        sf[:, 0], sf[:, 1] = case.stress(case.ncol)
    return sf


def jerlov(case):
    return (1 + (np.arange(case.ncol) % 5)).astype(np.int32) if case.jerlov_mix else None


def land(case):
    """run_physics of the case (1 = ocean)"""
    rp = np.ones(case.ncol, dtype=np.int32)
    if case.land_every:
        rp[::case.land_every] = 0
    return rp


def active_columns(case):
    """indices of the columns the reference steps (all but the land columns); digests are over these"""
    return np.nonzero(land(case))[0]


def bottom_temp(case, ob):
    return ob["T"][:, case.nz + 1] - 0.5


def oracle_start(case, exp_mode=1, solver_mode=0):
    """(Const, Batch, pre, post): the oracle's state after init_ocean and the post-init perturbation, the forcing of
    step 1 set."""
    sw = dict(case.switches)
    oc, ob = cm.make_oracle(case.ncol, case.nz, init=False, exp_mode=exp_mode, grid=case.grid, dto=case.dto,
                            solver_mode=solver_mode, **sw)
    nzp1 = case.nz + 1
    pre = case.pre(case.ncol, nzp1, ob) if case.pre else {}
    j = jerlov(case)
    if j is not None:
        pre["jerlov"] = j
    _apply_batch(ob, nzp1, pre)
    orc.init_ocean(oc, ob, 0)
    post = case.post(case.ncol, nzp1, ob) if case.post else {}
    _apply_batch(ob, nzp1, post)
    ob["sflux"] = forcing(case, 1)
    return oc, ob, pre, post


def canonical(a):
    """float64 copy with -0.0 -> +0.0 and every NaN the same, as cm.compare counts those equal"""
    a = np.array(a, dtype=np.float64)
    a[a == 0] = 0.0
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a)


def digest(a):
    """SHA-256 of the canonical bytes, as the 32 uint8 the golden file stores"""
    return np.frombuffer(hashlib.sha256(canonical(a).tobytes()).digest(), dtype=np.uint8)


def field_of(ob, name, nz):
    """Batch field `name` over the range the suite compares (cm.compare), shape (ncol, count) or (ncol,)"""
    if name in ("hmixd0", "hmixd1"):
        return ob["hmixd"][:, int(name[-1])]
    if name in cm.SCALAR_FIELDS or name in cm.EXT_SCALARS:
        return ob[name]
    if name in cm.DIAG_FIELDS:
        _, _, lo, cnt = cm.DIAG_FIELDS[name]
        return ob.a[name][:, lo:lo + cnt(nz)]
    return ob.a[name][:, 1:nz + 2]


def input_digest(ob):
    """One SHA-256 over every input field of a starting state (oracle batch after init, forcing set)."""
    h = hashlib.sha256()
    for k in INPUT_FIELDS + ["sflux"]:
        h.update(k.encode())
        h.update(canonical(ob[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def run_oracle(case, oc, ob):
    """The oracle through the case's steps (ob updated in place); yields after each step."""
    bt = bottom_temp(case, ob) if case.bottom_temp else None
    for nt in range(1, case.nsteps + 1):
        ob["sflux"] = forcing(case, nt)
        orc.physics_driver(oc, ob, nt)
        if bt is not None:
            orc.bottomtemp(oc, ob, bt)
        yield nt


def run_reference(case, oc, ob, exp_mode):
    """The compiled reference through the case's steps from the same start: one Batch per step."""
    bt = bottom_temp(case, ob) if case.bottom_temp else None
    return orc.ref_step(oc, ob, [forcing(case, nt) for nt in range(1, case.nsteps + 1)], exp_mode=exp_mode,
                        run_physics=land(case), bottom_temp=bt, vary_bottom_temp=case.bottom_temp)


CORE = ["T", "hmix", "kmix"]


def record(case, steps):
    """(digests, values) of one case's reference outputs (steps: list of Batch): digests[step - 1, i] is the SHA-256
    of STEP_FIELDS[i] after that step over the active columns; values[field] holds T, hmix, kmix of the last step in
    full (case.full), for the diagnosis of a mismatch"""
    act = active_columns(case)
    digests = np.array([[digest(np.asarray(field_of(r, name, case.nz))[act]) for name in STEP_FIELDS] for r in steps])
    values = {}
    if case.full:
        values = {name: canonical(np.asarray(field_of(steps[-1], name, case.nz))[act]) for name in CORE}
    return digests, values


def mismatches(case, digests, values, step, get):
    """{field: what differs} between a state after model step `step` (get(field) -> its array over the range
    `field_of` takes) and one build's record of the case (digests: [nsteps, len(STEP_FIELDS), 32] as `record` makes
    them; values: {field: array} of the last step, or {}), over the active columns (the record leaves out land
    columns, which the reference and the HIP path never step and the oracle does)."""
    act = active_columns(case)
    bad = {}
    for i, name in enumerate(STEP_FIELDS):
        v = np.asarray(get(name))[act]
        if not np.array_equal(digest(v), digests[step - 1, i]):
            if step == case.nsteps and name in values:
                bad[name] = f"{int((canonical(v).view(np.int64) != values[name].view(np.int64)).sum())} values"
            else:
                bad[name] = "digest"
    return bad


def hip_get(k3, nz):
    """get(field) for `mismatches` on a HIP Kpp3dFields"""
    def get(name):
        if name in ("hmixd0", "hmixd1"):
            return k3.hmixd[:, int(name[-1])]
        if name in cm.SCALAR_FIELDS or name in cm.EXT_SCALARS:
            return getattr(k3, name)
        return cm.hip_field(k3, name, nz)[0]
    return get


def run_hip(mk, tag, golden, solver_mode=0):
    """The HIP kernel through the case from the same start, through the C-ABI as the parity tests drive it; returns
    [(step, Kpp3dFields copy of the fields, plus the status words and pass counts)] after asserting that its starting state is the oracle's and that the
    oracle's is the recorded one."""
    case = CASES[tag]
    oc, ob, pre, post = oracle_start(case, exp_mode=1, solver_mode=solver_mode)
    assert np.array_equal(input_digest(ob), golden.input_sha(tag, "pexp")), \
        f"the starting state of {tag} is not the recorded one"
    kc, k3 = cm.make_hip_case(case.ncol, case.nz, grid=case.grid, dto=case.dto, land_every=case.land_every)
    for k, v in case.switches.items():
        setattr(kc, k, v)
    apply_hip(k3, pre)
    ctx = mk.mckpp_initialize_ocean_model(k3, kc)
    ctx.set_solver_mode(solver_mode)
    apply_hip(k3, post)
    ctx.upload(k3)
    act = active_columns(case)
    init = cm.compare(k3, ob, case.nz, STEP_FIELDS, act)
    assert not {k: v for k, v in init.items() if v[2]}, f"HIP starting state differs from the oracle's: {init}"
    if case.bottom_temp:
        kc.L_VARY_BOTTOM_TEMP = 1
        k3.bottom_temp[:] = bottom_temp(case, ob)
    out = []
    for nt in range(1, case.nsteps + 1):
        cm.set_forcing_3d(k3, forcing(case, nt))
        ctx = mk.mckpp_physics_driver(k3, kc, nt)
        got = {n: np.array(hip_get(k3, case.nz)(n)) for n in STEP_FIELDS}
        got["status"], _, got["npasses"] = (np.array(a) for a in ctx.status())
        out.append((nt, got))
    return out


class Golden:
    """tests/golden/ref_step.npz: per case and build ("libm", "pexp") the digest of the starting state and of every
    field after every step, and for the portable-exp build T, hmix, kmix of the last step"""

    def __init__(self):
        import os

        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_step.npz")
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        assert list(self.z["fields"]) == STEP_FIELDS, "tests/golden/ref_step.npz records another field list"

    def cases(self):
        return sorted({k.split("/")[0] for k in self.z if "/" in k})

    def input_sha(self, tag, build):
        return self.z[f"{tag}/{build}/input_sha"]

    def digests(self, tag, build):
        return self.z[f"{tag}/{build}/sha"]

    def values(self, tag):
        p = f"{tag}/pexp/val/"
        return {k[len(p):]: v for k, v in self.z.items() if k.startswith(p)}
