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
    surface: Optional[Callable] = None      # (sflux rows [ncol, 6]) -> None: edits the assembled forcing in place
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


# ---------------------------------------------------------------------------------------------------------------
# prescribed advection of salinity (rhsmod, src/mckpp_physics_solvers.F90:176-335; ocnint applies it whenever
# nmodeadv(2) > 0, src/mckpp_physics_ocnint_mod.F90:179) and the switch pairs of ocnint of which one member is
# silently ignored.  Closed forms of the column index, like the regimes.
#
# What the reference's declarations allow (src/mckpp_data_fields.F90:494-496: zm(nzp1), hm(nzp1), dm(0:nz); ocnint's
# rhs(NZtmax) with NZtmax = nz + 1), and what the cases therefore may hold:
#   km = kmixe comes from bldepth, which leaves kbl in 2 .. km = NZ (bldepth_mod.F90:101, :105, :183; kppmix hands it
#   km = NZ).  So km = 1 cannot occur (no hm(0), no n1 = 0 in mode 7), and a mixed layer over the full depth is
#   km = NZ: dm(NZ), hm(NZ), hm(NZ-1) are all inside.  ocnstep's `kmixn == NZP1` (ocnstep_mod.F90:158) can never be
#   true for the same reason: no input reaches it, and no case is named after it.
#   Modes 6 and 7 read hm(n+1) for n <= nzi = NZ: hm(nzp1), inside.  Mode 6 always meets dmax = dm(km) - (hm(km) +
#   hm(km-1))/2 by n = km - 1 < nzi, its depth then being dm(km); it cannot run to nzi with km <= NZ.  Mode 7 runs
#   to nzi on a grid shallower than 100 m, inside the arrays.
#   Mode 4 looks for the first zm(n1) < -100 without a bound: on a grid with no level below 100 m (zm(nzp1) >= -100)
#   it reads past zm(nzp1).  No recorded column has mode 4 on such a grid (adv_edges_90m leaves it out); the column
#   kernel and the oracle stop the search at nzp1 and are compared there on the device alone.
#   A mode above 7 aborts the reference (solvers.F90:320-323): none is recorded, the upload refuses it.
# ---------------------------------------------------------------------------------------------------------------
ADV0 = 2e-5     # PSU m/s; a step's change of S is dto * A * 0.033 / (the depth it is spread over)


def advection_inputs(ncol, slots, index1=False):
    """{nmodeadv, modeadv, advection} of a batch - (ncol, 2), (ncol, 2, 6), (ncol, 2, 6), [:, 1] being the
    reference's index 2 (salinity), the only one it reads.  slots(c) -> (the modes of column c's slots, how many of
    them nmodeadv(c,2) declares live); every slot given gets a magnitude of either sign, 1 ... 5 times ADV0, the dead
    ones included.  index1: index 1 (temperature), which the reference never reads, holds live-looking values too."""
    nm = np.zeros((ncol, 2), dtype=np.int32)
    mode = np.zeros((ncol, 2, 6), dtype=np.int32)
    adv = np.zeros((ncol, 2, 6))
    for c in range(ncol):
        modes, live = slots(c)
        nm[c, 1] = live
        for j, m in enumerate(modes):
            mode[c, 1, j] = m
            adv[c, 1, j] = ADV0 * (1 + (c + j) % 5) * (1 if (c + j) % 2 == 0 else -1)
        if index1:
            nm[c, 0] = 1 + c % 6
            mode[c, 0, :] = 1 + (c + np.arange(6)) % 7
            adv[c, 0, :] = 40.0 * (1 + np.arange(6)) * (1 if c % 2 else -1)
    return {"nmodeadv": nm, "modeadv": mode, "advection": adv}


def _adv_one_mode(ncol, nzp1, ob):
    return advection_inputs(ncol, lambda c: ((1 + c % 7,), 1))


# (modes of the slots, nmodeadv(2)): all six slots; a mode twice; a zero and a negative mode between live ones (the
# reference returns at mode <= 0 and goes on with the next slot); nothing live with modes and magnitudes behind it;
# the three modes whose range follows the mixed layer, twice; two live with more behind them; all six with holes
ADV_PATTERNS = (((1, 2, 3, 4, 5, 6), 6), ((7, 7, 2), 3), ((6, 0, 3, -2, 7), 5), ((4, 5, 1), 0),
                ((2, 6, 7, 2, 6, 7), 6), ((5, 3, 7, 1), 2), ((3, -1, 0, 5, 2, 4), 6))


def _adv_patterns(ncol, nzp1, ob):
    return advection_inputs(ncol, lambda c: ADV_PATTERNS[c % 7])


def _adv_patterns_index1(ncol, nzp1, ob):
    return advection_inputs(ncol, lambda c: ADV_PATTERNS[c % 7], index1=True)


def _adv_patterns_scorr(ncol, nzp1, ob):
    """the advection term and sinc_fcorr (L_SFCORR_WITHZ, L_RELAX_SAL) in one right-hand side"""
    d = _adv_patterns(ncol, nzp1, ob)
    z = np.arange(nzp1)[None, :]
    d["sfcorr_withz"] = 1e-7 * np.cos(z / 7.0) * np.linspace(-1, 1, ncol)[:, None]
    d["sal_clim"] = ob["S"][:, 1:nzp1 + 1] + 0.05
    d["relax_sal"] = np.full(ncol, 1.0 / (15 * 86400.0))
    return d


def _cooling(sf):
    """every column loses 400 W/m2 in the dark: with `isothermal` it convects as deep as its sea floor lets it"""
    sf[:, 2] = 0.0
    sf[:, 3] = -400.0
    sf[:, 5] = 6e-5 - 400.0 / cm.synth.EL


# -ocdepth of the edge columns on the 40-level grid (5 m levels, centres at 2.5, 7.5, ...): the sea floor makes
# km = kmix the first level whose centre lies below it - 2, 3, 13, 20 (centre 97.5 m), 21 (102.5), 22, 31 - and the
# last lets the column mix down to km = NZ
ADV_EDGE_FLOORS = (2.0, 9.0, 60.0, 93.0, 100.0, 103.0, 150.0, 10000.0)
ADV_EDGE_MODES = ((2,), (6,), (7,), (2, 6, 7))


def _adv_edges(ncol, nzp1, ob):
    """Eight mixed-layer depths times the modes whose range follows km - 2, 6, 7 alone and together - on convecting
    isothermal columns: km = 2 (mode 2 over one level, mode 7 from level 1, mode 6 meeting dmax on its first level);
    km = 20 and 21, 22 (just above and below 100 m: mode 7's first `depth >= dmax` is true at once) against km = 3
    and 13 (true only after many levels); km = 31 and NZ (mode 6 meeting dmax deep)."""
    d = _isothermal(ncol, nzp1, ob)
    d["ocdepth"] = -np.resize(np.array(ADV_EDGE_FLOORS), ncol)
    def slots(c):
        modes = ADV_EDGE_MODES[(c // len(ADV_EDGE_FLOORS)) % len(ADV_EDGE_MODES)]
        return modes, len(modes)
    d.update(advection_inputs(ncol, slots))
    return d


def _adv_small_grid(modes):
    def hook(ncol, nzp1, ob):
        return advection_inputs(ncol, lambda c: ((modes[c % len(modes)], modes[(c + 3) % len(modes)]), 2))
    return hook


def _both(*hooks):
    def hook(ncol, nzp1, ob):
        d = {}
        for h in hooks:
            d.update(h(ncol, nzp1, ob))
        return d
    return hook


def _trap_v(ncol, nzp1, ob):
    """20 m/s northward in the four top levels of every fourth column, U as the generators leave it (5 cm/s)"""
    V = ob["V"][:, 1:nzp1 + 1].copy()
    V[::4, 0:4] = 20.0
    return {"V": V}


def _trap_v_clim(ncol, nzp1, ob):
    d = _trap_v(ncol, nzp1, ob)
    d["ocnT_clim"] = ob["T"][:, 1:nzp1 + 1] - 0.25
    d["sal_clim"] = ob["S"][:, 1:nzp1 + 1] + 0.01
    return d


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
    # prescribed advection: one mode a column over a widely spread mixed layer ...
    "adv_modes_nz40": Case(49, 40, 3, switches=dict(L_ADVECT=1), pre=_adv_one_mode, stress=_stress_ramp),
    # ... several slots a column at the depths that have kernels with the level count as a literal; its twin with
    # live-looking values at index 1 (temperature), which the reference never reads ...
    "adv_modes_nz60": Case(56, 60, 3, switches=dict(L_ADVECT=1), pre=_adv_patterns, land_every=4, jerlov_mix=True,
                           stress=_stress_ramp),
    "adv_modes_nz60_index1": Case(56, 60, 3, switches=dict(L_ADVECT=1), pre=_adv_patterns_index1, land_every=4,
                                  jerlov_mix=True, stress=_stress_ramp),
    "adv_modes_nz69_stretched": Case(56, 69, 4, grid="stretched", dto=1200.0, pre=_adv_patterns_scorr, land_every=5,
                                     jerlov_mix=True, stress=_stress_ramp,
                                     switches=dict(L_ADVECT=1, L_SFCORR_WITHZ=1, L_RELAX_SAL=1)),
    # ... the edges of the level ranges: the mixed layer at chosen levels of the 40-level grid; 12-level grids whose
    # first level below 100 m is NZ-1 (mode 4 over one level: 120 m), NZ (105 m) and NZP1 (102 m: both empty, n1 >
    # nzend) ...
    "adv_edges_nz40": Case(32, 40, 3, switches=dict(L_ADVECT=1), pre=_adv_edges, surface=_cooling),
    "adv_edges_120m": Case(14, 12, 2, grid="uniform_120", switches=dict(L_ADVECT=1), pre=_adv_small_grid(range(1, 8))),
    "adv_edges_105m": Case(14, 12, 2, grid="uniform_105", switches=dict(L_ADVECT=1), pre=_adv_small_grid(range(1, 8))),
    "adv_edges_102m": Case(14, 12, 2, grid="uniform_102", switches=dict(L_ADVECT=1), pre=_adv_small_grid(range(1, 8))),
    # ... a grid of 8 m levels, all of its arithmetic exact: the centre of level 13 lies AT 100 m (mode 4's `zm >= -100`
    # goes on to level 14) and mode 7's running depth comes to 100 m exactly (`depth >= dmax` stops there) ...
    "adv_edges_128m": Case(14, 16, 2, grid="uniform_128", switches=dict(L_ADVECT=1), pre=_adv_small_grid(range(1, 8))),
    # ... and a 90 m grid, where mode 7 runs to nzi without meeting 100 m (no mode 4 there: see above)
    "adv_edges_90m": Case(18, 12, 2, grid="uniform_90", switches=dict(L_ADVECT=1),
                          pre=_adv_small_grid((1, 2, 3, 5, 6, 7))),
    # the switch pairs of ocnint of which one member (or both) is silently ignored, inputs non-zero for both ...
    "prec_relax_sst_fcorr_withz": Case(24, 40, 2, switches=dict(L_RELAX_SST=1, L_FCORR_WITHZ=1),
                                       pre=_both(_relax_sst, _fcorr_withz)),
    "prec_relax_sst_fcorr": Case(24, 40, 2, switches=dict(L_RELAX_SST=1, L_FCORR=1), pre=_both(_relax_sst, _fcorr_twod)),
    "prec_fcorr_fcorr_withz": Case(24, 40, 2, switches=dict(L_FCORR=1, L_FCORR_WITHZ=1),
                                   pre=_both(_fcorr_twod, _fcorr_withz)),
    "prec_sfcorr_sfcorr_withz": Case(24, 40, 2, switches=dict(L_SFCORR=1, L_SFCORR_WITHZ=1), pre=_fcorr_withz),
    "prec_relax_sst_fcorr_withz_relax_ocnt": Case(24, 40, 2, pre=_both(_relax_sst, _fcorr_withz, _relax_ocnt_sal),
                                                  switches=dict(L_RELAX_SST=1, L_FCORR_WITHZ=1, L_RELAX_OCNT=1)),
    # ... and the V half of the instability trap
    "trap_v_nz40": Case(24, 40, 2, post=_trap_v),
    "trap_v_clim_nz40": Case(24, 40, 2, switches=dict(clim_present=1), post=_trap_v_clim),
}


REGIME_CASES = [t for t in CASES if t.startswith(("seafloor_", "fulldepth_", "tjump_", "rms_retry_", "ssref0_",
                                                  "ldd_diffconv_", "regime_sweep_"))]
ADVECTION_CASES = [t for t in CASES if t.startswith("adv_")]
PRECEDENCE_CASES = [t for t in CASES if t.startswith("prec_")]


def _apply_batch(ob, nzp1, d):
    for k, v in d.items():
        if k in orc.LEVEL_FIELDS:
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
        elif k in ("modeadv", "advection"):     # the batch's (ncol, 2, 6) on the reference's (npts, maxmodeadv, 2)
            getattr(k3, k)[...] = np.asarray(v).transpose(0, 2, 1)
        else:
            getattr(k3, k)[...] = v


def forcing(case, step):
    """sflux(1:6) of model step `step` (1-based)"""
    t = step * case.dto if case.diurnal else None
    sf = cm.synth.forcing(case.ncol, "bench", t_seconds=t)
    if case.stress:
        sf[:, 0], sf[:, 1] = case.stress(case.ncol)
    if case.surface:
        case.surface(sf)
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


def start_hip(mk, tag, golden, solver_mode=0):
    """The HIP side of a case at its start, through the C-ABI as the parity tests drive it: (KppConstFields,
    Kpp3dFields, context, the oracle's Const and Batch at the same start), after asserting that the oracle's starting
    state is the recorded one and that the HIP one is the oracle's."""
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
    return kc, k3, ctx, oc, ob


def hip_fields(k3, ctx, nz):
    """{field: array} of STEP_FIELDS as `mismatches` takes them, plus the status words and pass counts"""
    got = {n: np.array(hip_get(k3, nz)(n)) for n in STEP_FIELDS}
    got["status"], _, got["npasses"] = (np.array(a) for a in ctx.status())
    return got


def run_hip(mk, tag, golden, solver_mode=0):
    """The HIP kernel through the case from the same start, a launch per step; returns [(step, {field: array} of
    STEP_FIELDS, plus the status words and pass counts)]."""
    case = CASES[tag]
    kc, k3, ctx, oc, ob = start_hip(mk, tag, golden, solver_mode)
    if case.bottom_temp:
        kc.L_VARY_BOTTOM_TEMP = 1
        k3.bottom_temp[:] = bottom_temp(case, ob)
    out = []
    for nt in range(1, case.nsteps + 1):
        cm.set_forcing_3d(k3, forcing(case, nt))
        ctx = mk.mckpp_physics_driver(k3, kc, nt)
        out.append((nt, hip_fields(k3, ctx, case.nz)))
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
