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


# ---------------------------------------------------------------------------------------------------------------
# the edge cases: inputs that put a comparison of the step AT equality (tools/oracle_boundaries.py,
# profiles/coverage/oracle_boundaries.md).  The columns of a case come in triples (below, at, above): three columns
# alike in every input - profiles, Coriolis parameter, forcing - but the one that controls the comparison, which the
# middle column has at the compared value and the outer two one np.nextafter to either side of it (where one ulp of
# the input is lost before it reaches the comparison, the smallest step that is not; said at the hook).  Plain columns
# stand beside them.  EDGE_TRIPLES[tag] lists the triples of a case; a lost equality makes two columns of one alike.
# ---------------------------------------------------------------------------------------------------------------
def _state(ob, nzp1):
    """{T, S, U, V, f} of a batch before init_ocean, for the edge hooks to edit in place"""
    T, S, U, V = _profiles(ob, nzp1)
    return {"T": T, "S": S, "U": U, "V": V, "f": ob["f"].copy()}


def triples(first, n):
    return [(first + 3 * j, first + 3 * j + 1, first + 3 * j + 2) for j in range(n)]


def _alike(d, trio):
    """the outer columns of a triple take the middle one's inputs"""
    lo, eq, hi = trio
    for v in d.values():
        v[lo] = v[eq]
        v[hi] = v[eq]


def _around(x):
    return np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)


def _dd_edges(d, first, k):
    """Three triples from column `first`, LDD: salinity bit-equal at the levels k+1 and k+2 (Fortran), betaDS = 0
    there, with temperature falling with depth across them (alphaDT > 0: ddmix's `betaDS > 0.` of the salt-finger arm,
    ddmix_mod.F90:32) and rising by half a kelvin (alphaDT < 0: `betaDS < 0.0` of the diffusive-convection arm, :40);
    the outer columns have S(k+2) one ulp either side.  The third triple has T and S both bit-equal at the two levels:
    dbloc = 0 and Rig = 0 exactly, z121's `V < vlo` with vlo = 0 (z121_mod.F90:28); one ulp of T does not move
    sigma0, so its outer columns have T(k+2) 64 ulps either side."""
    out = triples(first, 3)
    for j, trio in enumerate(out):
        _alike(d, trio)
        T, S = d["T"], d["S"]
        if j == 1:
            for c in trio:
                T[c, k + 1:] += 0.5
        if j < 2:
            for c, s in zip(trio, _around(S[trio[1], k])):
                S[c, k + 1] = s
        else:
            t = T[trio[1], k]
            for c, n in zip(trio, (-64, 0, 64)):
                S[c, k + 1] = S[c, k]
                T[c, k + 1] = t + n * np.spacing(t)
    return out


RELAX_EDGE = 1.e-10      # ocnint's `relax_sst .gt. 1.e-10` (ocnint_mod.F90:98)


def _relax_edges(d, ob, first, ncol):
    """Two triples from column `first`, L_RELAX_SST: relax_sst at 1.e-10 and one ulp either side; 1/(5 days) on the
    other columns, none on every fourth"""
    r = np.full(ncol, 1.0 / (5 * 86400.0))
    r[::4] = 0.0
    out = triples(first, 2)
    for trio in out:
        _alike(d, trio)
        r[list(trio)] = _around(RELAX_EDGE)
    d["relax_sst"] = r
    d["SST0"] = d["T"][:, 0] + 1.5
    return out


def _ldd_equal(ncol, nzp1, ob):
    d = _state(ob, nzp1)
    _dd_edges(d, 3, nzp1 // 3)
    return d


def _relax_edge(ncol, nzp1, ob):
    d = _state(ob, nzp1)
    _relax_edges(d, ob, 3, ncol)
    return d


def _some_bathymetry(ncol, nzp1, ob):
    """a sea floor between 3 and 40 m under every third column: hbl is -ocdepth pass after pass, hmixn == hmixe"""
    return {"ocdepth": bathymetry(ncol, 3.0, 40.0, every=3)}


ZERO_FLUX_STEP = 1e-300    # W/m2: one ulp from zero is a subnormal that the division by rho cp flushes to zero


def _zero_flux_columns(ncol, nzp1, ob):
    """Two triples from column 3, alike in all but the non-solar heat flux (_zero_flux): the second is a column of
    -1.8 degC and one salinity at every level (L_NO_FREEZE's `X < -1.8`, overrides.F90:87; with L_NO_ISOTHERM and
    iso_thresh = 0, `ABS(dtdz_total) < iso_thresh` at 0, :112)"""
    d = _state(ob, nzp1)
    d["ocdepth"] = np.full(ncol, -10000.0)
    for j, trio in enumerate(triples(3, 5)):
        eq = trio[1]
        if j == 1:
            d["T"][eq, :], d["S"][eq, :] = -1.8, 0.0
        if j >= 2:
            d["T"][eq, :], d["S"][eq, :], d["f"][eq] = 15.0, 0.0, EKMAN_F
        _alike(d, trio)
        if j == 2:
            d["ocdepth"][list(trio)] = [-x for x in _around(7.5)]
        if j == 3:
            d["ocdepth"][list(trio)] = -7.0
            d["f"][list(trio)] = _around(EKMAN_F_EDGE)
    d["ocnT_clim"] = 5.0 + 0 * d["T"]
    d["sal_clim"] = 0.1 + 0 * d["S"]
    return d


# Coriolis parameters of the Ekman triples (60 N; 1 / s) and the wind stress over them (N/m2): hekman = 0.7 ustar / (|f| +
# 1e-16) is 1.7 m at EKMAN_F and, bit for bit, 2.5 m - the centre of level 1 of the 40-level grid - at EKMAN_F_EDGE
EKMAN_F = float(cm.synth.coriolis(60.0))
EKMAN_F_EDGE = 8.740752130227744e-05
EKMAN_STRESS = 1e-4
# wind stress and heating (W/m2) under which the Monin-Obukhov depth ustar^3 / vonk / (bfsfc + 1e-16) over the uniform
# water of those triples is 7.5 m, the centre of level 2, bit for bit
MONOB_STRESS, MONOB_HEAT = 0.02, 55.73046706341893


def _zero_flux(sf):
    """No solar, no heat, no ice melt, no fresh water on the middle columns: the surface buoyancy flux is exactly zero
    (wscale's `zehat <= zmax` at zehat = 0, wscale_mod.F90:63; bfsfc = 0 in bldepth, blmix and `stable`); -1e-300 and
    +1e-300 W/m2 of heat on the outer ones of the first two triples, under a stress of 0.3 N/m2 on the first (the
    boundary layer ends where the bulk Richardson number says, which the velocity scales enter).
    The third and fourth triples have no buoyancy flux on any column and a light wind over uniform water: the Ekman
    depth, 1.7 m, is the shallowest limit and lies above the centre of level 1, so bldepth takes its second minimum,
    without the Ekman depth (bldepth_mod.F90:173-180).  Third: that minimum is the sea floor at 7.5 m, the centre of
    level 2 (`hmin2 < -zm(kl)` at equality), 7.5 m -+ one ulp on the outer columns.  Fourth: the Coriolis parameter
    puts the Ekman depth itself at 2.5 m, the centre of level 1 (`hmin < -zm(kl-1)` at equality), over a sea floor at
    7 m; f one ulp either side on the outer columns.  The fifth is heated under a wind of 0.02 N/m2: the Monin-Obukhov
    depth is 7.5 m (`dmo(ku) <= -zm(kl)` at equality, bldepth_mod.F90:148), the heating one ulp either side."""
    for j, trio in enumerate(triples(3, 5)):
        for c, q in zip(trio, (-ZERO_FLUX_STEP, 0.0, ZERO_FLUX_STEP)):
            sf[c] = sf[trio[1]]
            sf[c, 2:6] = 0.0
            if j < 2:
                sf[c, 3] = q
            if j == 0:
                sf[c, 0] = 0.3
            if j >= 2:
                sf[c, 0:2] = EKMAN_STRESS, 0.0
        if j == 4:
            sf[list(trio), 0] = MONOB_STRESS
            sf[list(trio), 3] = _around(MONOB_HEAT)


def _mixed_edges(ncol, nzp1, ob):
    """the double-diffusion and the relaxation triples side by side, over some bathymetry (the 60- and 69-level
    cases: the kernels with the level count as a literal, workgroups of more than one slot)"""
    d = _state(ob, nzp1)
    _dd_edges(d, 3, nzp1 // 3)
    _relax_edges(d, ob, 12, ncol)
    floor = np.arange(18, ncol, 3)
    d["ocdepth"] = np.full(ncol, -10000.0)
    d["ocdepth"][floor] = -np.linspace(3.0, 40.0, len(floor))
    return d


def _retry_columns(ncol, nzp1, ob):
    """every column the same closed form at 30 S, moving at 2 m/s in U and V (as _moving): the wind stress alone
    decides how many tries of ocnstep's trap a column takes"""
    k = np.arange(nzp1)[None, :] + np.zeros((ncol, 1))
    return {"T": 20.0 - 0.01 * k, "S": 0.001 * k, "U": 2.0 + 0 * k, "V": 2.0 + 0 * k,
            "f": np.full(ncol, float(cm.synth.coriolis(-30.0)))}


# Values at which a quantity at the end of a rounding chain meets its threshold bit for bit, each found by bisecting
# the oracle on the input named, over a few hundred second inputs an ulp apart, until one of them landed on equality.
# tests/test_boundaries_cpu.py fails when generator drift takes a column off its equality.
EXACT_K = 13                                   # the levels EXACT_K + 1 and EXACT_K + 2 (Fortran)
EXACT_FINGER = (198, 0.0034566584223760426)    # T(k) raised by 198 ulps; S(k) - S(k+1): alphaDT == betaDS > 0
EXACT_DIFFCONV = (39, 0.0034885944406148387)   # likewise, S(k+1) - S(k): alphaDT == betaDS < 0
EXACT_RIG = (222, 0.014424298321962993)        # U(k) - U(k+1): Rig == Riinfty = 0.8
EXACT_RMS = (9, 4.6370233105856125)            # T raised by 9e-3 K; taux: the rms change of U over a step == 1 m/s
EXACT_U10 = 9.999693559642605                  # U at every level: U(1) == 10 m/s after a step under 1e-4 N/m2
EXACT_V10 = 9.999999999999998                  # V at every level: V(k) == 10 m/s after a step
EXACT_T10 = 10.0187298883641                   # a temperature step at 40 m: T(8) - T(9) == 10 K after a step


def _exact_edges(ncol, nzp1, ob):
    """Three triples from column 3 on the closed-form columns of _retry_columns, LDD: ddmix's `alphaDT > betaDS`
    (ddmix_mod.F90:32) and `alphaDT < betaDS` (:41) with both sides equal, and rimix's Rig equal to Riinfty, z121's
    `V > vhi` (z121_mod.F90:28), among levels whose Rig is near 0.25.  The outer columns have S(k+1) (U(k+1)) one ulp
    either side."""
    d = _retry_columns(ncol, nzp1, ob)
    K = EXACT_K
    k = np.arange(nzp1)
    ulp = np.spacing(20.0)
    for j, (lo, eq, hi) in enumerate(triples(3, 3)):
        trio = [lo, eq, hi]
        n, p = (EXACT_FINGER, EXACT_DIFFCONV, EXACT_RIG)[j]
        sgn = -1.0 if j == 1 else 1.0
        if j < 2:
            d["S"][trio] = -sgn * d["S"][trio]
            d["T"][trio] = 20.0 + sgn * (d["T"][trio] - 20.0)
        else:
            d["U"][trio] = np.where(k == K, 0.5 - 0.01 * K, (0.5 - 0.01 * K) - 0.025 * (k - K))
            d["V"][trio] = 0.0
        d["T"][trio, K] = d["T"][trio, K] + np.arange(512)[n] * ulp
        name = "S" if j < 2 else "U"
        d[name][trio, K + 1] = _around(d[name][eq, K] - sgn * p)
    return d


def _trap_uv_columns(ncol, nzp1, ob):
    """Two triples from column 3: no Coriolis term, no buoyancy flux, 1e-4 N/m2 of wind over a uniform current of
    EXACT_U10 in U (the second: EXACT_V10 in V), 0.25 m/s in the other component: after the step the largest |U|
    (|V|) of the column is 10 m/s bit for bit, the trap's `>= 10` at equality (ocnstep_mod.F90:202); the current one
    ulp either side on the outer columns.  f = 0 is an input the reference's step takes like any other; its own
    geography never yields it (the Coriolis parameter is that of 2.5 degrees inside 2.5 degrees of the equator)."""
    d = _retry_columns(ncol, nzp1, ob)
    for j, trio in enumerate(triples(3, 2)):
        for c, q in zip(trio, _around((EXACT_U10, EXACT_V10)[j])):
            d["f"][c] = 0.0
            d["U" if j == 0 else "V"][c] = q
            d["V" if j == 0 else "U"][c] = 0.25
    return d


def _trap_t_columns(ncol, nzp1, ob):
    """One triple from column 3: likewise at rest, a temperature step of EXACT_T10 down between levels 8 and 9: after
    the step T(8) - T(9) is 10 K bit for bit (ocnstep_mod.F90:203)"""
    d = _retry_columns(ncol, nzp1, ob)
    for c, q in zip((3, 4, 5), _around(EXACT_T10)):
        d["f"][c] = 0.0
        d["U"][c], d["V"][c] = 0.0, 0.0
        d["T"][c, 8:] -= q
    # and a column at rest but for 15 m/s at level NZ and below it: the deepest level the trap looks at is the only
    # one past 10 m/s after the step (the bound of its loop, ocnstep_mod.F90:201)
    d["f"][8], d["U"][8], d["V"][8] = 0.0, 0.0, 0.0
    d["U"][8, nzp1 - 2:] = 15.0
    return d


def _light_wind(first, n):
    def stress(ncol):
        taux = np.full(ncol, 0.01)
        taux[first:first + 3 * n] = 1e-4
        return taux, np.zeros(ncol)
    return stress


def _no_buoyancy(sf):
    """no solar, no heat, no ice melt, no fresh water: the wind alone works on the column"""
    sf[:, 2:6] = 0.0


RETRY_ON_THE_BOUND, RETRY_PAST_THE_BOUND = 20, 22


def _retry_stress(ncol):
    """4.60, 4.61, ... N/m2 eastward: on the 10 m grid at 30 S the rms change of U is 1 m/s near 4.64 N/m2, and every
    retry's f * 1.01 takes the Coriolis term further against the stress: each 0.02 N/m2 more costs one more try.
    Column 20 (4.80) is accepted on its 10th try, reset_flag = comp_iter_max (`reset_flag > comp_iter_max` at
    equality, ocnstep_mod.F90:229); column 22 (4.82) is still trapped on its 11th and fails, one past it."""
    return 4.6 + 0.01 * np.arange(ncol), np.zeros(ncol)


def _retry_and_rms_columns(ncol, nzp1, ob):
    """_retry_columns; the columns 0, 1, 2 a little warmer: the triple of the rms threshold (_rms_edge)"""
    d = _retry_columns(ncol, nzp1, ob)
    d["T"][0:3] = d["T"][0:3] + 1e-3 * EXACT_RMS[0]
    return d


def _rms_edge(sf):
    """columns 0, 1, 2 under column 0's heat and fresh water and a stress of EXACT_RMS[1] and one ulp either side: the
    rms change of U over the step is 1 m/s bit for bit on column 1 (`rmsd >= rmsd_threshold`, ocnstep_mod.F90:222)"""
    for c, q in zip((0, 1, 2), _around(EXACT_RMS[1])):
        sf[c] = sf[0]
        sf[c, 0] = q


def _alike_forcing(first, n):
    def hook(sf):
        for lo, eq, hi in triples(first, n):
            sf[lo] = sf[eq]
            sf[hi] = sf[eq]
    return hook


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
    # the edge cases: comparisons AT equality, the two neighbours beside them (EDGE_TRIPLES) ...
    "edge_ldd_equal_nz40": Case(24, 40, 2, switches=dict(LDD=1), pre=_ldd_equal, surface=_alike_forcing(3, 3)),
    "edge_relax_sst_nz40": Case(24, 40, 2, switches=dict(L_RELAX_SST=1), pre=_relax_edge, surface=_alike_forcing(3, 2)),
    "edge_zero_flux_nz40": Case(24, 40, 3, switches=dict(L_NO_FREEZE=1, L_NO_ISOTHERM=1, iso_thresh=0.0),
                                pre=_zero_flux_columns, surface=_zero_flux),
    # ... the integer counters of ocnstep: with itermax = 3 a column that does not deepen leaves the iteration at
    # iter = itermax + 1 (`iter > itermax + 1` at equality), one that deepens once leaves one past it; over a sea
    # floor hmixn == hmixe (`hmixn > hmixe`), and with hmixtolfrac = 0 that is `|hmixn - hmixe| > tol` at 0 = 0 ...
    "edge_itermax3_nz40": Case(30, 40, 4, switches=dict(itermax=3), pre=_some_bathymetry, diurnal=True),
    "edge_tol0_seafloor_nz40": Case(30, 40, 2, switches=dict(hmixtolfrac=0.0, itermax=8), pre=_some_bathymetry),
    "edge_retry_count_thin": Case(24, 12, 2, grid="thin", pre=_retry_and_rms_columns, stress=_retry_stress,
                                  surface=_rms_edge),
    # ... quantities at the end of a rounding chain, met bit for bit (EXACT_*): alphaDT == betaDS of either sign and
    # Rig == Riinfty; the trap's 10 m/s in U and in V, and its 10 K between two levels ...
    "edge_exact_dd_rig_nz40": Case(24, 40, 2, switches=dict(LDD=1), pre=_exact_edges, surface=_alike_forcing(3, 3)),
    "edge_trap_uv_thin": Case(24, 12, 2, grid="thin", pre=_trap_uv_columns, stress=_light_wind(3, 2),
                              surface=_no_buoyancy),
    "edge_trap_tjump_nz40": Case(12, 40, 2, pre=_trap_t_columns, stress=_light_wind(3, 1), surface=_no_buoyancy),
    # ... and several of them side by side at the depths that have kernels with the level count as a literal
    "edge_mixed_nz60": Case(48, 60, 3, switches=dict(LDD=1, L_RELAX_SST=1, itermax=3), pre=_mixed_edges,
                            surface=_alike_forcing(3, 5), jerlov_mix=False),
    "edge_mixed_nz69_stretched": Case(48, 69, 3, grid="stretched", dto=1200.0, pre=_mixed_edges,
                                      switches=dict(LDD=1, L_RELAX_SST=1, itermax=3), surface=_alike_forcing(3, 5)),
}


REGIME_CASES = [t for t in CASES if t.startswith(("seafloor_", "fulldepth_", "tjump_", "rms_retry_", "ssref0_",
                                                  "ldd_diffconv_", "regime_sweep_"))]
ADVECTION_CASES = [t for t in CASES if t.startswith("adv_")]
PRECEDENCE_CASES = [t for t in CASES if t.startswith("prec_")]
EDGE_CASES = [t for t in CASES if t.startswith("edge_")]
# (below, at, above) columns of each edge case; the cases of the integer counters have none
EDGE_TRIPLES = {
    "edge_ldd_equal_nz40": triples(3, 3),
    "edge_relax_sst_nz40": triples(3, 2),
    "edge_zero_flux_nz40": triples(3, 5),
    "edge_itermax3_nz40": [],
    "edge_tol0_seafloor_nz40": [],
    "edge_retry_count_thin": triples(0, 1),
    "edge_exact_dd_rig_nz40": triples(3, 3),
    "edge_trap_uv_thin": triples(3, 2),
    "edge_trap_tjump_nz40": triples(3, 1),
    "edge_mixed_nz60": triples(3, 5),
    "edge_mixed_nz69_stretched": triples(3, 5),
}


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
