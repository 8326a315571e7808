"""The column kernel's instantiations through its launch forms: inputs and the matrix, stated once.

k_column_ps<XV, SM, LF> is compiled 18 times (mckpp_kernels_ps.hip, mckpp_launch_column_kernel_ps): XV the physics
variant (0 default, 1 optional physics, 2 optional physics with double diffusion - another row layout of a slot, other
sweeps, a finish round with more in it), SM the solver, LF the number of level items as a literal (63, 72, 103; XV < 2)
or 0.  The launch forms - several steps in a launch, the views, forced geometries, queue adoption, the reference-level
sums both ways, the second bulk-Ri round - reorder who does the work, when, and in which rows.  MATRIX crosses the two:
switch sets that give each XV, on a mix of columns that has stragglers, trapped and clamped columns and something for
every switch to act on, through every form.  tests/test_variants_cpu.py settles on the oracle that the matrix is
complete and the mix reaches what it is for; tests/test_variants_gpu.py runs it on the device against the oracle
stepped one step at a time; profiles/coverage/kernel_variants.md is the record.  No pytest here, nothing touches a GPU."""
import functools
import os
import re
from dataclasses import dataclass, field

import numpy as np

import common as cm
import ref_step_cases as rc
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "mckpp_f90_amd", "csrc", "mckpp_kernels_ps.hip")

# ---------------------------------------------------------------------------------------------------------------
# the switch sets.  Each is live under the precedence of ocnint (src/mckpp_physics_ocnint_mod.F90:97-215):
# L_RELAX_SST counts only without L_FCORR_WITHZ and L_FCORR (:97), L_FCORR_WITHZ only without L_FCORR (:134),
# L_SFCORR_WITHZ only without L_SFCORR (:190).  iso_bot, iso_thresh as tests/test_options_gpu.py sets them.
# ---------------------------------------------------------------------------------------------------------------
_RELAXED = dict(L_RELAX_SST=1, L_RELAX_OCNT=1, L_RELAX_SAL=1, L_DAMP_CURR=1, dt_uvdamp=360, L_NO_FREEZE=1,
                L_NO_ISOTHERM=1, clim_present=1, iso_bot=20, iso_thresh=0.002)
_CORRECTED = dict(L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1, L_ADVECT=1)
SETS = {
    "default": {},
    "relaxed": _RELAXED,
    "corrected": _CORRECTED,
    "relaxed_dd": dict(_RELAXED, LDD=1),
    "corrected_dd": dict(_CORRECTED, LDD=1),
}
PARAMETERS = ("dt_uvdamp", "iso_bot", "iso_thresh")     # values, not switches: "every switch counts" leaves them


def switches_of(name):
    """the on/off switches of a set, without the values that go with them"""
    return [k for k in SETS[name] if k not in PARAMETERS]


# what makes a context take the optional-physics build: mckpp_runtime.cpp, `h->ext_kernel = ...` (clim_present alone
# does not), which `p.ext` hands to the launcher
EXT_KERNEL_SWITCHES = ("LDD", "L_RELAX_SST", "L_FCORR", "L_FCORR_WITHZ", "L_SFCORR", "L_SFCORR_WITHZ", "L_RELAX_SAL",
                       "L_RELAX_OCNT", "L_NO_FREEZE", "L_NO_ISOTHERM", "L_DAMP_CURR", "L_ADVECT")
LITERAL_L = (63, 72, 103)


def instantiation(switches, solver, nz, env):
    """(XV, SM, LF) of the kernel a step of such a context runs, by the launcher's rule - a restatement of
    mckpp_launch_column_kernel_ps (mckpp_kernels_ps.hip): `xv = p.ext ? (p.LDD ? 2 : 1) : 0` with p.ext from
    mckpp_runtime.cpp's ext_kernel; `fixed_l` unless MCKPP_PS_FIXED_L is 0; the literal kernels for xv < 2 and
    L = nzp1 + 2 of 63, 72, 103.  The library does not say which instantiation ran; what it says - kernel_name,
    `k_column_ps<EXT>` exactly when XV > 0 - the GPU module checks against this."""
    ext = any(switches.get(k) for k in EXT_KERNEL_SWITCHES)
    xv = (2 if switches.get("LDD") else 1) if ext else 0
    L = nz + 3
    fixed_l = not ("MCKPP_PS_FIXED_L" in env and int(env["MCKPP_PS_FIXED_L"]) == 0)
    return xv, int(solver), (L if fixed_l and xv < 2 and L in LITERAL_L else 0)


def compiled_instantiations():
    """the (XV, SM, LF) the launcher's tables name: every `k_column_ps<...>` of mckpp_kernels_ps.hip"""
    with open(KERNEL_SOURCE) as f:
        src = f.read()
    out = set()
    for m in re.finditer(r"k_column_ps<\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(\d+)\s*)?>", src):
        out.add((int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the LDS a workgroup of W slots takes: ps_lds_bytes / ps_ss_default / ps_rows of mckpp_kernels_ps.hip restated, the
# enums read from the source.  ps_geometry takes MCKPP_PS=<slots>x<waves>x<workgroups per CU> with at most 21 slots
# and 16 waves; the launcher refuses what is more than 160 KiB.  (The GPU module compares lds_bytes with what
# kernel_residency reports.)
# ---------------------------------------------------------------------------------------------------------------
LDS_LIMIT, MOST_SLOTS, MOST_WAVES = 160 * 1024, 21, 16


@functools.lru_cache(maxsize=None)
def _enums():
    """{name: value} of the enumerators of mckpp_kernels_ps.hip's anonymous enums"""
    with open(KERNEL_SOURCE) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    val = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S):
        nxt = 0
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            name, _, expr = (s.strip() for s in item.partition("="))
            if expr:
                nxt = int(eval(re.sub(r"\(int\)", "", expr), {"__builtins__": {}}, val))   # noqa: S307 (own source)
            val[name] = nxt
            nxt += 1
    return val


def lds_bytes(L, W, xv):
    e = _enums()
    rows = (e["Q_COUNT"], e["Q_COUNT_EXT"], e["Q_COUNT_EXT_DD"])[xv]
    ss = rows * L
    if not ss & 1:
        ss += 1
    while ss & 31 in (1, 31):
        ss += 2
    return (e["K_STRIDE"] * L + 2 + W * ss + W * e["C_COUNT"]) * 8 + (W * e["I_COUNT"] + 32) * 4


def most_slots(nz, xv):
    """the most slots a workgroup of this variant and depth may be forced to"""
    return max(w for w in range(1, MOST_SLOTS + 1) if lds_bytes(nz + 3, w, xv) <= LDS_LIMIT)


def most_slots_geometry(nz, xv):
    """MCKPP_PS for F11: that many slots, a wave per 64 items up to 16, one workgroup a CU"""
    w = most_slots(nz, xv)
    return f"{w}x{min(MOST_WAVES, (w * (nz + 3) + 63) // 64)}x1"


# ---------------------------------------------------------------------------------------------------------------
# the column mix
# ---------------------------------------------------------------------------------------------------------------
MIX = ("plain", "shallow", "isothermal", "tjump", "trap_u", "frozen", "deep_currents", "fingers", "diffconv",
       "reef", "isothermal_seafloor", "shallow_reversed")
DEEP_U, DEEP_V = 3.0, -2.5


def regime_columns(ncol):
    """regime name -> its columns: column index modulo len(MIX)"""
    i = np.arange(ncol)
    return {name: np.nonzero(i % len(MIX) == r)[0] for r, name in enumerate(MIX)}


def land_columns(ncol):
    """as tests/test_regimes_gpu.py masks them"""
    return np.arange(5, ncol, 23)


def deep_from(nz):
    """the first level (0-based) of the strong deep currents: below the 64th level where the depth has one, so that
    the damped-level counts cross a wave boundary (tests/test_options_gpu.py, prep_damp)"""
    return min(60, nz - 8), min(66, nz - 4)


def column_mix(switches):
    """A hook of the shape of rc.regime_mix, for a switch set: the regimes of MIX dealt by column index modulo 12, so
    that every workgroup holds different ones side by side -
      plain                 the generators' stratified start
      shallow, shallow_reversed, reef    bathymetry 0.5 ... 20 m, 40 ... 0.5 m, 0.5 ... 6 m: the sea floor clamps, also
                            the boundary layer of two or three metres that the relaxation towards a warmer SST0 leaves
      isothermal            rc.isothermal (L_NO_ISOTHERM resets it); isothermal_seafloor: over 3 ... 260 m
      tjump                 the 12 K temperature step: trapped, 11 tries of 6 passes, every step - the stragglers
      trap_u                50 m/s in the four top levels: trapped in the first step, then back at U_init
      frozen                -2.2 degC at every level (L_NO_FREEZE clamps it)
      deep_currents         3 m/s eastward from level deep_from(nz)[0], -2.5 m/s northward from deep_from(nz)[1]
      fingers, diffconv     salt fingers (rc._salt_fingers' profile) and rc.diffconv
    - and the inputs the sets read, as the closed forms of ref_step_cases (those of tests/test_options_gpu.py): SST0
    and relax_sst, fcorr_withz and sfcorr_withz, ocnT_clim, sal_clim and their rates; with L_ADVECT two advection
    modes a column, cycling through all seven.  The climatologies follow the MIXED profiles (T - 0.3, S + 0.05): a
    trapped column that clim_present resets keeps its temperature step and is trapped again in the next step.
    The hook writes its profiles into `ob` before it forms them, which apply_both then does again."""
    def hook(ncol, nzp1, ob):
        nz = nzp1 - 1
        reg = regime_columns(ncol)
        T, S, U, V = rc._profiles(ob, nzp1)
        d = np.full(ncol, -10000.0)
        for name, (lo, hi) in {"shallow": (0.5, 20.0), "shallow_reversed": (40.0, 0.5), "reef": (0.5, 6.0),
                               "isothermal_seafloor": (3.0, 260.0)}.items():
            d[reg[name]] = -np.linspace(lo, hi, len(reg[name]))
        iso = np.concatenate([reg["isothermal"], reg["isothermal_seafloor"]])
        T[iso], S[iso] = rc.isothermal(T[iso], S[iso])
        T[reg["tjump"]] = rc.tjump(T[reg["tjump"]])
        U[reg["trap_u"], 0:4] = 50.0
        T[reg["frozen"]] = -2.2
        ku, kv = deep_from(nz)
        U[reg["deep_currents"], ku:] = DEEP_U
        V[reg["deep_currents"], kv:] = DEEP_V
        S[reg["fingers"]] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
        T[reg["diffconv"]], S[reg["diffconv"]] = rc.diffconv(T[reg["diffconv"]], S[reg["diffconv"]])
        out = {"T": T, "S": S, "U": U, "V": V, "ocdepth": d}
        rc._apply_batch(ob, nzp1, out)
        for h in (rc._relax_sst, rc._fcorr_withz, rc._relax_ocnt_sal):
            out.update(h(ncol, nzp1, ob))
        if switches.get("L_ADVECT"):
            out.update(rc._adv_small_grid(range(1, 8))(ncol, nzp1, ob))
        return out
    return hook


# ---------------------------------------------------------------------------------------------------------------
# the forms: an environment, a call pattern, a shape and a step count
# ---------------------------------------------------------------------------------------------------------------
VIEWS_FORCED = {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}
NCOL, NSTEPS = 2048, 3                 # as tests/test_regimes_gpu.py::test_regimes_through_the_launch_forms
QUEUE_NCOL, QUEUE_NSTEPS = 300, 10     # fewer columns than the device has slots (test_columns_behind_the_queue_...)
L3_CAP = 5
UNIFORM, STRETCHED = (60, "uniform", 3600.0), (69, "stretched", 1200.0)
DEEP = (100, "uniform", 3600.0)


@dataclass(frozen=True)
class Form:
    name: str
    what: str
    env: dict = field(default_factory=dict, hash=False)
    one_call: bool = False
    shape: tuple = UNIFORM             # (nz, grid, dto)
    ncol: int = NCOL
    nsteps: int = NSTEPS
    geometry: str = ""                 # "most": MCKPP_PS from most_slots_geometry; else MCKPP_PS itself, or none
    runs: int = 1


FORMS = {f.name: f for f in (
    Form("F1", "a call per step"),
    Form("F2", "one call of N steps", one_call=True),
    Form("F3", "one call under MCKPP_MULTISTEP=0", {"MCKPP_MULTISTEP": "0"}, one_call=True),
    Form("F4", "views forced, a call per step", VIEWS_FORCED),
    Form("F5", "views forced, one call", VIEWS_FORCED, one_call=True),
    Form("F6", "MCKPP_VIEW_KMAX=1, one call", {"MCKPP_VIEW_KMAX": "1"}, one_call=True),
    Form("F7", "MCKPP_L2PRE=0 on the stretched 69-level grid", {"MCKPP_L2PRE": "0"}, shape=STRETCHED),
    Form("F8", "MCKPP_L2PRE=1 on the stretched 69-level grid", {"MCKPP_L2PRE": "1"}, shape=STRETCHED),
    Form("F9", "MCKPP_L3_CAP below some column's kmix", {"MCKPP_L3_CAP": str(L3_CAP)}),
    Form("F10", "MCKPP_PS=1x1x1", geometry="1x1x1"),
    Form("F11", "the most slots whose LDS fits", geometry="most"),
    Form("F12", "MCKPP_PS=5x8x2, one call", one_call=True, geometry="5x8x2"),
    Form("F13", "columns behind the queue, queues adopted (MCKPP_XCC_DROP=0x55), one call, twice",
         {"MCKPP_XCC_DROP": "0x55"}, one_call=True, ncol=QUEUE_NCOL, nsteps=QUEUE_NSTEPS, runs=2),
)}
# every MCKPP_* variable a form sets, and the two the matrix sets beside them: the GPU module clears these
ENV = sorted({k for f in FORMS.values() for k in f.env} | {"MCKPP_PS", "MCKPP_PS_FIXED_L", "MCKPP_SOLVER_MODE"})


@dataclass(frozen=True)
class Case:
    set_name: str
    solver: int
    form: str
    nz: int
    grid: str
    dto: float
    general: bool = False              # MCKPP_PS_FIXED_L=0: the general kernel at a depth that has a literal one

    @property
    def switches(self):
        return SETS[self.set_name]

    @property
    def env(self):
        f = FORMS[self.form]
        e = dict(f.env)
        if f.geometry:
            e["MCKPP_PS"] = most_slots_geometry(self.nz, self.xv) if f.geometry == "most" else f.geometry
        if self.general:
            e["MCKPP_PS_FIXED_L"] = "0"
        return e

    @property
    def xv(self):
        return instantiation(self.switches, self.solver, self.nz, {})[0]

    @property
    def instantiation(self):
        return instantiation(self.switches, self.solver, self.nz, self.env)

    @property
    def ncol(self):
        """the form's columns; half of them at 100 levels, where the first case of an oracle run - which pays for it -
        otherwise takes more than twice the slowest case of test_regimes_through_the_launch_forms (measured: 1.61 s
        against 2 x 0.79 s; profiles/coverage/kernel_variants.md).  The reach conditions hold at either size."""
        return FORMS[self.form].ncol // 2 if self.nz == DEEP[0] else FORMS[self.form].ncol

    @property
    def oracle_key(self):
        return (self.set_name, self.solver, self.nz, self.grid, self.dto, self.ncol, FORMS[self.form].nsteps)

    @property
    def id(self):
        xv, sm, lf = self.instantiation
        return f"{self.set_name}-sm{self.solver}-{self.form}-nz{self.nz}-k{xv}_{sm}_{lf}"


SETS_OF_XV = {0: ("default",), 1: ("relaxed", "corrected"), 2: ("relaxed_dd", "corrected_dd")}


def _matrix():
    """Every (XV, SM) pair through F1 ... F13, the two sets of an XV taking turns by form and solver (each set meets
    every form under one solver or the other); the literal kernels of 69 and 100 levels and, under
    MCKPP_PS_FIXED_L=0, the general ones of XV < 2 through F2 and F5 (the literal ones F1 too).  Sorted by what the
    oracle has to step, so that a small cache serves the cases one after the other."""
    out = []
    for xv, names in SETS_OF_XV.items():
        for solver in (0, 1):
            for j, f in enumerate(FORMS.values()):
                out.append(Case(names[(j + solver) % len(names)], solver, f.name, *f.shape))
            if xv == 2:
                continue
            for j, shape in enumerate((STRETCHED, DEEP)):
                for i, form in enumerate(("F1", "F2", "F5")):
                    out.append(Case(names[(i + j + solver) % len(names)], solver, form, *shape))
            for i, form in enumerate(("F2", "F5")):
                out.append(Case(names[(i + solver + 1) % len(names)], solver, form, *UNIFORM, general=True))
    return sorted(out, key=lambda c: (c.oracle_key, int(c.form[1:]), c.general))


MATRIX = _matrix()


# ---------------------------------------------------------------------------------------------------------------
# the oracle's runs, each stepped once
# ---------------------------------------------------------------------------------------------------------------
KEPT = list(rc.STEP_FIELDS) + ["status", "npasses", "old", "newi", "hmixd", "ocdepth"]


def _kept(ob, nz):
    """the compared fields of a batch, read-only: a Batch that cm.compare and harness.assert_equal_to_oracle take"""
    b = orc.Batch(ob.ncol, nz, fields=[])
    for n in {"hmixd" if n.startswith("hmixd") else n for n in KEPT}:
        b.a[n] = ob.a[n].copy()
        b.a[n].flags.writeable = False
    return b


def start(set_name, solver, nz, grid, dto, ncol, without=None, hip=False):
    """(oracle Const, Batch, land columns[, KppConstFields, Kpp3dFields]): the generators' columns with the set's
    column mix on top, before init_ocean, on the oracle and - hip=True - on the library's side from the same inputs.
    `without` names one switch of the set that is left off (for L_ADVECT, which the oracle keys on nmodeadv alone:
    no advection inputs)."""
    sw = {k: v for k, v in SETS[set_name].items() if k != without}
    oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid, dto=dto, solver_mode=solver, **sw)
    d = column_mix(sw)(ncol, nz + 1, ob)
    land = land_columns(ncol)
    if not hip:
        rc._apply_batch(ob, nz + 1, d)
        return oc, ob, land
    kc, k3 = cm.make_hip_case(ncol, nz, grid=grid, dto=dto)
    for k, v in sw.items():
        setattr(kc, k, v)
    rc.apply_both(ob, k3, nz + 1, d)
    k3.run_physics[land] = 0
    k3.l_ocean[land] = 0
    return oc, ob, land, kc, k3


@dataclass
class Run:
    active: np.ndarray       # the columns that are no land
    init: object             # the state after init_ocean
    steps: list              # the state after each step


@functools.lru_cache(maxsize=3)
def oracle_run(set_name, solver, nz, grid, dto, ncol, nsteps, without=None):
    """The oracle from start(...) through init_ocean and `nsteps` steps of the bench forcing, one model step at a
    time.  Cached: MATRIX is sorted by this function's arguments, so the GPU module steps each of its 32 runs once, and
    so does the CPU module but for the five that test_every_switch_counts comes back to (0.7 s each).  The cache is
    small and its arrays read-only in place of copies: a run of 2048 columns is about 150 MB."""
    oc, ob, land = start(set_name, solver, nz, grid, dto, ncol, without)
    active = np.setdiff1d(np.arange(ncol), land)
    orc.init_ocean(oc, ob, 0)
    init = _kept(ob, nz)
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    steps = []
    for nt in range(1, nsteps + 1):
        orc.physics_driver(oc, ob, nt)
        steps.append(_kept(ob, nz))
    return Run(active, init, steps)


def run_of(case, without=None):
    return oracle_run(*case.oracle_key, without=without)


# ---------------------------------------------------------------------------------------------------------------
# what the mix reaches (the conditions tests/test_variants_cpu.py asserts; the figures of the record)
# ---------------------------------------------------------------------------------------------------------------
TRAPPED_AT_LEAST = CLAMPED_AT_LEAST = 0.05
REACHED_AT_LEAST, SWITCH_AT_LEAST = 0.02, 0.01
CORRECTIONS = {"tinc_fcorr": ("L_FCORR_WITHZ", "L_RELAX_OCNT"), "ocnTcorr": ("L_FCORR_WITHZ", "L_RELAX_OCNT"),
               "sinc_fcorr": ("L_SFCORR_WITHZ", "L_RELAX_SAL"), "scorr": ("L_SFCORR_WITHZ", "L_RELAX_SAL")}


def reach(run, set_name, nz):
    """{what: (bound, the smallest fraction of the active columns over the steps of `run`)}: trapped and clamped
    columns for every set, and whatever the set's switches exist for - the flags of check_profile, non-zero
    corrections (below level 64 where the depth has one), under LDD a dift that differs from difs on some level
    below the boundary layer."""
    sw, act = SETS[set_name], run.active
    deep = slice(64, nz + 2) if nz >= 64 else slice(1, nz + 2)

    def frac(f):
        return min(float(np.mean(f(ob))) for ob in run.steps)

    out = {"trapped": (TRAPPED_AT_LEAST, frac(lambda ob: (ob["status"][act] & 12 == 12) & (ob["npasses"][act] >= 66))),
           "clamped": (CLAMPED_AT_LEAST, frac(lambda ob: ob["hmix"][act] == -ob["ocdepth"][act]))}
    if sw.get("L_DAMP_CURR"):
        out["damped"] = (REACHED_AT_LEAST, frac(lambda ob: (ob["dampu_flag"][act] > 0) | (ob["dampv_flag"][act] > 0)))
    if sw.get("L_NO_FREEZE"):
        out["frozen"] = (REACHED_AT_LEAST, frac(lambda ob: ob["freeze_flag"][act] > 0))
    if sw.get("L_NO_ISOTHERM"):
        out["reset_isothermal"] = (REACHED_AT_LEAST, frac(lambda ob: ob["reset_flag"][act] < 0))
        out["reset_trapped"] = (REACHED_AT_LEAST, frac(lambda ob: np.abs(ob["reset_flag"][act]) == 999))
    if sw.get("L_RELAX_SST"):
        out["fcorr"] = (REACHED_AT_LEAST, frac(lambda ob: ob["fcorr"][act] != 0))
    for name, needs in CORRECTIONS.items():
        if any(sw.get(k) for k in needs):
            out[name] = (REACHED_AT_LEAST, frac(lambda ob, name=name: (ob[name][act][:, deep] != 0).any(axis=1)))
    if sw.get("LDD"):
        k = np.arange(nz + 4)[None, :]

        def below(ob):
            under = (k > ob["kmix"][act][:, None]) & (k <= nz)
            return ((ob["dift"][act] != ob["difs"][act]) & under).any(axis=1)
        out["dift_not_difs"] = (REACHED_AT_LEAST, frac(below))
    return out


def columns_differing(a, b, active, fields=rc.STEP_FIELDS):
    """{field: fraction of the active columns on which two states differ in some bit of it} (canonical zeros, NaNs)"""
    out = {}
    for n in fields:
        x, y = (rc.canonical(rc.field_of(s, n, s.nz))[active].view(np.int64) for s in (a, b))
        d = x != y
        out[n] = float(np.mean(d.any(axis=1) if d.ndim > 1 else d))
    return out


if __name__ == "__main__":      # the tables of profiles/coverage/kernel_variants.md
    head = " | ".join(FORMS) + " |\n|---|" + "---|" * len(FORMS)
    print("| instantiation | " + head)
    for inst in sorted(compiled_instantiations()):
        cells = ["<br>".join(c.id for c in MATRIX if c.instantiation == inst and c.form == f) or "empty" for f in FORMS]
        print(f"| `<{inst[0]}, {inst[1]}, {inst[2]}>` | " + " | ".join(cells) + " |")
    print()
    for key in sorted({c.oracle_key for c in MATRIX if c.solver == 0}):
        r = reach(oracle_run(*key), key[0], key[2])
        print(f"| {key[0]} | {key[2]} {key[3]} | {key[5]} x {key[6]} | "
              + ", ".join(f"{k} {100 * v:.1f} %" for k, (_, v) in r.items()) + " |")
