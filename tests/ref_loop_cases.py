"""The reference-pinned loop cases: raw seeded profiles and flux records on which the compiled reference's OWN start of
a run (mckpp_initialize_time, mckpp_initialize_fluxes, mckpp_initialize_ocean_model, which computes tri itself) and
its own time loop (mckpp_update_time, mckpp_fluxes at the update steps through its own flux reader and
mckpp_get_update_time, mckpp_physics_driver) are recorded (tests/golden/make_ref_loop_golden.py ->
tests/golden/ref_loop.npz), and against which the oracle (tests/test_ref_loop_cpu.py) and the HIP paths
(tests/test_ref_loop_gpu.py) are asserted bit for bit.

The starting state is what the reference's init receives: the profiles of mckpp_f90_amd.synth before any init (plus a
seeded smooth perturbation where a case asks for it), Jerlov types, land mask.  The flux records are seeded per case;
record r (0-based) is the one the run reads at step r*ndtocn + 1 - in the reference because its reader finds it by
time, in the oracle and the HIP paths because the driver here / mckpp_hip_run_forced take index (nt-1)//ndtocn.

Not reachable through the reference, and therefore not pinned here: `snow` (the reference's reader sets it to zero,
src/mckpp_read_fluxes_mod.F90:104, so flsn never matters there; the records keep snow = 0), mckpp_boundary_update,
XIOS output."""
import hashlib
import os
from dataclasses import dataclass, field

import numpy as np

import common as cm
import ref_step_cases as rc
from oracle import orc

canonical, digest = rc.canonical, rc.digest

SFLUX_ROWS = [f"sflux{i}" for i in range(1, 7)]
BOOKKEEPING = ["old", "newi"]
# after init: everything the suite compares after a step (which holds wU, wX, Us, Xs, hmixd, hmix, kmix, Tref),
# old / new, and the tridiagonal factors the reference's init computed
INIT_FIELDS = rc.STEP_FIELDS + BOOKKEEPING + ["tri0", "tri1"]
# after every step: the same set (wXNT1 and swdk_opt are in it), old / new, and the six sflux rows
LOOP_FIELDS = rc.STEP_FIELDS + BOOKKEEPING + SFLUX_ROWS
CORE = ["T", "hmix", "kmix", "wXNT1"] + SFLUX_ROWS       # of the last step in full, on the small cases
BUILDS = {"libm": 0, "pexp": 1}
FLUX_NAMES = cm.synth.FLUX_NAMES
# mckpp_fluxes without a flux file (src/mckpp_fluxes_mod.F90:41-49): taux tauy swf lwf lhf shf rain snow
NO_FILE_CONSTANTS = (0.01, 0.0, 200.0, 0.0, -150.0, 0.0, 6e-5, 0.0)
FLSN, EL = cm.synth.FLSN, cm.synth.EL


@dataclass
class LoopCase:
    ncol: int
    nz: int
    nsteps: int
    ndtocn: int
    seed: int
    grid: str = "uniform"
    dto: float = 3600.0
    switches: dict = field(default_factory=dict)
    land_every: int = 0            # l_ocean = run_physics = 0 on every land_every-th column
    calm_every: int = 0            # record r has taux == tauy == 0 exactly where (column + r) % calm_every == 0
    sun: bool = False              # swf follows the sun (records of exactly zero at night); else random per record
    perturb: bool = False          # a seeded smooth perturbation of T per column (sweeps)
    salt_fingers: bool = False     # every other column salty over fresh, so that LDD's dift differs from difs
    l_rest: int = 0
    flux_file: bool = True         # False: l_fluxdata = .FALSE., the eight constants
    startt: float = 0.0            # days
    full: bool = True              # record CORE of the last step in full too (else: digests only)


CASES = {
    # every step a flux update, all five Jerlov types, land columns, calm points
    "every_step_nz40": LoopCase(40, 40, 12, 1, seed=101, land_every=4, calm_every=5),
    # flux interval longer than a step, the sun with records of exactly zero short wave
    "diurnal_nz60_nd3": LoopCase(30, 60, 24, 3, seed=102, sun=True, land_every=7, calm_every=6),
    # the shipped namelist's shape: 69 stretched levels, 20-minute steps, about a third land
    "namelist_nz69_nd2": LoopCase(36, 69, 8, 2, seed=103, grid="stretched", dto=1200.0, land_every=3, calm_every=5),
    "deep_nz100_nd4": LoopCase(24, 100, 12, 4, seed=104, full=False),
    "l_rest": LoopCase(20, 40, 4, 2, seed=105, l_rest=1, land_every=6),
    "no_flux_file": LoopCase(20, 40, 4, 2, seed=106, flux_file=False, land_every=6),
    "ldd_nz60": LoopCase(24, 60, 4, 1, seed=107, switches=dict(LDD=1), salt_fingers=True),
    "startt_nd3": LoopCase(20, 40, 7, 3, seed=108, startt=17.3, calm_every=4),
    # the seeded sweeps: a model day of 2000 columns with random shapes of forcing
    "sweep_nd1": LoopCase(2000, 60, 24, 1, seed=109, sun=True, perturb=True, land_every=11, calm_every=9, full=False),
    "sweep_nd3": LoopCase(2000, 40, 24, 3, seed=110, sun=True, perturb=True, land_every=13, calm_every=8, full=False),
}


def nrec(case):
    return (case.nsteps + case.ndtocn - 1) // case.ndtocn


def jerlov(case):
    return (1 + (np.arange(case.ncol) % 5)).astype(np.int32)


def ocean(case):
    """l_ocean = run_physics of the case (1 = ocean)"""
    m = np.ones(case.ncol, dtype=np.int32)
    if case.land_every:
        m[::case.land_every] = 0
    return m


def active_columns(case):
    """the columns the reference works on (all but land); digests are over these"""
    return np.nonzero(ocean(case))[0]


def calm(case, r):
    """columns of record r with taux == tauy == 0 exactly (never the same column in two successive records)"""
    c = np.zeros(case.ncol, dtype=bool)
    if case.calm_every:
        c[(np.arange(case.ncol) + r) % case.calm_every == 0] = True
    return c


def flux_records(case):
    """[nrec, 8, ncol] taux tauy swf lwf lhf shf rain snow, record r for steps r*ndtocn + 1 ..; every case has them
    (the case without a flux file holds the reference's eight constants, which is what the oracle and the HIP paths
    are then given)."""
    n, ncol = nrec(case), case.ncol
    if not case.flux_file:
        return np.ascontiguousarray(np.broadcast_to(np.array(NO_FILE_CONSTANTS)[None, :, None], (n, 8, ncol)))
    rng = np.random.default_rng(case.seed)
    rec = np.zeros((n, 8, ncol))
    cloud = rng.uniform(0.4, 1.0, ncol)
    for r in range(n):
        rec[r, 0] = rng.uniform(-0.2, 0.3, ncol)
        rec[r, 1] = rng.uniform(-0.1, 0.1, ncol)
        if case.sun:      # the sun at the middle of the record's interval, seen through a column's own cloud
            t = case.startt * 86400.0 + (r + 0.5) * case.ndtocn * case.dto
            rec[r, 2] = max(0.0, 800.0 * np.sin(2.0 * np.pi * t / 86400.0)) * cloud * rng.uniform(0.9, 1.0, ncol)
        else:
            rec[r, 2] = rng.uniform(0.0, 800.0, ncol)
        rec[r, 3] = rng.uniform(-80.0, -20.0, ncol)
        rec[r, 4] = rng.uniform(-300.0, 0.0, ncol)
        rec[r, 5] = rng.uniform(-40.0, 10.0, ncol)
        rec[r, 6] = rng.uniform(0.0, 1e-4, ncol)
        c = calm(case, r)
        rec[r, 0, c] = 0.0
        rec[r, 1, c] = 0.0
    return rec


def profile_changes(case, ob):
    """{batch field: array (ncol, nzp1)} laid over synth's profiles before any init"""
    nzp1 = case.nz + 1
    d = {}
    if case.perturb:
        rng = np.random.default_rng(case.seed + 1000)
        zm = cm.grid_for(case.nz, case.grid)[0]
        z = -zm[1:nzp1 + 1]
        amp, depth = rng.uniform(-1.0, 1.0, case.ncol), rng.uniform(10.0, 100.0, case.ncol)
        d["T"] = ob["T"][:, 1:nzp1 + 1] + amp[:, None] * np.exp(-z[None, :] / depth[:, None])
    if case.salt_fingers:
        S = ob["S"][:, 1:nzp1 + 1].copy()
        S[::2] = 0.4 - 0.8 * np.linspace(0, 1, nzp1)[None, :]
        d["S"] = S
    return d


def oracle_raw(case, exp_mode):
    """(Const, Batch, changes): the oracle's constants and the raw columns of the case, nothing initialised"""
    oc, ob = cm.make_oracle(case.ncol, case.nz, init=False, exp_mode=exp_mode, grid=case.grid, dto=case.dto,
                            solver_mode=0, **case.switches)
    ob["jerlov"] = jerlov(case)
    ob["l_ocean"] = ocean(case)
    ch = profile_changes(case, ob)
    rc._apply_batch(ob, case.nz + 1, ch)
    return oc, ob, ch


def input_digest(case, ob, rec):
    """One SHA-256 over what a run of the case is given: every field of the raw batch, the flux records, the masks
    and the switches of the run."""
    h = hashlib.sha256()
    for k in rc.INPUT_FIELDS + ["sflux"]:
        h.update(k.encode())
        h.update(canonical(ob[k]).tobytes())
    h.update(canonical(rec).tobytes())
    h.update(canonical(ocean(case)).tobytes())
    h.update(repr((case.nz, case.nsteps, case.ndtocn, case.grid, case.dto, sorted(case.switches.items()), case.l_rest,
                   case.flux_file, case.startt)).encode())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def field_of(ob, name, nz, tri=None):
    """Batch field `name` over the range the suite compares; tri = (tri0, tri1) for the two factors"""
    if name in SFLUX_ROWS:
        return ob["sflux"][:, int(name[-1]) - 1]
    if name in BOOKKEEPING:
        return ob[name]
    if name in ("tri0", "tri1"):
        return tri[int(name[-1])][0:nz + 1]
    return rc.field_of(ob, name, nz)


def hip_get(k3, kc, nz):
    """get(field) on a HIP Kpp3dFields / KppConstFields"""
    base = rc.hip_get(k3, nz)

    def get(name):
        if name in SFLUX_ROWS:
            return k3.sflux[:, int(name[-1]) - 1, 4, 0]
        if name in BOOKKEEPING:
            return {"old": k3.old, "newi": k3.new_}[name]
        if name in ("tri0", "tri1"):
            return kc.tri[0:nz + 1, int(name[-1]), 0]
        return base(name)
    return get


def batch_get(ob, nz, tri=None):
    return lambda name: field_of(ob, name, nz, tri)


def _over_columns(case, name, a):
    a = np.asarray(a)
    return a if name in ("tri0", "tri1") else a[active_columns(case)]


def digests_of(case, names, get):
    return np.array([digest(_over_columns(case, n, get(n))) for n in names])


# ---------------------------------------------------------------------------
# the reference and the oracle through a case
# ---------------------------------------------------------------------------
def run_reference(case, exp_mode):
    """The compiled reference through the case: ((Batch after init, tri0, tri1), [Batch after each step])"""
    oc, ob, _ = oracle_raw(case, exp_mode)
    init = orc.ref_init(oc, ob, exp_mode=exp_mode, run_physics=ocean(case),
                        flux_records=flux_records(case) if case.flux_file else None, ndtocn=case.ndtocn,
                        startt=case.startt, l_rest=case.l_rest, flsn=FLSN, el=EL)
    return init, orc.ref_loop(1, case.nsteps, exp_mode)


def oracle_record_index(case, nt):
    """The flux record the oracle's loop takes at update step nt (the reference finds its own by time)."""
    return (nt - 1) // case.ndtocn


def run_oracle(case, exp_mode):
    """The oracle driven as the reference's loop: yields (0, Const, Batch) after init_ocean, then (nt, Const, Batch)
    after every step; orc.fluxes only at the update steps, with record oracle_record_index(nt)."""
    oc, ob, _ = oracle_raw(case, exp_mode)
    rec = flux_records(case)
    orc.init_ocean(oc, ob, 0)
    yield 0, oc, ob
    for nt in range(1, case.nsteps + 1):
        if (nt - 1) % case.ndtocn == 0:
            orc.fluxes(oc, ob, nt, **dict(zip(FLUX_NAMES, rec[oracle_record_index(case, nt)])), l_rest=case.l_rest,
                       flsn=FLSN, el=EL)
        orc.physics_driver(oc, ob, nt)
        yield nt, oc, ob


def record(case, init, steps):
    """What the golden file keeps of one build's run of the case."""
    ib, t0, t1 = init
    out = {"init_sha": digests_of(case, INIT_FIELDS, batch_get(ib, case.nz, (t0, t1))),
           "sha": np.array([digests_of(case, LOOP_FIELDS, batch_get(s, case.nz)) for s in steps])}
    if case.full:
        for name in CORE:
            out[f"val/{name}"] = canonical(_over_columns(case, name, field_of(steps[-1], name, case.nz)))
    return out


def first_difference(case, name, got, want):
    """'column c level k: got x, recorded y' of the first differing value (columns as the case numbers them)"""
    g, w = canonical(got), canonical(want)
    if g.shape != w.shape:
        return f"shape {g.shape} against {w.shape}"
    idx = np.argwhere(g.view(np.int64) != w.view(np.int64))
    if not len(idx):
        return None
    i = tuple(idx[0])
    col = i[0] if name in ("tri0", "tri1") else int(active_columns(case)[i[0]])
    where = f"level index {col}" if name in ("tri0", "tri1") else \
        f"column {col}" + (f" level index {i[1]}" if len(i) > 1 else "")
    return f"{where}: got {g[i]!r}, reference {w[i]!r} ({len(idx)} values differ)"


def mismatches(case, names, want_sha, get, values=None):
    """{field: what differs} between a state (get(field)) and the recorded digests want_sha[len(names), 32] over the
    active columns; `values` {field: array} names the first differing value where the record holds the field."""
    bad = {}
    for i, name in enumerate(names):
        v = _over_columns(case, name, get(name))
        if not np.array_equal(digest(v), want_sha[i]):
            bad[name] = (first_difference(case, name, v, values[name]) if values and name in values
                         else "digest differs")
    return bad


# ---------------------------------------------------------------------------
# the HIP paths
# ---------------------------------------------------------------------------
def hip_raw(case):
    """(KppConstFields, Kpp3dFields) with the raw columns of the case"""
    kc, k3 = cm.make_hip_case(case.ncol, case.nz, grid=case.grid, dto=case.dto, land_every=case.land_every)
    for k, v in case.switches.items():
        setattr(kc, k, v)
    k3.jerlov[:] = jerlov(case)
    rc.apply_hip(k3, oracle_raw(case, 1)[2])
    assert np.array_equal(k3.l_ocean, ocean(case)) and np.array_equal(k3.run_physics, ocean(case))
    return kc, k3


class Golden:
    """tests/golden/ref_loop.npz: per case and build ("libm", "pexp") the digest of the inputs, of every INIT_FIELDS
    field after the reference's init and of every LOOP_FIELDS field after every step of its loop; for the portable-exp
    build the CORE fields of the last step in full (small cases)."""

    def __init__(self):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loop.npz")
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        assert list(self.z["init_fields"]) == INIT_FIELDS and list(self.z["loop_fields"]) == LOOP_FIELDS, \
            "tests/golden/ref_loop.npz records another field list"

    def cases(self):
        return sorted({k.split("/")[0] for k in self.z if "/" in k})

    def input_sha(self, tag, build):
        return self.z[f"{tag}/{build}/input_sha"]

    def init_sha(self, tag, build):
        return self.z[f"{tag}/{build}/init_sha"]

    def sha(self, tag, build):
        return self.z[f"{tag}/{build}/sha"]

    def values(self, tag, build):
        p = f"{tag}/{build}/val/"
        return {k[len(p):]: v for k, v in self.z.items() if k.startswith(p)}
