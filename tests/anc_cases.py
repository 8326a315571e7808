"""Cases of the ancillary record series (mckpp_hip_set_ancillary_series / mckpp_hip_ancillary_schedule): the same set-up
for the CPU oracle and the HIP side, the records of every kind as closed forms of column, level and record number, and
the oracle's run - one step at a time, the field of the step's epoch written into its state before the step, an
interpolated field formed in numpy as nxt*wn + prv*wp (two products and a sum, as boundary_interpolate.F90:60, :115).
Nothing here touches a GPU."""
import functools

import numpy as np

import common as cm
import ref_step_cases as rc
from mckpp_f90_amd import api as A
from oracle import orc

# name -> (kind, the oracle batch's field or None, values per column: 1 or nzp1)
KINDS = {
    "SST0": (A.ANC_SST0, "SST0", False),
    "fcorr_twod": (A.ANC_FCORR_TWOD, "fcorr_twod", False),
    "fcorr_withz": (A.ANC_FCORR_WITHZ, "fcorr_withz", True),
    "sfcorr_withz": (A.ANC_SFCORR_WITHZ, "sfcorr_withz", True),
    "ocnT_clim": (A.ANC_OCNT_CLIM, "ocnT_clim", True),
    "sal_clim": (A.ANC_SAL_CLIM, "sal_clim", True),
    "bottom_temp": (A.ANC_BOTTOM_TEMP, None, False),
}


def record(name, r, T, S):
    """Record number r of a kind: (ncol) or (ncol, nzp1), from the starting profiles T, S (ncol, nzp1).  Records of
    different numbers differ on every column (at every level)."""
    ncol, nzp1 = T.shape
    c = np.arange(ncol, dtype=float)
    z = np.arange(nzp1, dtype=float)[None, :]
    if name == "SST0":
        return T[:, 0] + 1.5 + 0.4 * r + 0.1 * np.sin(c + r)
    if name == "fcorr_twod":
        return np.linspace(-80.0, 80.0, ncol) + 30.0 * r + 5.0 * np.sin(c + r)
    if name == "fcorr_withz":
        return 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, ncol)[:, None] + 0.8 * r * np.exp(-z / 12.0) + 0.0 * c[:, None]
    if name == "sfcorr_withz":
        return 1e-7 * np.cos(z / 7.0) + 4e-8 * r * np.exp(-z / 9.0) + 0.0 * c[:, None]
    if name == "ocnT_clim":
        return T - 0.3 + 0.2 * r + 0.05 * np.sin(c[:, None] + z / 5.0 + r)
    if name == "sal_clim":
        return S + 0.05 + 0.02 * r + 0.005 * np.cos(c[:, None] + z / 4.0 + r)
    if name == "bottom_temp":
        return T[:, nzp1 - 1] - 0.5 + 0.25 * np.sin(c + r) + 0.1 * r
    raise KeyError(name)


# ---------------------------------------------------------------------------
# what is set before init_ocean, on both sides ({batch field: array}, ref_step_cases.apply_both)
# ---------------------------------------------------------------------------
def _rates(ncol, nzp1, ob):
    """every relaxation rate non-zero on every column, and every field the switches may read at its record 0"""
    T, S = ob["T"][:, 1:nzp1 + 1].copy(), ob["S"][:, 1:nzp1 + 1].copy()
    r = np.full(ncol, 1.0 / (5 * 86400.0))
    d = {"relax_sst": r, "relax_ocnT": r / 6, "relax_sal": r / 3}
    for n, (_, f, _) in KINDS.items():
        if f:
            d[f] = record(n, 0, T, S)
    return d


def _tjump_records(ncol, nzp1, ob):
    """ref_step_cases' 12 K temperature step on every third column, with the rates above"""
    d = _rates(ncol, nzp1, ob)
    d.update(rc._tjump(ncol, nzp1, ob))
    return d


def _isothermal_records(ncol, nzp1, ob):
    d = _rates(ncol, nzp1, ob)
    T = ob["T"][:, 1:nzp1 + 1].copy()
    T[1::3, :] = 12.0
    d["T"] = T
    return d


PRE = {"rates": _rates, "tjump": _tjump_records, "isothermal": _isothermal_records}


def special_records(pre, name, r, rec, T):
    """The reset cases: the climatology a reset restores carries the condition of the next reset, so that resets fall
    in later epochs too - the temperature step again (every record but the last), or an isothermal column again."""
    if pre == "tjump" and name == "ocnT_clim" and r < 3:
        rec = rec.copy()
        rec[::3] = rc.tjump(rec[::3])
    if pre == "isothermal" and name == "ocnT_clim" and r < 3:
        rec = rec.copy()
        rec[1::3, :] = 11.0 + r
    return rec


def both(ncol, nz, grid="uniform", land_every=7, pre="rates", solver_mode=None, itermax=None, **switches):
    """Oracle const + batch and the HIP side's constants + fields of one case, before initialisation; and the starting
    profiles the records are made from."""
    oc, ob, kc, k3 = cm.make_both(ncol, nz, grid, land_every, solver_mode, itermax, **switches)
    T, S = ob["T"][:, 1:nz + 2].copy(), ob["S"][:, 1:nz + 2].copy()
    rc.apply_both(ob, k3, nz + 1, PRE[pre](ncol, nz + 1, ob))
    return oc, ob, kc, k3, (T, S)


def nrec_of(epochs):
    return 1 + max(max(e[0], e[1]) if np.ndim(e) else e for e in epochs)


def records_of(sched, T, S, pre="rates"):
    """{kind name: [nrec, ncol(, nzp1)]} for a schedule {kind name: (cadence, epochs)}"""
    return {n: np.stack([special_records(pre, n, r, record(n, r, T, S), T) for r in range(nrec_of(ep))])
            for n, (cad, ep) in sched.items()}


def field_at(recs, cadence, epochs, nt, origin=1):
    e = epochs[(nt - origin) // cadence]
    if np.ndim(e) == 0:
        return recs[e]
    p, n, wp, wn = e
    return recs[n] * wn + recs[p] * wp


def put_field(ob, nz, name, f):
    """the field of a step's epoch into the oracle's state (bottom_temp: applied after the step, orc.bottomtemp)"""
    fld, is3d = KINDS[name][1], KINDS[name][2]
    if is3d:
        ob.a[fld][:, 1:nz + 2] = f
    elif fld:
        ob[fld] = f


class Run:
    """what the oracle's run of a case leaves: the batch after the last step; status words, pass counts and reset flags of
    every step; the records; the active points"""


@functools.lru_cache(maxsize=None)
def oracle_run(ncol, nz, nsteps, sched_key, hold_record0=False, series_key=None, ndtocn=1, **case):
    """The oracle's run, once per case, shared and left unchanged.  sched_key: tuple of (name, cadence, epochs).
    hold_record0: every step reads record 0 (the run the reach conditions compare with).  series_key: seed of a flux
    series applied every ndtocn steps (None: the bench forcing, constant)."""
    sched = {n: (cad, ep) for n, cad, ep in sched_key}
    oc, ob, kc, k3, (T, S) = both(ncol, nz, **case)
    out = Run()
    out.active = np.nonzero(k3.run_physics)[0]
    out.recs = records_of(sched, T, S, case.get("pre", "rates"))
    orc.init_ocean(oc, ob, 0)
    if series_key is None:
        ob["sflux"] = cm.synth.forcing(ncol, "bench")
    else:
        out.series = flux_series(ncol, -(-nsteps // ndtocn), series_key)
    out.status, out.npasses, out.reset_flags, out.batches = [], [], [], []
    for nt in range(1, nsteps + 1):
        if series_key is not None and (nt - 1) % ndtocn == 0:
            orc.fluxes(oc, ob, nt, **dict(zip(cm.synth.FLUX_NAMES, out.series[(nt - 1) // ndtocn])))
        for n, (cad, ep) in sched.items():
            put_field(ob, nz, n, out.recs[n][0] if hold_record0 else field_at(out.recs[n], cad, ep, nt))
        orc.physics_driver(oc, ob, nt)
        if "bottom_temp" in sched:
            cad, ep = sched["bottom_temp"]
            orc.bottomtemp(oc, ob, out.recs["bottom_temp"][0] if hold_record0 else field_at(out.recs["bottom_temp"], cad, ep, nt))
        out.status.append(np.array(ob["status"]))
        out.npasses.append(np.array(ob["npasses"]))
        out.reset_flags.append(np.array(ob["reset_flag"]))
    out.ob = ob
    return out


def flux_series(ncol, nrec, seed):
    rng = np.random.default_rng(seed)
    series = np.empty((nrec, 8, ncol))
    for r in range(nrec):
        series[r] = [rng.uniform(-0.2, 0.3, ncol), rng.uniform(-0.1, 0.1, ncol), 300.0 * (r % 3) * np.ones(ncol),
                     rng.uniform(-80, -20, ncol), rng.uniform(-300, 0, ncol), rng.uniform(-40, 10, ncol),
                     rng.uniform(0, 1e-4, ncol), np.zeros(ncol)]
    return series


def key(sched):
    return tuple((n, cad, tuple(ep)) for n, (cad, ep) in sched.items())


def differs_on(a, b, nz, active):
    """the active columns on which two oracle batches differ in some field of STEP_FIELDS"""
    diff = np.zeros(len(active), bool)
    for name in rc.STEP_FIELDS:
        x, y = np.asarray(rc.field_of(a, name, nz))[active], np.asarray(rc.field_of(b, name, nz))[active]
        ne = ~((x == y) | (np.isnan(x) & np.isnan(y)))
        diff |= ne.reshape(len(active), -1).any(axis=1)
    return diff


def stepwise(cadence, nsteps):
    """epochs of a stepwise schedule over nsteps from step 1: epoch e is record e"""
    return tuple(range(-(-nsteps // cadence)))


def interpolated(nsteps):
    """cadence 1: every step its own pair and weights - 0 and 1, and weights whose products are inexact"""
    w = [(1.0, 0.0), (1.0 - 1.0 / 3.0, 1.0 / 3.0), (1.0 / 3.0, 1.0 - 1.0 / 3.0), (0.0, 1.0), (19.0 / 30.0, 11.0 / 30.0),
         (0.9, 0.1)]
    return tuple((i // 3, i // 3 + 1, w[i % len(w)][0], w[i % len(w)][1]) for i in range(nsteps))


def mixed(nsteps):
    """interpolated and stepwise epochs in one table"""
    ep = list(interpolated(nsteps))
    for i in range(0, nsteps, 4):
        ep[i] = i // 3
    return tuple(ep)
