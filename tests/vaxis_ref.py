"""The yardstick of the caller's vertical axes (include/mckpp_hip_vaxis.h): a numpy restatement of the reference's
vertical interpolation and of what it does with its initial profiles.

No compiled piece of the reference under oracle/_ref reaches mckpp_initialize_ocean_profiles_vinterp, so this module is
written from the source, src/mckpp_initialize_ocean_profiles_mod.F90:122-159 (vinterp) and :83-117 (the Kelvin rule, the
reference salinity, the surface references): one numpy operation per rounded operation - numpy contracts nothing -, the
tests of the branches as the reference writes them (.GT. and .LT., so equality takes the bracket), and the search for
the bracket as the reference has it: one DO WHILE whose kin is carried from one target level to the next.  The
expression `var_in(kin) + deltavar * (model_z(k) - var_z(kin)) / deltaz` is evaluated left to right: the product, then
the quotient, then the sum.

smallest_brackets states the rule the header gives for the same bracket - the smallest index whose lower level is not
above the target - without carrying anything; tests/test_vaxis_cpu.py holds the two to each other and both to the
library's table.

Arrays here are (levels, points), the layout of the caller's planes; heights are negative downwards like zm and
strictly decreasing.  No GPU, no library."""
import numpy as np

ABOVE, BELOW, BRACKET = 0, 1, 2


def carried_brackets(zs, zt):
    """(branch, kin) per target, 0-based, by the reference's :136-148: kin starts at the first level and the DO WHILE
    moves it on, for bracketed targets only, never back.  A clamped target reads level kin = 0 (ABOVE) or len(zs) - 1
    (BELOW)."""
    zs, zt = np.asarray(zs, dtype=np.float64), np.asarray(zt, dtype=np.float64)
    n = len(zs)
    branch, kin_of = np.zeros(len(zt), dtype=np.int32), np.zeros(len(zt), dtype=np.int32)
    kin = 0
    for k in range(len(zt)):
        if zt[k] > zs[0]:
            branch[k], kin_of[k] = ABOVE, 0
        elif zt[k] < zs[n - 1]:
            branch[k], kin_of[k] = BELOW, n - 1
        else:
            while zs[kin + 1] > zt[k]:
                kin += 1
            branch[k], kin_of[k] = BRACKET, kin
    return branch, kin_of


def smallest_brackets(zs, zt):
    """(branch, kin) per target by the header's rule: kin is the smallest index with zs[kin + 1] <= zt"""
    zs, zt = np.asarray(zs, dtype=np.float64), np.asarray(zt, dtype=np.float64)
    n = len(zs)
    branch, kin_of = np.zeros(len(zt), dtype=np.int32), np.zeros(len(zt), dtype=np.int32)
    for k in range(len(zt)):
        if zt[k] > zs[0]:
            branch[k], kin_of[k] = ABOVE, 0
        elif zt[k] < zs[n - 1]:
            branch[k], kin_of[k] = BELOW, n - 1
        else:
            branch[k], kin_of[k] = BRACKET, min(i for i in range(n - 1) if zs[i + 1] <= zt[k])
    return branch, kin_of


def levels_read(zs, zt):
    """per target the source levels its branch reads: one for a clamp, two for a bracket"""
    branch, kin = carried_brackets(zs, zt)
    return [(int(i),) if b != BRACKET else (int(i), int(i) + 1) for b, i in zip(branch, kin)]


def vinterp(zs, vs, zt):
    """vs (len(zs), npts), float64 or float32 - widened exactly first -, onto the targets zt: (len(zt), npts) float64"""
    zs, zt = np.asarray(zs, dtype=np.float64), np.asarray(zt, dtype=np.float64)
    vs = np.asarray(vs).astype(np.float64)
    assert vs.shape[0] == len(zs) and (np.diff(zs) < 0).all()
    n = len(zs)
    out = np.empty((len(zt),) + vs.shape[1:])
    kin = 0
    for k in range(len(zt)):
        if zt[k] > zs[0]:                                   # :139-140
            out[k] = vs[0]
        elif zt[k] < zs[n - 1]:                             # :142-143
            out[k] = vs[n - 1]
        else:
            while zs[kin + 1] > zt[k]:                      # :146-148
                kin += 1
            deltaz = zs[kin] - zs[kin + 1]                  # :149
            deltavar = vs[kin] - vs[kin + 1]                # :150
            t = zt[k] - zs[kin]
            p = deltavar * t                                # :151-152, left to right
            q = p / deltaz
            out[k] = vs[kin] + q
    return out


def untouched(zs, vs, zt, skip):
    """(len(zt), npts) bool: the target levels MCKPP_PUT_SKIP leaves alone - an input value their branch reads equals skip"""
    vs = np.asarray(vs).astype(np.float64)
    hit = vs == skip
    return np.array([np.any([hit[i] for i in lv], axis=0) for lv in levels_read(zs, zt)])


def init_profiles(zm, u, v, temp, sal, zvel, ztemp, zsal, tk0, l_ssref, resident=None):
    """The reference's :55-117 on arrays (levels, points): a dict of U, V, U_init, V_init, T, X2 as (nzp1, npts) and
    Sref, SSref, Tref, Ssurf as (npts,).  resident: the points the Kelvin rule's ANY looks at - the library's resident
    columns; None: every point, which is the reference's own rule, land included."""
    U, V = vinterp(zvel, u, zm), vinterp(zvel, v, zm)                        # :55-61
    T = vinterp(ztemp, temp, zm)                                            # :78-79
    seen = T if resident is None else T[:, np.asarray(resident, dtype=bool)]
    if np.any((seen > 200) & (seen < 400)):                                 # :83-85
        T = T - tk0
    S = vinterp(zsal, sal, zm)                                              # :99-100
    Sref = (S[0] + S[-1]) / 2.                                              # :104-105
    SSref = Sref.copy()                                                     # :106
    X2 = S - Sref[None, :]                                                  # :107-109
    Tref = T[0].copy()                                                      # :112
    Ssurf = SSref.copy() if l_ssref else X2[0] + Sref                       # :113-117
    return dict(U=U, V=V, U_init=U.copy(), V_init=V.copy(), T=T, X2=X2, Sref=Sref, SSref=SSref, Tref=Tref, Ssurf=Ssurf)


def axes(zm):
    """The caller axes of the tests against the model levels zm(1:nzp1), the smallest that reach every branch:
      two        n = 2, spanning the column and a little more: every model level brackets in the one pair
      coarse7    7 levels that start below zm(1) and end above zm(nzp1): several model levels take each clamp, several
                 share a bracket
      fine130    130 levels, finer than the model: kin skips entries between two model levels; more than two 64-level
                 tiles of caller levels
      equal      contains zm(1), zm(nzp1) and two interior zm(k) exactly, between others: the three equality cases -
                 a target on the first level (kin = 0, t = 0), on the last (the last pair, evaluated), on an interior one"""
    zm = np.asarray(zm, dtype=np.float64)
    top, bot, n = zm[0], zm[-1], len(zm)
    span = top - bot
    out = {
        "two": np.array([top + 0.25 * (zm[0] - zm[1]), bot - 0.25 * (zm[0] - zm[1])]),
        "coarse7": top - span * np.array([0.11, 0.19, 0.3, 0.52, 0.61, 0.8, 0.93]),
        "fine130": top + 1.0 - (span + 2.0) * (np.arange(130) / 129.0) ** 1.5,
        "equal": np.array([top, 0.5 * (zm[1] + zm[2]), zm[n // 3], 0.3 * zm[n // 2] + 0.7 * zm[n // 2 + 1], zm[(2 * n) // 3],
                           0.5 * (zm[-3] + zm[-2]), bot]),
    }
    for z in out.values():
        assert np.isfinite(z).all() and (np.diff(z) < 0).all()
    return out
