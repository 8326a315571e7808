"""How far down a pass forms the bulk Richardson numbers of bldepth is a guess: in a column's first pass of a step
the level its boundary layer ended at in its previous step (kmix in the column's record) plus MCKPP_FIRST_MARGIN,
in later passes the level the scan of the pass before ended at plus MCKPP_GUESS_MARGIN.  A guess that is too
shallow costs a second round of the scan and nothing else, so every case here asks the same thing: every field,
status word and pass count equal, bit for bit, to the CPU oracle (portable exp) and to a run under
MCKPP_FIRST_GUESS=0 (every level in a first pass, the scan's end plus eight after it).

The switches are read when a context is created, so each run sets them first and makes its own context."""
import numpy as np
import pytest

import common as cm
from harness import mk  # noqa: F401

pytestmark = pytest.mark.gpu

ALL_FIELDS = cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["hmixd0", "hmixd1"] + list(cm.DIAG_FIELDS.keys())
RAW_FIELDS = ("U", "X", "Us", "Xs", "hmixd", "hmix", "kmix", "Tref", "uref", "vref", "Ssurf", "old", "new_", "rho", "cp", "buoy",
              "difm", "difs", "dift", "ghat", "wU", "wX", "wXNT", "Rig", "dbloc", "Shsq")
SWITCHES = ("MCKPP_FIRST_GUESS", "MCKPP_FIRST_MARGIN", "MCKPP_GUESS_MARGIN", "MCKPP_L3_CAP", "MCKPP_PS_FIXED_L", "MCKPP_MULTISTEP",
            "MCKPP_SOLO_AFTER", "MCKPP_SOLO_LIMIT")
OLD_RULES = {"MCKPP_FIRST_GUESS": "0"}
# the library's default first margin (mckpp_runtime.cpp: FIRST_MARGIN_DEFAULT), set explicitly where a reach condition
# is stated in terms of it
FIRST_MARGIN = 12


def _bench(ncol):
    return cm.synth.forcing(ncol, "bench")


def _class(ncol, cls):
    """every column in class `cls` of synth.forcing's bench mix (0 heating and calm, 1 cooling, 2 storm), or in the
    classes of the array `cls`"""
    return cm.synth.forcing(ncol, "bench", index=np.broadcast_to(np.asarray(cls), (ncol,)))


_ORACLE = {}


def _oracle(key, ncol, nz, plan, solver=0, switches=None, prep=None):
    """The oracle's run of `plan` = [(forcing, nsteps), ...], one step at a time, computed once per `key` and left
    alone: (const, batch after the last step, per-step status, pass counts and kmix)."""
    if key not in _ORACLE:
        from oracle import orc

        oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, solver_mode=solver, **(switches or {}))
        if prep is not None:
            kc, k3 = cm.make_hip_case(ncol, nz)
            prep(k3, ob)
        orc.init_ocean(oc, ob, 0)
        st, npass, kmix, nt = [], [], [np.array(ob["kmix"]).copy()], 0
        for sf, n in plan:
            ob["sflux"] = sf
            for _ in range(n):
                nt += 1
                orc.physics_driver(oc, ob, nt)
                st.append(np.array(ob["status"]).copy()); npass.append(np.array(ob["npasses"]).copy())
                kmix.append(np.array(ob["kmix"]).copy())
        _ORACLE[key] = (oc, ob, st, npass, kmix)
    return _ORACLE[key]


def _gpu(mk, monkeypatch, env, ncol, nz, plan, one_launch=True, solver=0, switches=None, prep=None, reupload=None):
    """The device's run of `plan` in a context of its own made under `env`: a launch per entry of the plan, or a launch
    per step.  reupload = (after_step, kmix or None): the state is downloaded after that step and uploaded again, with
    `kmix` in place of the record's own if given.  Returns the fields and the status words and pass counts of every launch."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kc, k3 = cm.make_hip_case(ncol, nz)
    for k, v in (switches or {}).items():
        setattr(kc, k, v)
    if prep is not None:
        prep(k3, None)
    ctx = mk.MckppHip(kc)
    ctx.set_solver_mode(solver)
    ctx.upload(k3)
    ctx.init_ocean(0)
    nt, stat = 0, {}
    for sf, n in plan:
        cm.set_forcing_3d(k3, sf)
        ctx.set_forcing(k3.sflux)
        for first, count in ([(nt + 1, n)] if one_launch else [(nt + 1 + i, 1) for i in range(n)]):
            if reupload is not None and first - 1 < reupload[0] < first - 1 + count:
                raise AssertionError("a re-upload inside a launch")
            ctx.step(first, count)
            st, nf, npass = ctx.status()
            stat[first + count - 1] = (st.copy(), npass.copy())
            if reupload is not None and reupload[0] == first + count - 1:
                ctx.download(k3)
                if reupload[1] is not None:
                    k3.kmix[:] = reupload[1]
                ctx.upload(k3)
                ctx.set_forcing(k3.sflux)
        nt += n
    ctx.download(k3)
    ctx.close()
    return k3, stat


def _same_as_oracle(k3, stat, orc_run, nz, tag, fields=ALL_FIELDS):
    oc, ob, st, npass, kmix = orc_run
    for step, (s, n) in stat.items():   # (status and pass counts describe the last step of a launch)
        assert np.array_equal(s, st[step - 1]), f"{tag}: status words after step {step}"
        assert np.array_equal(n, npass[step - 1]), f"{tag}: pass counts after step {step}"
    bad = {k: v for k, v in cm.compare(k3, ob, nz, fields).items() if v[2] != 0}
    assert not bad, f"{tag}: fields differing from the oracle (max_abs, max_rel, n_values): {bad}"


def _same_as_run(a, b, tag):
    (k3a, sa), (k3b, sb) = a, b
    assert sa.keys() == sb.keys()
    for step in sa:
        assert np.array_equal(sa[step][0], sb[step][0]) and np.array_equal(sa[step][1], sb[step][1]), f"{tag}: step {step}"
    for name in RAW_FIELDS:
        assert np.array_equal(np.asarray(getattr(k3a, name)), np.asarray(getattr(k3b, name)), equal_nan=True), f"{tag}: {name}"


def _check(mk, monkeypatch, env, key, ncol, nz, plan, tag, fields=ALL_FIELDS, **kw):
    """the run under `env` against the oracle and against the run under the rules before the guesses"""
    new = _gpu(mk, monkeypatch, env, ncol, nz, plan, **kw)
    okw = {k: kw[k] for k in ("solver", "switches", "prep") if k in kw}
    orc_run = _oracle(key, ncol, nz, plan, **okw)
    _same_as_oracle(new[0], new[1], orc_run, nz, tag, fields)
    old_env = dict({k: v for k, v in env.items() if k not in ("MCKPP_FIRST_MARGIN", "MCKPP_GUESS_MARGIN", "MCKPP_L3_CAP")}, **OLD_RULES)
    old = _gpu(mk, monkeypatch, old_env, ncol, nz, plan, **kw)
    _same_as_run(new, old, tag + " against MCKPP_FIRST_GUESS=0")
    return new, orc_run


@pytest.mark.parametrize("nz", [40, 60])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("one_launch", [True, False])
def test_plain_run(mk, monkeypatch, nz, solver, one_launch):
    """256 columns of the bench mix, six steps from the analytic start (its second step has columns at itermax; from the
    third on the first pass of every column works from its previous step's kmix), as one launch and as a launch per
    step, in both solver modes."""
    ncol = 256
    _check(mk, monkeypatch, {}, ("plain", nz, solver), ncol, nz, [(_bench(ncol), 6)], f"nz={nz} solver={solver} one_launch={one_launch}",
           one_launch=one_launch, solver=solver)


@pytest.mark.parametrize("nz", [40, 60])
def test_plain_run_level_count_at_run_time(mk, monkeypatch, nz):
    """the same with the kernels that take the level count as an argument (MCKPP_PS_FIXED_L=0)"""
    ncol = 256
    _check(mk, monkeypatch, {"MCKPP_PS_FIXED_L": "0"}, ("plain", nz, 0), ncol, nz, [(_bench(ncol), 6)], f"nz={nz} MCKPP_PS_FIXED_L=0")


@pytest.mark.parametrize("nz,first_margin,one_launch", [(509, FIRST_MARGIN, True), (300, 4, True), (300, 4, False)])
def test_layer_deepening_faster_than_any_margin(mk, monkeypatch, nz, first_margin, one_launch):
    """Four steps under the calm, heating class of synth.forcing, then four with every column in the cooling or the
    storm class: at the switch the boundary layer deepens by more levels than the first guess and the scan's own
    overrun allow for, so the first pass of that step takes the second round.  Levels of 0.4 m (509) make that true
    of the library's own first margin; at 300 levels it is set to 4.
    Reach condition, on the oracle's kmix: nine columns in ten deepen by more than first_margin + 8 levels from step
    4 to step 5 (the oracle alone: all of them, by 30 levels of 509 and by 18 of 300)."""
    ncol = 24
    plan = [(_class(ncol, 0), 4), (_class(ncol, 1 + np.arange(ncol) % 2), 4)]
    env = {"MCKPP_FIRST_MARGIN": str(first_margin)}
    new, orc_run = _check(mk, monkeypatch, env, ("deepening", nz), ncol, nz, plan, f"nz={nz} first_margin={first_margin}", one_launch=one_launch)
    kmix = orc_run[4]
    deeper = (kmix[5] - kmix[4]) > first_margin + 8
    assert deeper.mean() >= 0.9, f"only {deeper.mean():.2f} of the columns deepen by more than {first_margin + 8} levels: nothing tested"


@pytest.mark.parametrize("nz", [40, 60])
@pytest.mark.parametrize("cap", [None, "3"])
def test_worst_case_margins(mk, monkeypatch, nz, cap):
    """No margin at all: the first pass goes down to the previous step's kmix and the later ones to where the scan
    ended, so whenever a boundary layer deepens at all the second round runs; with MCKPP_L3_CAP=3 on top it runs in
    every pass of every column deeper than three levels."""
    ncol = 256
    env = {"MCKPP_GUESS_MARGIN": "0", "MCKPP_FIRST_MARGIN": "0"}
    if cap:
        env["MCKPP_L3_CAP"] = cap
    new, orc_run = _check(mk, monkeypatch, env, ("plain", nz, 0), ncol, nz, [(_bench(ncol), 6)], f"nz={nz} no margins, cap {cap}")
    assert np.any(np.asarray(new[0].kmix) > 3), "no column deeper than the cap: nothing tested"


def test_out_of_range_kmix_in_an_uploaded_record(mk, monkeypatch):
    """kmix of an uploaded record is whatever the host holds: 0, negative, beyond the grid, NaN, 1e300 (and, on every
    sixth column, the true value) must cost time only.  Three steps, download, upload with kmix overwritten, three
    more: equal to the oracle, and to the same run with the record's own kmix uploaded."""
    ncol, nz = 256, 60
    bad = np.array([0.0, -3.0, nz + 7.0, np.nan, 1e300])
    plan = [(_bench(ncol), 3), (_bench(ncol), 3)]

    def overwritten(kmix_true):
        v = np.array(kmix_true, dtype=np.float64).copy()
        for i, b in enumerate(bad):
            v[i::6] = b
        return v

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    true = _gpu(mk, monkeypatch, {}, ncol, nz, plan, reupload=(3, None))
    kmix3 = _oracle(("plain", nz, 0), ncol, nz, [(_bench(ncol), 6)])[4][3]
    new = _gpu(mk, monkeypatch, {}, ncol, nz, plan, reupload=(3, overwritten(kmix3)))
    _same_as_run(new, true, "overwritten kmix against the record's own")
    orc_run = _oracle(("plain", nz, 0), ncol, nz, [(_bench(ncol), 6)])
    _same_as_oracle(new[0], {6: new[1][6]}, orc_run, nz, "overwritten kmix")
    old = _gpu(mk, monkeypatch, OLD_RULES, ncol, nz, plan, reupload=(3, overwritten(kmix3)))
    _same_as_run(new, old, "overwritten kmix against MCKPP_FIRST_GUESS=0")


def test_fewer_columns_than_slots(mk, monkeypatch):
    """64 columns, twelve steps in one launch: workgroups whose slots are in different steps and passes, columns that
    go on where they are - a workgroup's guess is the deepest of what its slots need."""
    ncol, nz = 64, 40
    _check(mk, monkeypatch, {}, ("few", nz), ncol, nz, [(_bench(ncol), 12)], "64 columns, 12 steps in one launch")


@pytest.mark.parametrize("one_launch", [True, False])
def test_forced_views(mk, monkeypatch, one_launch):
    """every column a straggler from its first pass, no limit on their number: the workgroups work in views of a few
    slots throughout, columns start beside others that go on"""
    ncol, nz = 256, 60
    env = {"MCKPP_SOLO_AFTER": "0", "MCKPP_SOLO_LIMIT": "1000000"}
    _check(mk, monkeypatch, env, ("plain", nz, 0), ncol, nz, [(_bench(ncol), 6)], f"forced views, one_launch={one_launch}", one_launch=one_launch)


def _prep_relax_sst(k3, ob):
    n = k3.npts
    r = np.full(n, 1.0 / (5 * 86400.0)); r[::4] = 0.0
    sst = np.asarray(k3.X[:, 0, 0]) + 1.5
    k3.relax_sst[:] = r; k3.SST0[:] = sst
    if ob is not None:
        ob["relax_sst"] = r; ob["SST0"] = sst


def _prep_salt_fingers(k3, ob):
    nzp1 = k3.X.shape[1]
    z = np.linspace(0, 1, nzp1)[None, :]
    S = np.asarray(k3.X[:, :, 1]).copy()
    S[::2] = 0.4 - 0.8 * z
    k3.X[:, :, 1] = S
    if ob is not None:
        ob.a["S"][:, 1:nzp1 + 1] = S


@pytest.mark.parametrize("name,switches,prep", [("relax_sst", dict(L_RELAX_SST=1), _prep_relax_sst),
                                                ("double_diffusion", dict(LDD=1), _prep_salt_fingers)])
def test_optional_physics_kernels(mk, monkeypatch, name, switches, prep):
    """The optional-physics builds of the kernel: SST relaxation, which works from the guesses as the plain kernel
    does, and double diffusion, whose passes form every level whatever the record holds (the second round would
    need rows it has in use)."""
    ncol, nz = 96, 40
    _check(mk, monkeypatch, {}, ("ext", name), ncol, nz, [(_bench(ncol), 4)], name, fields=ALL_FIELDS + cm.EXT_SCALARS,
           switches=switches, prep=prep)
