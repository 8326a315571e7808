"""The caller's vertical axes on the device (include/mckpp_hip_vaxis.h: mckpp_hip_vaxis_define, _put_dev, _put_host,
_init_profiles_dev, _init_profiles_host, _fetch_dev and their multi_ twins; k_vaxis_put_planes, k_vaxis_init_finish,
k_vaxis_fetch_planes).

The yardstick is tests/vaxis_ref.py, the numpy restatement of the reference's vertical interpolation and of its initial
profiles.  A put on a caller's axis is compared with the restatement's values handed to the existing put_host on model
levels, on a second context; the initial profiles with the restatement applied on the host and uploaded; a fetch with
the restatement applied to window_fetch(field, 3) of the same context.  Every comparison is an equality of bits; no test
has a tolerance.

Axes: the four of vaxis_ref.axes - two levels, seven coarse ones inside the column, 130 fine ones around it, and one
that holds model levels exactly.  Cases: every_step_nz40 (30 resident of 40 points), sweep_nd3 (more than 256 columns,
tails in both paths) and deep_nz100_nd4 (two level tiles), as tests/test_put_gpu.py.  Two shards are two contexts on
the one device, as everywhere in this suite."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ref_loop_cases as lc
import variant_cases as vc
import vaxis_ref as vr
from harness import assert_same, flux_args, force_bench, initialised, loop_state, mk, resident  # noqa: F401
from test_device_arrays_gpu import _bits, _dev, _intervals, _state
from test_put_gpu import FIELD_AT, WRITTEN, _case, _written
from test_restart_schedule_gpu import _same_bytes

pytestmark = pytest.mark.gpu

LAND = 1e20
SKIP = -999.0
TK0 = 273.15
AXES = ("two", "coarse7", "fine130", "equal")
AXIS_NO = {name: i for i, name in enumerate(AXES)}
AMPLITUDE = {"u": 1e-4, "v": 1e-4, "T": 1e-3, "S_anom": 1e-4, "S": 1e-4}   # small: the run stays on its path


def _define(h, kc):
    """the four axes on the handle; {name: heights}"""
    ax = vr.axes(kc.zm)
    for name, z in ax.items():
        h.vaxis_define(AXIS_NO[name], z)
    return ax


def _to_axis(zm, prof, z):
    """a model profile (npts, nzp1) brought to the heights z - by numpy's interpolation, any would do: inputs only"""
    return np.ascontiguousarray(np.stack([np.interp(-z, -zm, p) for p in prof], axis=1))


# ---------------------------------------------------------------------------
# 1. state in: a put on a caller's axis is the restatement's values through put_host
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class Spec:
    """One put: the planes as (field, axis name), the call's keywords, the element type, the form"""
    tag: str
    planes: tuple
    op: str = "add"
    dtype: type = np.float64
    time_levels: bool = False
    skip: bool = False
    ssref: int = 1
    way: str = "dev"

    def arrays(self, k3, ax):
        """(field, axis name, array (n, npts)): the increment amplitude * sin(point + height / 20), on top of the field as
        it stands - brought to the axis - where the operation is a set; with skip, every third point holds the skip value
        at one input level only, the middle one"""
        zm, out = ax["zm"], []
        for i, (name, axis) in enumerate(self.planes):
            z = ax[axis]
            v = AMPLITUDE[name] * np.sin(np.arange(k3.npts)[None, :] + z[:, None] / 20.0 + i + 0.5)
            if self.op == "set":
                a, l = FIELD_AT[name]
                now = getattr(k3, a)[:, :, l] + (k3.Sref[:, None] if name == "S" else 0.0)
                v = _to_axis(zm, now, z) + v
            v = np.ascontiguousarray(v.astype(self.dtype))
            if self.skip:
                assert not (v == SKIP).any()
                v[len(z) // 2, 1::3] = SKIP
            out.append((name, axis, v))
        return out

    def kw(self):
        return dict(op=self.op, time_levels=self.time_levels, skip=SKIP if self.skip else None)


SPECS = {
    "add_f64": Spec("every_step_nz40", (("T", "coarse7"), ("u", "two"), ("S_anom", "equal"))),
    "set_f32_S_time_levels": Spec("every_step_nz40", (("S", "fine130"), ("v", "coarse7"), ("T", "equal")), op="set",
                                  dtype=np.float32, time_levels=True, ssref=0),
    "add_f32_S_skip_time_levels_host": Spec("sweep_nd3", (("u", "coarse7"), ("T", "equal"), ("S", "fine130")), dtype=np.float32,
                                            time_levels=True, skip=True, ssref=0, way="host"),
    "set_f64_skip": Spec("sweep_nd3", (("T", "fine130"), ("S", "coarse7"), ("v", "two")), op="set", skip=True),
    "deep_add_skip_time_levels": Spec("deep_nz100_nd4", (("T", "fine130"), ("S_anom", "coarse7"), ("v", "equal")), skip=True,
                                      time_levels=True),
    "deep_set_f32_time_levels_host": Spec("deep_nz100_nd4", (("T", "coarse7"), ("S_anom", "equal"), ("u", "fine130"), ("v", "two")),
                                          op="set", dtype=np.float32, time_levels=True, way="host"),
}


def test_the_specs_cover_what_the_kernel_can_be_asked():
    s = SPECS.values()
    assert {x.op for x in s} == {"set", "add"} and {x.dtype for x in s} == {np.float64, np.float32}
    assert {x.way for x in s} == {"dev", "host"} and {x.tag for x in s} == {"every_step_nz40", "sweep_nd3", "deep_nz100_nd4"}
    assert any(x.time_levels for x in s) and any(not x.time_levels for x in s)
    assert any(x.skip and x.op == "set" for x in s) and any(x.skip and x.op == "add" for x in s)
    planes = [(x, p) for x in s for p in x.planes]
    assert {p[1] for _, p in planes} == set(AXES)
    assert any(p[0] == "S" and x.op == "set" and not x.ssref for x, p in planes)     # minus Sref, Ssurf restated
    assert any(p[0] == "S" and x.op == "add" for x, p in planes) and any(p[0] == "S" and x.ssref for x, p in planes)
    assert any(p[0] == "S_anom" and x.op == "set" for x, p in planes)


def _same_put(mk, spec, shards=0):
    """Context a takes the put on the caller's axes (`shards` > 0: a multi handle), context b the restatement's values
    through put_host on model levels: the sixteen written arrays right after the put, and the whole state after three
    further steps.  With skip, the model levels left alone are exactly those whose branch reads the skipped input level."""
    case = _case(spec.tag, spec.ssref)
    rec, args, active = lc.flux_records(case), flux_args(case), lc.active_columns(case)
    a, kca, k3a = resident(mk, case, shards)
    b, kcb, k3b = resident(mk, case)
    ax = _define(a, kca)
    ax["zm"] = np.array(kca.zm[:case.nz + 1])
    both = ((a, kca, k3a), (b, kcb, k3b))
    intervals = list(_intervals(case))

    def advance(r, nt, n):
        for h, _, _ in both:
            h.fluxes(nt, *rec[r], **args)
            h.step(nt, n)

    advance(*intervals[0])
    before = _state(b, k3b, kcb, case.nz)
    assert_same(_state(a, k3a, kca, case.nz), before, active, f"{spec.tag}: before the put")
    arrays = spec.arrays(k3b, ax)
    if spec.way == "dev":
        a.vaxis_put_dev([(f, AXIS_NO[axis], _dev(v)) for f, axis, v in arrays], **spec.kw())
    else:
        a.vaxis_put_host([(f, AXIS_NO[axis], v) for f, axis, v in arrays], **spec.kw())
    model = []
    for f, axis, v in arrays:
        w = vr.vinterp(ax[axis], v, ax["zm"])
        if spec.skip:
            left = vr.untouched(ax[axis], v, ax["zm"], SKIP)
            reads = [len(ax[axis]) // 2 in lv for lv in vr.levels_read(ax[axis], ax["zm"])]
            assert np.array_equal(left, np.outer(reads, np.arange(case.ncol) % 3 == 1)) and left.any() and not (w == SKIP).any()
            w[left] = SKIP
        model.append((f, np.ascontiguousarray(w), 0))
    b.put_host(model, **spec.kw())
    got, want = _written(a, k3a, kca, case.nz), _written(b, k3b, kcb, case.nz)
    assert_same(got, want, active, f"{spec.tag}: right after the put")
    assert any(not np.array_equal(got[k][active], before[k][active]) for k in WRITTEN), "the put changed nothing"
    if spec.skip:   # ... seen on the state itself: exactly the levels that read the skipped input level stay
        for (f, axis, v), (_, w, _) in zip(arrays, model):
            name = {"u": "U", "v": "V", "T": "T", "S_anom": "S", "S": "S"}[f]
            stayed = _bits(got[name][active]) == _bits(before[name][active])
            assert np.array_equal(stayed, (w == SKIP).T[active]), (spec.tag, f, axis)
    steps = 0
    for r, nt, n in intervals[1:]:
        if steps >= 3:
            break
        advance(r, nt, n)
        steps += n
    assert steps >= 3
    end = _state(b, k3b, kcb, case.nz)
    assert_same(_state(a, k3a, kca, case.nz), end, active, f"{spec.tag}: {steps} steps after the put")
    assert np.isfinite(end["T"][active]).all()
    a.close()
    b.close()


@pytest.mark.parametrize("name", sorted(SPECS))
def test_a_put_on_a_callers_axis_is_the_restatement_through_put_host(mk, name):
    _same_put(mk, SPECS[name])


# ---------------------------------------------------------------------------
# 2. the reference's initial profiles
# ---------------------------------------------------------------------------
RESTART = ("U", "X", "Us", "Xs", "hmixd", "hmix", "kmix", "Tref", "uref", "vref", "Ssurf", "old", "new_", "reset_flag")
ZEROED = ("U", "X", "U_init", "Sref", "SSref", "Tref", "Ssurf")


def _profile_inputs(kc, k3, ax, axes3, dtype):
    """u, v, temp, sal on the three axes, from the model profiles k3 holds"""
    zm = np.array(kc.zm[:kc.nzp1])
    vel, temp, sal = (ax[n] for n in axes3)
    return dict(u=_to_axis(zm, k3.U[:, :, 0], vel).astype(dtype), v=_to_axis(zm, k3.U[:, :, 1], vel).astype(dtype),
                temp=_to_axis(zm, k3.X[:, :, 0], temp).astype(dtype),
                sal=_to_axis(zm, k3.X[:, :, 1] + k3.Sref[:, None], sal).astype(dtype))


def _init_both(mk, kc, k3, inp, axes3, way, tmp_path, shards=0, nsteps=3, forcing=None):
    """Context a: upload with zeroed profiles and references, vaxis_init_profiles, init_ocean, steps.  Context b: the
    restatement applied on the host, upload, init_ocean, steps.  The restart sets - as downloaded, and as the files of
    save_restart, which hold U_init, Sref and SSref too (one context) - are equal after the initialisation and after
    the steps.  Returns the restatement and the two downloaded states."""
    ocean = k3.run_physics != 0
    active = np.nonzero(ocean)[0]
    zm = np.array(kc.zm[:kc.nzp1])
    k3a, k3b = copy.deepcopy(k3), copy.deepcopy(k3)
    for n in ZEROED:
        getattr(k3a, n)[...] = 0.0
    a = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    ax = _define(a, kc)
    a.upload(k3a)
    no = [AXIS_NO[n] for n in axes3]
    if way == "dev":
        a.vaxis_init_profiles_dev(*[_dev(inp[n]) for n in ("u", "v", "temp", "sal")], *no, tk0=TK0)
    else:
        a.vaxis_init_profiles_host(*[inp[n] for n in ("u", "v", "temp", "sal")], *no, tk0=TK0)
    a.init_ocean(0)
    ref = vr.init_profiles(zm, inp["u"], inp["v"], inp["temp"], inp["sal"], *[ax[n] for n in axes3], TK0, kc.L_SSref, resident=ocean)
    k3b.U[:, :, 0], k3b.U[:, :, 1] = ref["U"].T, ref["V"].T
    k3b.U_init[...] = k3b.U
    k3b.X[:, :, 0], k3b.X[:, :, 1] = ref["T"].T, ref["X2"].T
    k3b.Sref[:], k3b.SSref[:], k3b.Tref[:], k3b.Ssurf[:] = ref["Sref"], ref["SSref"], ref["Tref"], ref["Ssurf"]
    b = initialised(mk, kc, k3b)

    def compare(what):
        for h, k in ((a, k3a), (b, k3b)):
            h.synchronize()
            h.download(k)
        for n in RESTART:
            assert np.array_equal(getattr(k3a, n)[active], getattr(k3b, n)[active], equal_nan=True), (what, n)
        assert np.array_equal(a.status()[0][active], b.status()[0][active]), what
        if not shards:
            a.save_restart(tmp_path / "a")
            b.save_restart(tmp_path / "b")
            _same_bytes(tmp_path / "a", tmp_path / "b", what)

    compare("after the initialisation")
    assert np.array_equal(_bits(k3a.X[active, :, 0]), _bits(ref["T"].T[active])) and np.array_equal(k3a.Tref[active], ref["T"][0, active])
    for nt in range(1, nsteps + 1):
        for h, k in ((a, k3a), (b, k3b)):
            if forcing is None:
                force_bench(h, k)
            else:
                h.fluxes(nt, *forcing[nt - 1])
            h.step(nt, 1)
        compare(f"after step {nt}")
    a.close()
    b.close()
    return ref, k3a, k3b


@pytest.mark.parametrize("tag,axes3,dtype,way,ssref", [
    ("every_step_nz40", ("coarse7", "fine130", "equal"), np.float64, "dev", 1),
    ("every_step_nz40", ("equal", "two", "coarse7"), np.float32, "host", 0),
    ("sweep_nd3", ("fine130", "equal", "two"), np.float32, "dev", 0),
    ("deep_nz100_nd4", ("two", "coarse7", "fine130"), np.float64, "host", 1),
])
def test_init_profiles_is_the_restatement_uploaded(mk, tmp_path, tag, axes3, dtype, way, ssref):
    case = _case(tag, ssref)
    kc, k3 = lc.hip_raw(case)
    inp = _profile_inputs(kc, k3, vr.axes(kc.zm), axes3, dtype)
    ref, k3a, _ = _init_both(mk, kc, k3, inp, axes3, way, tmp_path)
    ocean = k3.run_physics != 0
    assert not np.any((ref["T"][:, ocean] > 200) & (ref["T"][:, ocean] < 400)), "no column in Kelvin: nothing subtracted"
    assert np.isfinite(k3a.X[ocean]).all() and (k3a.hmix[ocean] > 0).all()


KELVIN = ("none", "one_column", "exactly_200_and_400", "land_only")


@pytest.mark.parametrize("what", KELVIN)
def test_the_kelvin_rule(mk, tmp_path, what):
    """temp on the axis that starts on zm(1): T(1) of a column is its first input value, exactly."""
    case = lc.CASES["every_step_nz40"]
    kc, k3 = lc.hip_raw(case)
    ocean = k3.run_physics != 0
    axes3 = ("coarse7", "equal", "fine130")
    inp = _profile_inputs(kc, k3, vr.axes(kc.zm), axes3, np.float64)
    sea, land = np.nonzero(ocean)[0], np.nonzero(~ocean)[0]
    if what == "one_column":
        inp["temp"][:, sea[7]] += TK0
    elif what == "exactly_200_and_400":
        inp["temp"][0, sea[3]], inp["temp"][0, sea[11]] = 200.0, 400.0
    elif what == "land_only":
        inp["temp"][:, land[2]] += TK0
    plain = vr.init_profiles(np.array(kc.zm[:kc.nzp1]), inp["u"], inp["v"], inp["temp"], inp["sal"],
                             *[vr.axes(kc.zm)[n] for n in axes3], 0.0, kc.L_SSref)     # (tk0 = 0: T as interpolated)
    ref, k3a, _ = _init_both(mk, kc, k3, inp, axes3, "dev", tmp_path, nsteps=3 if what in ("none", "land_only") else 0)
    subtracted = what == "one_column"
    want = plain["T"] - TK0 if subtracted else plain["T"]
    assert np.array_equal(_bits(ref["T"][:, ocean]), _bits(want[:, ocean]))
    if what == "exactly_200_and_400":
        T = plain["T"][:, ocean]
        assert (T == 200.0).sum() == 1 and (T == 400.0).sum() == 1 and not np.any((T > 200) & (T < 400))
    if what == "land_only":   # the documented difference: the reference's ANY runs over the land points too
        everywhere = vr.init_profiles(np.array(kc.zm[:kc.nzp1]), inp["u"], inp["v"], inp["temp"], inp["sal"],
                                      *[vr.axes(kc.zm)[n] for n in axes3], TK0, kc.L_SSref, resident=None)
        assert np.array_equal(everywhere["T"], plain["T"] - TK0) and not np.array_equal(everywhere["T"][:, ocean], ref["T"][:, ocean])


def test_u_init_reaches_check_profile(mk, tmp_path):
    """The relaxed switch set of tests/variant_cases.py with its column mix: the columns with 50 m/s in their top levels
    are trapped in the first step and check_profile puts their currents back to U_init - which here only
    vaxis_init_profiles has written (the upload held zeros)."""
    nz, ncol = 40, 96
    _, _, land, kc, k3 = vc.start("relaxed", 0, nz, "uniform", 3600.0, ncol, hip=True)
    axes3 = ("fine130", "fine130", "equal")
    inp = _profile_inputs(kc, k3, vr.axes(kc.zm), axes3, np.float64)
    ref, k3a, k3b = _init_both(mk, kc, k3, inp, axes3, "dev", tmp_path, nsteps=1)
    trapped = np.setdiff1d(vc.regime_columns(ncol)["trap_u"], land)
    assert len(trapped) and (np.abs(k3a.reset_flag[trapped]) == 999).all(), "no column was reset"
    assert np.array_equal(_bits(k3a.U[trapped, :, 0]), _bits(ref["U_init"].T[trapped])) and np.abs(ref["U_init"][:, trapped]).max() > 40
    assert np.array_equal(_bits(k3a.U[trapped, :, 1]), _bits(ref["V_init"].T[trapped]))


# ---------------------------------------------------------------------------
# 3. fields out
# ---------------------------------------------------------------------------
FETCHED = ("T", "S", "u", "rho", "dbloc")


@pytest.fixture(scope="module")
def stepped(mk):
    """the three cases after their first flux interval, the four axes defined; and per case window_fetch(field, 3) of
    the fetched fields, computed once"""
    made = {}

    def get(tag):
        if tag not in made:
            case = lc.CASES[tag]
            h, kc, k3 = resident(mk, case)
            ax = _define(h, kc)
            h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
            h.step(1, case.ndtocn)
            model = {}
            for f in FETCHED:
                out = np.full((case.ncol, case.nz + 1), LAND, order="F")
                h.window_fetch(mk.api._win_field(f), mk.api.OP_INSTANT, out)
                model[f] = np.ascontiguousarray(out.T)
                model[f].flags.writeable = False
            made[tag] = (h, kc, k3, case, ax, model)
        return made[tag]

    yield get
    for m in made.values():
        m[0].close()


@pytest.mark.parametrize("fill_land", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tag", ["every_step_nz40", "sweep_nd3", "deep_nz100_nd4"])
def test_fetch_is_the_restatement_of_window_fetch(mk, stepped, tag, dtype, fill_land):
    """Twenty planes in one launch: five fields on four axes.  A float plane is numpy.float32 of the double plane;
    without fill_land the land points keep the bytes the array held."""
    import torch

    h, kc, k3, case, ax, model = stepped(tag)
    zm, ocean = np.array(kc.zm[:case.nz + 1]), lc.ocean(case).astype(bool)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    planes = [(f, axis) for f in FETCHED for axis in AXES]
    outs = [torch.full((len(ax[axis]), case.ncol), -7.0, dtype=tdt, device="cuda") for _, axis in planes]
    h.vaxis_fetch_dev([(f, AXIS_NO[axis], o) for (f, axis), o in zip(planes, outs)], land_value=LAND, fill_land=fill_land)
    for (f, axis), o in zip(planes, outs):
        want = vr.vinterp(zm, model[f], ax[axis])
        want[:, ~ocean] = LAND if fill_land else -7.0
        got = o.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want.astype(dtype))), (tag, f, axis, dtype.__name__, fill_land)
        assert case.land_every == 0 or np.all(got[:, ~ocean] == (dtype(LAND) if fill_land else -7.0))


def test_the_round_trip_is_both_maps_and_not_the_identity(mk, stepped):
    """T out onto the axis that holds model levels, and set back from it: the restatement of the one map applied to the
    restatement of the other.  Levels between the caller's come back changed."""
    import torch

    tag = "every_step_nz40"
    case = lc.CASES[tag]
    h, kc, k3 = resident(mk, case)
    ax = _define(h, kc)
    h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    h.step(1, 1)
    zm, z, active = np.array(kc.zm[:case.nz + 1]), ax["equal"], lc.active_columns(case)
    h.download(k3)
    T0 = k3.X[:, :, 0].copy()
    t = torch.empty((len(z), case.ncol), dtype=torch.float64, device="cuda")
    h.vaxis_fetch_dev([("T", AXIS_NO["equal"], t)], land_value=LAND)
    h.vaxis_put_dev([("T", AXIS_NO["equal"], t)], op="set", fence=True)
    h.synchronize()
    h.download(k3)
    want = vr.vinterp(z, vr.vinterp(zm, T0.T, z), zm).T
    assert np.array_equal(_bits(k3.X[active, :, 0]), _bits(want[active]))
    assert np.array_equal(k3.Tref[active], want[active, 0])
    assert not np.array_equal(want[active], T0[active]), "the round trip is not the identity"
    h.close()


# ---------------------------------------------------------------------------
# 4. refusals, before anything is queued
# ---------------------------------------------------------------------------
def _short_of(torch, need_bytes):
    """(tensor, address, bytes): an address in device memory with 8 bytes fewer than need_bytes from it to the end of its
    allocation - the tail of the block that torch's allocator got from the runtime and the tensor, which keeps it
    alive, lies in.  Whatever else the block holds: a refused call reads and writes nothing."""
    big = torch.zeros(12 << 17, dtype=torch.float64, device="cuda")   # 12 MiB
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= big.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1 and seg[0]["total_size"] > need_bytes
    return big, seg[0]["address"] + seg[0]["total_size"] - (need_bytes - 8), need_bytes - 8


def test_every_refusal_by_name_leaves_everything_as_it_was(mk):
    import torch

    A, E = mk.api, mk.MckppHipError
    case = lc.CASES["every_step_nz40"]
    npts, nzp1 = case.ncol, case.nz + 1
    h, kc, k3 = resident(mk, case)
    h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    h.step(1, 1)
    ax = _define(h, kc)
    n7 = len(ax["coarse7"])
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()

    def everything():
        s = _state(h, k3, kc, case.nz)
        return {k: _bits(np.nan_to_num(v.astype(np.float64))).copy() for k, v in s.items()}

    before = everything()
    # axes
    z = (A._dp._type_ * 3)
    for n, values, text in ((3, (0.0, -5.0, -2.0), "axis 6: z[2]=-2 is not below z[1]=-5"), (2, (0.0, 0.0, 0.0), "is not below"),
                            (1, (0.0, 0.0, 0.0), "axis 6: n=1 levels (2..1024, or 0 to drop the axis)"),
                            (1025, (0.0, 0.0, 0.0), "n=1025 levels"), (-2, (0.0, 0.0, 0.0), "n=-2 levels"),
                            (2, (0.0, float("nan"), 0.0), "z[1] is not finite"), (2, (float("inf"), 0.0, 0.0), "z[0] is not finite")):
        assert lib.mckpp_hip_vaxis_define(h._h, 6, n, z(*values)) < 0 and err().startswith("mckpp_hip_vaxis_define: ") and text in err(), err()
    assert lib.mckpp_hip_vaxis_define(h._h, 6, 3, None) < 0 and "axis 6: z is null" in err()
    assert lib.mckpp_hip_vaxis_define(h._h, 8, 2, z(0.0, -1.0, -2.0)) < 0 and "axis 8 (0..7)" in err()
    assert lib.mckpp_hip_vaxis_define(h._h, -1, 2, z(0.0, -1.0, -2.0)) < 0 and "axis -1 (0..7)" in err()
    with pytest.raises(ValueError, match="does not strictly decrease"):
        h.vaxis_define(6, [0.0, -5.0, -2.0])
    good = torch.zeros((n7, npts), dtype=torch.float64, device="cuda")
    pinned = torch.zeros(npts * n7, dtype=torch.float64).pin_memory()
    pageable = np.zeros(npts * n7)
    big, small, holds = _short_of(torch, npts * 130 * 8)
    P, O, R = A._VaxisPutPlaneC, A._VaxisDevPlaneC, A._VaxisProfilesC
    c7 = AXIS_NO["coarse7"]
    ok = dict(field=A.OUT["T"], axis=c7, dtype=A.EXP_F64, op=A.PUT_ADD, flags=0, skip_value=0.0)
    forms = {"mckpp_hip_vaxis_put_dev": lambda n, tab: lib.mckpp_hip_vaxis_put_dev(h._h, n, tab, None),
             "mckpp_hip_vaxis_put_host": lambda n, tab: lib.mckpp_hip_vaxis_put_host(h._h, n, tab)}
    ptr = {"mckpp_hip_vaxis_put_dev": good.data_ptr(), "mckpp_hip_vaxis_put_host": pageable.ctypes.data}

    def refused(text, k=0, only=None, first=None, **swap):
        """plane k of a table of k + 1 is the bad one; `first` changes the good planes before it"""
        for name, call in forms.items():
            if only and name != only:
                continue
            base = P(**{**ok, **(first or {})}, **{"in": ptr[name]})
            bad = P(**{**{**ok, "in": ptr[name]}, **swap})
            tab = (P * (k + 1))(*([base] * k + [bad]))
            assert call(k + 1, tab) < 0, (name, text)
            assert err().startswith(name + ": ") and f"planes[{k}]" in err() and text in err(), err()

    refused("axis 6 is not defined", axis=6)                    # (the refused definitions left it undefined)
    refused("axis 9 is not defined", axis=9)
    refused("axis -1 is not defined", k=1, first=dict(field=A.OUT["u"]), axis=-1)
    refused("unknown output field 99", field=99)
    refused("field 4 is an output of the step, not state", field=A.OUT["hmix"])
    refused("field 16 is an output of the step, not state", k=1, first=dict(field=A.OUT["u"]), field=A.OUT["rho"])
    refused("dtype 7 (MCKPP_EXP_F64 1, MCKPP_EXP_F32 2)", dtype=7)
    refused("op 2 (MCKPP_PUT_SET 0, MCKPP_PUT_ADD 1)", op=2)
    refused("flags 0x4", flags=4)
    refused("the skip value is NaN", flags=A.PUT_SKIP, skip_value=float("nan"))
    refused("planes[1] and planes[0] write the same field (2, 2)", k=1, axis=AXIS_NO["two"])
    refused("planes[1] and planes[0] write the same field (5, 3)", k=1, first=dict(field=A.OUT["S_anom"]), field=A.OUT["S"])
    dev, host = "mckpp_hip_vaxis_put_dev", "mckpp_hip_vaxis_put_host"
    refused("planes[0].in is pinned host memory", only=dev, **{"in": pinned.data_ptr()})
    refused("planes[1].in is host memory", only=dev, k=1, first=dict(field=A.OUT["u"]), **{"in": pageable.ctypes.data})
    refused("planes[0].in is null", only=dev, **{"in": None})
    # a buffer that does for a shorter axis, and for the model's levels, but not for this axis
    fine = AXIS_NO["fine130"]
    assert holds > npts * nzp1 * 8 > npts * n7 * 8
    refused(f"planes[0].in: the allocation holds {holds} bytes from the pointer on, the call needs {npts * 130 * 8}", only=dev,
            axis=fine, **{"in": small})
    refused("planes[0].in is null", only=host, **{"in": None})
    tab = (P * 65)(*[P(**ok, **{"in": good.data_ptr()})] * 65)
    for name, call in forms.items():
        assert call(65, tab) < 0 and f"{name}: nplanes=65 (0..64)" in err()
        assert call(1, None) < 0 and f"{name}: nplanes=1 (0..64) or a null table" in err()
        assert call(0, None) == 0 and call(0, tab) == 0
    # fields out
    out = torch.full((n7, npts), -7.0, dtype=torch.float64, device="cuda")
    okf = dict(field=A.OUT["T"], axis=c7, dtype=A.EXP_F64, fill_land=1, land_value=LAND, out=out.data_ptr())

    def fetch_refused(text, k=0, **swap):
        tab = (O * (k + 1))(*([O(**okf)] * k + [O(**{**okf, **swap})]))
        assert lib.mckpp_hip_vaxis_fetch_dev(h._h, k + 1, tab, None) < 0
        assert err().startswith("mckpp_hip_vaxis_fetch_dev: ") and f"planes[{k}]" in err() and text in err(), err()

    fetch_refused("field 9 (wT) lives on the interface axis", field=A.OUT["wT"])
    fetch_refused("field 13 (difm) lives on the interface axis", k=1, field=A.OUT["difm"])
    fetch_refused("field 4 (hmix) is two-dimensional", field=A.OUT["hmix"])
    fetch_refused("field 28 is two-dimensional", field=A.OUT["solar_in"])
    fetch_refused("unknown output field 99", field=99)
    fetch_refused("axis 6 is not defined", axis=6)
    fetch_refused("dtype 0", dtype=0)
    fetch_refused("planes[0].out is pinned host memory", out=pinned.data_ptr())
    fetch_refused("planes[1].out is host memory", k=1, out=pageable.ctypes.data)
    fetch_refused(f"the allocation holds {holds} bytes from the pointer on, the call needs {npts * 130 * 8}", axis=fine, out=small)
    assert np.array_equal(out.cpu().numpy(), np.full((n7, npts), -7.0)), "a refused delivery wrote"
    with pytest.raises(ValueError, match="field wu lives on the interface axis"):
        h.vaxis_fetch_dev([("wu", c7, out)])
    with pytest.raises(ValueError, match="field hmix is two-dimensional"):
        h.vaxis_fetch_dev([("hmix", c7, out)])
    # the profiles
    okr = dict(axis_vel=c7, axis_temp=c7, axis_sal=c7, dtype=A.EXP_F64, tk0=TK0, u=good.data_ptr(), v=good.data_ptr(),
               temp=good.data_ptr(), sal=good.data_ptr())
    for swap, text in ((dict(axis_temp=6), "temp: axis 6 is not defined"), (dict(dtype=3), "dtype 3"),
                       (dict(tk0=float("inf")), "tk0 is not finite"), (dict(sal=pinned.data_ptr()), "sal is pinned host memory"),
                       (dict(v=None), "v is null"), (dict(axis_vel=fine, u=small), f"u: the allocation holds {holds} bytes")):
        assert lib.mckpp_hip_vaxis_init_profiles_dev(h._h, C.byref(R(**{**okr, **swap})), None) < 0
        assert err().startswith("mckpp_hip_vaxis_init_profiles_dev: ") and text in err(), err()
    assert lib.mckpp_hip_vaxis_init_profiles_host(h._h, C.byref(R(**{**okr, "temp": None}))) < 0 and "temp is null" in err()
    assert lib.mckpp_hip_vaxis_init_profiles_dev(h._h, None, None) < 0 and "null argument" in err()
    # a context without a state
    fresh = mk.MckppHip(kc)
    fresh.vaxis_define(c7, ax["coarse7"])
    one = (P * 1)(P(**ok, **{"in": good.data_ptr()}))
    assert lib.mckpp_hip_vaxis_put_dev(fresh._h, 1, one, None) < 0 and err() == "mckpp_hip_vaxis_put_dev: upload the state first"
    assert lib.mckpp_hip_vaxis_fetch_dev(fresh._h, 1, (O * 1)(O(**okf)), None) < 0 and err() == "mckpp_hip_vaxis_fetch_dev: upload the state first"
    assert lib.mckpp_hip_vaxis_init_profiles_dev(fresh._h, C.byref(R(**okr)), None) < 0 and "upload the state first" in err()
    fresh.close()
    # a multi handle checks every plane of every shard before any shard queues
    m, kcm, k3m = resident(mk, case, shards=2)
    _define(m, kcm)
    m_before = {k: v.copy() for k, v in _state(m, k3m, kcm, case.nz).items()}
    tab2 = (P * 2)(P(**ok, **{"in": good.data_ptr()}), P(**{**ok, "field": A.OUT["u"], "in": pinned.data_ptr()}))
    assert lib.mckpp_hip_multi_vaxis_put_dev(m._h, 2, tab2, None) < 0
    assert err().startswith("mckpp_hip_multi_vaxis_put_dev: planes[1].in is pinned host memory"), err()
    tab2[1] = P(**{**ok, "axis": AXIS_NO["equal"], "in": pageable.ctypes.data})
    assert lib.mckpp_hip_multi_vaxis_put_host(m._h, 2, tab2) < 0 and "mckpp_hip_multi_vaxis_put_host: planes[1] and planes[0]" in err()
    assert_same(_state(m, k3m, kcm, case.nz), m_before, slice(None), "the shards after the refusals")
    m.close()
    # the library's texts through the Python layer, where it has no check of its own to be first
    with pytest.raises(ValueError, match="a host array"):
        h.vaxis_put_dev([("T", c7, pinned)])
    after = everything()
    assert after.keys() == before.keys() and all(np.array_equal(after[k], before[k]) for k in before), "a refusal touched the state"
    assert not good.cpu().numpy().any()
    # ... and the run goes on: the axes are as they were defined, a good put and the next launch
    h.vaxis_put_dev([("T", c7, good)], op="add")
    h.fluxes(2, *lc.flux_records(case)[1], **flux_args(case))
    h.step(2, 1)
    again = everything()
    assert not np.array_equal(again["T"], before["T"])
    h.close()


# ---------------------------------------------------------------------------
# 5. both handles: two shards on the one device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["add_f32_S_skip_time_levels_host", "set_f64_skip", "deep_add_skip_time_levels"])
def test_two_shards_take_the_same_put(mk, name):
    _same_put(mk, SPECS[name], shards=2)


def test_two_shards_init_profiles_with_the_kelvin_flag_of_shard_1_alone(mk, tmp_path):
    """The profiles through a multi handle are the restatement uploaded to one context, through three steps.  Then one
    column of shard 1 holds Kelvin: every column of both shards loses tk0, as on one context."""
    case = lc.CASES["sweep_nd3"]
    kc, k3 = lc.hip_raw(case)
    axes3 = ("coarse7", "equal", "fine130")
    inp = _profile_inputs(kc, k3, vr.axes(kc.zm), axes3, np.float64)
    _init_both(mk, kc, k3, inp, axes3, "host", tmp_path, shards=2)
    mask0, n0 = mk.api.host_shard_mask(k3.run_physics, 2, 0)
    mask1, n1 = mk.api.host_shard_mask(k3.run_physics, 2, 1)
    assert n0 and n1 and not (mask0 & mask1).any()
    col = np.nonzero(mask1)[0][5]
    inp["temp"][:, col] += TK0
    ref, k3a, _ = _init_both(mk, kc, k3, inp, axes3, "dev", tmp_path, shards=2, nsteps=0)
    plain = vr.init_profiles(np.array(kc.zm[:kc.nzp1]), inp["u"], inp["v"], inp["temp"], inp["sal"],
                             *[vr.axes(kc.zm)[n] for n in axes3], 0.0, kc.L_SSref)
    ocean = k3.run_physics != 0
    assert np.array_equal(_bits(ref["T"][:, ocean]), _bits((plain["T"] - TK0)[:, ocean]))
    in0 = np.nonzero(mask0)[0]
    assert np.array_equal(_bits(k3a.Tref[in0]), _bits((plain["T"][0] - TK0)[in0])), "shard 0 did not see shard 1's flag"


def test_two_shards_fetch(mk, stepped):
    """The planes of a multi handle are those of the single context bit for bit; shard 0 fills the points no shard holds."""
    import torch

    one, kc, k3, case, ax, model = stepped("sweep_nd3")
    m, kcm, k3m = resident(mk, case, shards=2)
    _define(m, kcm)
    m.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
    m.step(1, case.ndtocn)
    npts, ocean = case.ncol, lc.ocean(case).astype(bool)
    planes = [("T", "fine130"), ("S", "coarse7"), ("u", "equal"), ("rho", "two")]
    for dtype, fill in [(torch.float64, True), (torch.float32, True), (torch.float64, False)]:
        outs = {}
        for name, h in (("one", one), ("multi", m)):
            outs[name] = [torch.full((len(ax[axis]), npts), -7.0, dtype=dtype, device="cuda") for _, axis in planes]
            h.vaxis_fetch_dev([(f, AXIS_NO[axis], o) for (f, axis), o in zip(planes, outs[name])], land_value=LAND, fill_land=fill)
        for p, a, b in zip(planes, outs["one"], outs["multi"]):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(_bits(a), _bits(b)), (p, dtype, fill)
            assert np.all(b[:, ~ocean] == (a.dtype.type(LAND) if fill else -7.0)), (p, dtype, fill, "land points")
            assert not np.any(b[:, ocean] == a.dtype.type(LAND)) and not np.any(b[:, ocean] == -7.0), (p, "ocean points")
    m.close()
