"""The caller's horizontal grids (include/mckpp_hip_hgrid.h) on the device: forcing in from arrays on a caller's grid - at
once (mckpp_hip_hgrid_fluxes_dev) and into the flux ring (mckpp_hip_hgrid_flux_ring_put_dev) - and fields out onto it
(mckpp_hip_hgrid_fetch_dev).

Every value comparison is an equality of bits: the header states the order of the sums and every operation is rounded
once.  The yardsticks: tests/golden/ref_loop.npz, the compiled reference's time loop, for identity-like tables; for
general tables tests/hgrid_ref.py's numpy restatement of the header - remapped arrays through the existing
mckpp_hip_fluxes_dev / mckpp_hip_flux_ring_put_dev in, and applied to mckpp_hip_window_fetch(field, 3) out.  The cases:
sweep_nd3 (more than 256 resident columns, a block tail) and every_step_nz40 (land), each with the two grids of
hgrid_ref.grids - 37 points, fewer than a wave, and about 1.3 npts, no multiple of 64 - and rows of 0, 1, 4, 9 and 70
entries (tests/test_hgrid_cpu.py holds the tables to what they are built for).  Inputs hold no NaN."""
import ctypes as C

import numpy as np
import pytest

import hgrid_ref as hr
import ref_loop_cases as lc
from harness import assert_loop_step, assert_same, flux_args, loop_state, mk, resident  # noqa: F401
from harness import loop_golden as golden  # noqa: F401
from test_device_arrays_gpu import _assert_golden, _bits, _dev, _state
from test_vaxis_gpu import _short_of

pytestmark = pytest.mark.gpu

TAGS = ("every_step_nz40", "sweep_nd3")
LAND = hr.LAND
PER_CALL = 2


def _tables(case):
    """per grid (n, in table, out table): the general tables of the case"""
    ocean = lc.ocean(case)
    return [(n, hr.general_in(case.ncol, n, ocean, 7 + g), hr.general_out(n, case.ncol, ocean, 17 + g))
            for g, n in enumerate(hr.grids(case.ncol))]


def _define_general(h, case):
    tabs = _tables(case)
    for g, (n, tin, tout) in enumerate(tabs):
        h.hgrid_define(g, n, tin, tout)
    return tabs


def _caller_records(case, n, seed):
    """flux records on a caller grid of n points: the case's own value ranges, no NaN"""
    rng = np.random.default_rng(seed)
    rec = lc.flux_records(case)
    return np.ascontiguousarray(rec[:, :, rng.integers(0, case.ncol, size=n)])


def _remapped(table, rec, npts):
    """[8, npts]: record rec[8, n] through an in table, by the restatement"""
    return np.stack([hr.apply(table, rec[m], npts) for m in range(8)])


def _ring_run(h, case, nslots, put, after_call, nrec=None):
    n, nd = lc.nrec(case) if nrec is None else nrec, case.ndtocn
    for r0 in range(0, n, PER_CALL):
        count = min(PER_CALL, n - r0)
        for r in range(r0, r0 + count):
            put(r)
        assert h.flux_ring_records() == (max(0, r0 + count - nslots), r0 + count - 1)
        nt0, nt1 = r0 * nd + 1, min((r0 + count) * nd, case.nsteps)
        h.run_forced(nt0, nt1 - nt0 + 1, nd, **flux_args(case))
        after_call(nt1)


# ---------------------------------------------------------------------------
# 1. forcing in through an identity-like table: the golden record, step for step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_golden_cases_through_the_ring_from_a_permuted_caller_grid(mk, golden, tag):
    case = lc.CASES[tag]
    n = hr.grids(case.ncol)[1]
    table, perm = hr.identity_in(case.ncol, n, 31)
    recd = _dev(hr.through(perm, n, lc.flux_records(case)))
    h, kc, k3 = resident(mk, case)
    h.hgrid_define(2, n, table)
    h.flux_ring(3)
    _ring_run(h, case, 3, lambda r: h.hgrid_flux_ring_put_dev(2, r, recd[r]),
              lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, "remapped puts through a permutation"))
    h.close()


def test_host_device_and_remapped_puts_alternate_in_one_ring(mk, golden):
    tag = "sweep_nd3"
    case = lc.CASES[tag]
    n = hr.grids(case.ncol)[1]
    table, perm = hr.identity_in(case.ncol, n, 32)
    rec = lc.flux_records(case)
    recd, recc = _dev(rec), _dev(hr.through(perm, n, rec))
    h, kc, k3 = resident(mk, case)
    h.hgrid_define(0, n, table)
    h.flux_ring(2)

    def put(r):
        if r % 3 == 0:
            h.flux_ring_put(r, rec[r])
        elif r % 3 == 1:
            h.hgrid_flux_ring_put_dev(0, r, [recc[r, m] for m in range(8)])
        else:
            h.flux_ring_put_dev(r, recd[r])

    _ring_run(h, case, 2, put, lambda nt: _assert_golden(golden, tag, nt, h, k3, kc, "host, remapped and device puts"))
    h.close()


def test_hgrid_fluxes_dev_waits_for_its_producer_and_the_fence_holds_the_rewrite(mk, golden):
    """The record is produced on a side stream behind a few large fills, hgrid_fluxes_dev follows at once and the tensor
    is overwritten on that stream right after: a library that read too early, or whose fence did not hold, sees other
    values and the golden digests differ.  A race test can only fail, never prove."""
    import torch

    tag = "every_step_nz40"
    case = lc.CASES[tag]
    n = hr.grids(case.ncol)[1]
    table, perm = hr.identity_in(case.ncol, n, 33)
    recc = _dev(hr.through(perm, n, lc.flux_records(case)))
    h, kc, k3 = resident(mk, case)
    h.hgrid_define(1, n, table)
    side = torch.cuda.Stream()
    big = torch.empty((64 << 20) // 8, dtype=torch.float64, device="cuda")
    t = torch.full((8, n), 5e33, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for r in range(lc.nrec(case)):
        nt = r * case.ndtocn + 1
        with torch.cuda.stream(side):
            for i in range(4):
                big.fill_(float(i))
            t.copy_(recc[r])
        h.hgrid_fluxes_dev(1, nt, t, stream=side, fence=True, **flux_args(case))
        with torch.cuda.stream(side):
            t.fill_(5e33)
        h.step(nt, min(case.ndtocn, case.nsteps - nt + 1))
    _assert_golden(golden, tag, case.nsteps, h, k3, kc, "produced on a side stream, rewritten behind the fence")
    h.close()


# ---------------------------------------------------------------------------
# 2. forcing in through the general tables: the restatement's arrays through the existing calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 2])
@pytest.mark.parametrize("tag", TAGS)
def test_general_tables_in_are_the_restatement_through_fluxes_dev(mk, tag, shards):
    """a: the restatement's remapped arrays through fluxes_dev; b (shards: a multi handle): hgrid_fluxes_dev.  Two
    intervals per grid, the state compared after each."""
    case = lc.CASES[tag]
    args, active = flux_args(case), lc.active_columns(case)
    a, kca, k3a = resident(mk, case)
    b, kcb, k3b = resident(mk, case, shards)
    tabs = _define_general(b, case)
    nt = 1
    for g, (n, tin, _) in enumerate(tabs):
        rec = _caller_records(case, n, 40 + g)
        recd = _dev(rec)
        for r in range(2):
            a.fluxes_dev(nt, _dev(_remapped(tin, rec[r], case.ncol)), **args)
            a.step(nt, case.ndtocn)
            b.hgrid_fluxes_dev(g, nt, recd[r], **args)
            b.step(nt, case.ndtocn)
            nt += case.ndtocn
            assert_same(_state(b, k3b, kcb, case.nz), _state(a, k3a, kca, case.nz), active, f"{tag} grid {g} after step {nt - 1}")
    a.close()
    b.close()


@pytest.mark.parametrize("shards", [0, 2])
@pytest.mark.parametrize("tag", TAGS)
def test_general_tables_into_the_ring_are_the_restatement_through_ring_put_dev(mk, tag, shards):
    case = lc.CASES[tag]
    active = lc.active_columns(case)
    a, kca, k3a = resident(mk, case)
    b, kcb, k3b = resident(mk, case, shards)
    tabs = _define_general(b, case)
    recs = [_caller_records(case, n, 50 + g) for g, (n, _, _) in enumerate(tabs)]
    recd = [_dev(r) for r in recs]
    a.flux_ring(2)
    b.flux_ring(2)

    def put_a(r):
        g = r % 2
        a.flux_ring_put_dev(r, _dev(_remapped(tabs[g][1], recs[g][r], case.ncol)))

    def compare(nt):
        assert_same(_state(b, k3b, kcb, case.nz), _state(a, k3a, kca, case.nz), active, f"{tag} after step {nt}")

    _ring_run(a, case, 2, put_a, lambda nt: None, nrec=4)
    _ring_run(b, case, 2, lambda r: b.hgrid_flux_ring_put_dev(r % 2, r, recd[r % 2][r]), lambda nt: None, nrec=4)
    compare(4 * case.ndtocn)
    a.close()
    b.close()


def test_a_resident_column_with_an_empty_in_row_is_refused_by_point(mk):
    case = lc.CASES["every_step_nz40"]
    E = mk.MckppHipError
    h, kc, k3 = resident(mk, case)
    n = 37
    ptr, idx, w = hr.general_in(case.ncol, n, lc.ocean(case), 7)
    point = int(lc.active_columns(case)[5])
    rows = [[(int(i), float(v)) for i, v in zip(idx[ptr[p]:ptr[p + 1]], w[ptr[p]:ptr[p + 1]])] for p in range(case.ncol)]
    rows[point] = []
    h.hgrid_define(0, n, hr.csr(rows))
    h.flux_ring(2)
    before = _state(h, k3, kc, case.nz)
    fields = _dev(_caller_records(case, n, 1)[0])
    with pytest.raises(E, match=f"mckpp_hip_hgrid_fluxes_dev: grid 0: the in row of point {point}, a resident column, is empty"):
        h.hgrid_fluxes_dev(0, 1, fields)
    with pytest.raises(E, match=f"mckpp_hip_hgrid_flux_ring_put_dev: grid 0: the in row of point {point}, a resident column"):
        h.hgrid_flux_ring_put_dev(0, 0, fields)
    assert h.flux_ring_records() == (-1, -1)
    assert_same(_state(h, k3, kc, case.nz), before, np.arange(case.ncol), "after the refusals")
    # the same row at a land point is no refusal
    rows[point] = [(0, 1.0)]
    rows[0] = []
    assert lc.ocean(case)[0] == 0
    h.hgrid_define(0, n, hr.csr(rows))
    h.hgrid_fluxes_dev(0, 1, fields)
    h.close()


# ---------------------------------------------------------------------------
# 3. fields out
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped(mk):
    """the cases after their first flux interval, the general tables defined; with the fields as window_fetch gives them"""
    made = {}

    def get(tag, shards=0):
        if (tag, shards) not in made:
            case = lc.CASES[tag]
            h, kc, k3 = resident(mk, case, shards)
            h.fluxes(1, *lc.flux_records(case)[0], **flux_args(case))
            h.step(1, case.ndtocn)
            made[tag, shards] = (h, kc, k3, case, _define_general(h, case))
        return made[tag, shards]

    yield get
    for h, *_ in made.values():
        h.close()


def _model_field(h, A, npts, nzp1, field):
    """(nlev, npts): window_fetch(field, OP_INSTANT)"""
    f = A._win_field(field)
    out = np.zeros((npts,) if f in A._OUT_2D else (npts, nzp1), order="F")
    h.window_fetch(f, A.OP_INSTANT, out)
    return np.ascontiguousarray(out.reshape(npts, -1).T)


PLANES = (("T", 0, 1), ("T", 0, None), ("S", 0, None), ("hmix", 0, 1), ("S", 3, 5))   # (field, lev0, nlev; None: the whole axis)


def _fetch_and_compare(h, A, case, tabs, ocean, dtype, norm, fill, what, model=None):
    import torch

    npts, nzp1 = case.ncol, case.nz + 1
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    model = model or h
    planes, outs, wants = [], [], []
    for g, (n, _, tout) in enumerate(tabs):
        for k, (field, lev0, nlev) in enumerate(PLANES):
            nlev = nlev or nzp1
            held = np.random.default_rng(100 * g + k).uniform(-3.0, 3.0, (nlev, n)).astype(dtype)
            o = _dev(held)
            x = _model_field(model, A, npts, nzp1, field)[lev0:lev0 + nlev]
            want = np.stack([hr.apply(tout, x[j], n, ocean, norm, fill, LAND, held[j].astype(np.float64)) for j in range(nlev)])
            planes.append((field, g, o, lev0, nlev))
            outs.append(o)
            wants.append(want.astype(dtype))
    h.hgrid_fetch_dev(planes, norm=norm, land_value=LAND, fill_land=fill)
    for p, o, want in zip(planes, outs, wants):
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), (what, p[0], p[1], p[3], p[4], dtype.__name__, norm, fill)
    return wants


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "keep"])
@pytest.mark.parametrize("norm", hr.NORMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tag", TAGS)
def test_fields_out_are_the_restatement_of_window_fetch(mk, stepped, tag, dtype, norm, fill):
    h, kc, k3, case, tabs = stepped(tag)
    wants = _fetch_and_compare(h, mk.api, case, tabs, lc.ocean(case), dtype, norm, fill, tag)
    # what the tables are built for shows in the results: row 2 is land only, row 4's used weights sum to 0.0
    for g in range(2):
        t0 = wants[g * len(PLANES)][0]
        if fill:
            assert t0[0] == dtype(LAND) and t0[2] == dtype(LAND) and (t0[4] == dtype(LAND)) == (norm == "used")
        assert t0[3] != dtype(LAND) and abs(t0[5]) < 50.0


def test_norm_none_differs_from_used_where_a_row_has_land_entries(mk, stepped):
    import torch

    h, kc, k3, case, tabs = stepped("every_step_nz40")
    n = tabs[1][0]
    a, b = (torch.zeros((1, n), dtype=torch.float64, device="cuda") for _ in range(2))
    h.hgrid_fetch_dev([("T", 1, a, 0, 1)], norm="none")
    h.hgrid_fetch_dev([("T", 1, b, 0, 1)], norm="used")
    a, b = a.cpu().numpy()[0], b.cpu().numpy()[0]
    assert a[3] != b[3] and a[3] != LAND and b[3] != LAND and a[2] == LAND == b[2]


def test_hgrid_info_is_the_host_layout_of_the_resident_state(mk, stepped):
    A = mk.api
    for tag in TAGS:
        h, kc, k3, case, tabs = stepped(tag)
        ocean, rows = lc.ocean(case), lc.active_columns(case)
        for g, (n, tin, tout) in enumerate(tabs):
            info = h.hgrid_info(g)
            pin = len(A.host_hgrid_slices(tin, case.ncol, rows=rows)[2])
            pout = len(A.host_hgrid_slices(tout, n, keep=ocean)[2])
            assert info == dict(n=n, nnz_in=int(tin[0][-1]), nnz_out=int(tout[0][-1]), padded_in=pin, padded_out=pout, longest_row=70)


def test_the_grid_stays_after_an_upload_with_another_column_map(mk):
    """More land under the same grid: the tables stay, the device tables follow the new residency - out sums leave the
    new land points out, in sums are formed for the new columns."""
    A = mk.api
    case = lc.CASES["every_step_nz40"]
    h, kc, k3 = resident(mk, case)
    tabs = _define_general(h, case)
    ocean = lc.ocean(case)
    _fetch_and_compare(h, A, case, tabs, ocean, np.float64, "used", True, "first map")
    before = h.hgrid_info(1)
    k3.run_physics[2::6] = 0
    k3.l_ocean[2::6] = 0
    ocean2 = np.array(k3.run_physics != 0, dtype=np.int32)
    assert ocean2.sum() < ocean.sum()
    h.upload(k3)
    h.init_ocean(0)
    assert h.hgrid_info(1)["n"] == before["n"] and h.hgrid_info(1)["padded_in"] <= before["padded_in"]
    _fetch_and_compare(h, A, case, tabs, ocean2, np.float64, "used", True, "second map")
    _fetch_and_compare(h, A, case, tabs, ocean2, np.float32, "none", False, "second map")
    # ... and forcing in: against a context that was given the second map from the start
    b = mk.MckppHip(kc)
    b.upload(k3)
    b.init_ocean(0)
    n, tin, _ = tabs[0]
    rec = _caller_records(case, n, 3)[0]
    h.hgrid_fluxes_dev(0, 1, _dev(rec), **flux_args(case))
    b.fluxes_dev(1, _dev(_remapped(tin, rec, case.ncol)), **flux_args(case))
    h.step(1, 1)
    b.step(1, 1)
    assert_same(_state(h, k3, kc, case.nz), _state(b, k3, kc, case.nz), np.nonzero(ocean2)[0], "after the second upload")
    h.close()
    b.close()


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------
def test_every_refusal_by_name_leaves_everything_as_it_was(mk, stepped):
    import torch

    A, E = mk.api, mk.MckppHipError
    h, kc, k3, case, tabs = stepped("every_step_nz40")
    npts, nzp1 = case.ncol, case.nz + 1
    n = tabs[1][0]
    h.hgrid_define(2, n, tabs[1][1], None)      # no out table
    h.hgrid_define(3, n, None, tabs[1][2])      # no in table
    lib, err = A._lib(), lambda: A._lib().mckpp_hip_last_error().decode()
    before = _state(h, k3, kc, case.nz)
    good = torch.zeros((8, n), dtype=torch.float64, device="cuda")
    out = torch.full((nzp1, n), -5.0, dtype=torch.float64, device="cuda")
    pageable = np.zeros(8 * n)
    big, small, holds = _short_of(torch, n * 8)      # an address with room for n - 1 doubles
    P = A._HgridPlaneC
    ok = dict(field=A.OUT["T"], lev0=0, nlev=nzp1, dtype=A.EXP_F64, grid=1, norm=0, fill_land=1, land_value=LAND, out=out.data_ptr())

    def fields(base, last=None):
        return (C.c_void_p * 8)(*[base + 8 * n * m if last is None or m < 7 else last for m in range(8)])

    def fetch(*planes):
        return lib.mckpp_hip_hgrid_fetch_dev(h._h, len(planes), (P * len(planes))(*[P(**{**ok, **p}) for p in planes]), None)

    table = [   # (call, message fragment)
        (lambda: lib.mckpp_hip_hgrid_fluxes_dev(h._h, 5, 1, fields(good.data_ptr()), 0, 1.0, 1.0, None),
         "mckpp_hip_hgrid_fluxes_dev: grid: grid 5 is not defined"),
        (lambda: lib.mckpp_hip_hgrid_flux_ring_put_dev(h._h, 3, 0, fields(good.data_ptr()), None),
         "mckpp_hip_hgrid_flux_ring_put_dev: no flux ring is set"),
        (lambda: lib.mckpp_hip_hgrid_fluxes_dev(h._h, 3, 1, fields(good.data_ptr()), 0, 1.0, 1.0, None),
         "mckpp_hip_hgrid_fluxes_dev: grid 3 has no in table"),
        (lambda: lib.mckpp_hip_hgrid_fluxes_dev(h._h, 1, 1, fields(pageable.ctypes.data), 0, 1.0, 1.0, None),
         "mckpp_hip_hgrid_fluxes_dev: fields[0] (taux) is host memory"),
        (lambda: lib.mckpp_hip_hgrid_fluxes_dev(h._h, 1, 1, fields(good.data_ptr(), small), 0, 1.0, 1.0, None),
         f"mckpp_hip_hgrid_fluxes_dev: fields[7] (snow): the allocation holds {holds} bytes from the pointer on, the call needs {8 * n}"),
        (lambda: lib.mckpp_hip_hgrid_fluxes_dev(h._h, 1, 1, None, 0, 1.0, 1.0, None), "mckpp_hip_hgrid_fluxes_dev: null argument"),
        (lambda: fetch(dict(grid=-1)), "mckpp_hip_hgrid_fetch_dev: planes[0]: grid -1 is not defined"),
        (lambda: fetch({}, dict(grid=2)), "mckpp_hip_hgrid_fetch_dev: planes[1]: grid 2 has no out table"),
        (lambda: fetch(dict(out=pageable.ctypes.data, nlev=1)), "mckpp_hip_hgrid_fetch_dev: planes[0].out is host memory"),
        (lambda: fetch(dict(out=None)), "mckpp_hip_hgrid_fetch_dev: planes[0].out is null"),
        (lambda: fetch(dict(out=small, nlev=1)),
         f"mckpp_hip_hgrid_fetch_dev: planes[0].out: the allocation holds {holds} bytes from the pointer on, the call needs {8 * n}"),
        (lambda: fetch(dict(nlev=2), dict(out=out.data_ptr() + 8 * n, nlev=1, field=A.OUT["S"])),
         "mckpp_hip_hgrid_fetch_dev: planes[1].out and planes[0].out overlap"),
        (lambda: fetch(dict(norm=2)), "mckpp_hip_hgrid_fetch_dev: planes[0]: norm 2 (MCKPP_HGRID_NORM_NONE 0, MCKPP_HGRID_NORM_USED 1)"),
        (lambda: fetch(dict(dtype=7)), "mckpp_hip_hgrid_fetch_dev: planes[0]: dtype 7"),
        (lambda: fetch(dict(field=99)), "field 99"),
        (lambda: fetch(dict(lev0=nzp1 - 1, nlev=2)), "mckpp_hip_hgrid_fetch_dev: planes[0]: lev0="),
        (lambda: lib.mckpp_hip_hgrid_fetch_dev(h._h, 65, (P * 65)(), None), "mckpp_hip_hgrid_fetch_dev: nplanes=65 (0..64)"),
        (lambda: lib.mckpp_hip_hgrid_info(h._h, 1, None), "mckpp_hip_hgrid_info: null argument"),
        (lambda: lib.mckpp_hip_hgrid_define(h._h, 4, 5, None, None), "mckpp_hip_hgrid_define: grid 4 (0..3)"),
        (lambda: lib.mckpp_hip_hgrid_define(h._h, 0, -1, None, None), "mckpp_hip_hgrid_define: grid 0: n=-1"),
    ]
    for call, text in table:
        assert call() < 0, text
        assert text in err(), (text, err())
    # a refused define leaves the grid in place; its message names table, row and entry
    ptr, idx, w = (a.copy() for a in tabs[1][2])
    w[ptr[3] + 1] = float("inf")
    with pytest.raises(E, match=r"mckpp_hip_hgrid_define: table out: row 3: entry \d+: the weight is not finite"):
        h.hgrid_define(1, n, tabs[1][1], (ptr, idx, w))
    idx2 = tabs[1][1][1].copy()
    idx2[0] = n
    with pytest.raises(E, match=rf"mckpp_hip_hgrid_define: table in: row 0: entry 0: index {n} is outside 0\.\.{n - 1}"):
        h.hgrid_define(1, n, (tabs[1][1][0], idx2, tabs[1][1][2]), tabs[1][2])
    assert h.hgrid_info(1)["nnz_out"] == int(tabs[1][2][0][-1])
    assert (out.cpu().numpy() == -5.0).all(), "a refused call wrote into the caller's array"
    assert_same(_state(h, k3, kc, case.nz), before, np.arange(npts), "after the refusals")
    _fetch_and_compare(h, A, case, tabs, lc.ocean(case), np.float64, "used", True, "after the refusals")
    # a grid defined before a state of another size is refused by name when used
    h.hgrid_define(2, 0)
    h.hgrid_define(3, 0)
    fresh = mk.MckppHip(kc)
    with pytest.raises(ValueError, match="upload the state first"):
        fresh.hgrid_define(0, n, tabs[1][1])
    assert lib.mckpp_hip_hgrid_define(fresh._h, 0, n, None, None) < 0 and "upload the state first" in err()
    fresh.close()


# ---------------------------------------------------------------------------
# 5. two shards on the one device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_two_shards_deliver_the_single_contexts_bits(mk, stepped, tag):
    """the planes of a multi handle of two shards against the restatement applied to the single context's fields - the
    yardstick the single context's own planes are held to - with the union of the shards' columns as residency"""
    A = mk.api
    h, kc, k3, case, tabs = stepped(tag)
    m, kcm, k3m, _, _ = stepped(tag, 2)
    assert m.hgrid_info(1)["padded_out"] == h.hgrid_info(1)["padded_out"]
    for dtype, norm, fill in ((np.float64, "used", True), (np.float32, "none", False), (np.float64, "none", True)):
        _fetch_and_compare(m, A, case, tabs, lc.ocean(case), dtype, norm, fill, f"{tag}, two shards", model=h)
    mask0, n0 = A.host_shard_mask(k3m.run_physics, 2, 0)
    assert 0 < n0 < len(lc.active_columns(case)), "both shards hold columns"
