"""The correspondence between the caller's mckpp_state_ptrs_c and the device-resident state: which slab of which array
is which profile row, which member is which slot of a column record, which group of mckpp_hip_download brings what
back, and in which order the restart file holds it all.  The uploaded arrays hold markers that encode (member, slab,
level, point), so that a wrong slab, slot or offset shows up as a wrong number; no test here runs a step except the one
on the diagnostics' offsets."""
import os
import re

import numpy as np
import pytest

import common as cm
from harness import force_bench, initialised, mk  # noqa: F401

pytestmark = pytest.mark.gpu

NPTS, NZ = 13, 12
LAYOUTS = {"ocean": 0, "land": 3}   # land_every: all ocean downloads its records packed on the device, land points through the host loop
SENTINEL, ISENTINEL = -7777.0, -77

# what mckpp_hip_upload reads; a member's marker number is its place here plus one
UPLOADED = ["U", "X", "Us", "Xs", "U_init", "hmixd", "f", "ocdepth", "Sref", "SSref", "Ssurf", "hmix", "kmix", "Tref",
            "uref", "vref", "reset_flag", "dampu_flag", "dampv_flag", "freeze_flag", "fcorr", "sflux"]
OPTIONAL = UPLOADED[2:] + ["old", "new_", "jerlov", "l_ocean", "l_initflag"]   # everything but U and X may be NULL

# the groups of mckpp_hip_download (include/mckpp_hip.h), the uploaded members of each that come back
GROUPS = {
    "F_PROFILES": ["U", "X"],
    "F_SAVED": ["Us", "Xs", "hmixd", "old", "new_"],
    "F_SCALARS": ["hmix", "kmix", "Tref", "uref", "vref", "Ssurf", "reset_flag", "dampu_flag", "dampv_flag", "freeze_flag",
                  "l_initflag"],   # and sflux(:,1:6,5,0); fcorr only on a context with the optional physics
}
MASKS = ["F_PROFILES", "F_SAVED", "F_SCALARS", "F_DIAG", "F_RESTART", "F_ALL"]
# the diagnostic rows a context without the optional physics holds: before any step they are the zeros of the allocation
DIAG_ROWS = [n for n in cm.DIAG_FIELDS if n not in ("swfrac", "swdk_opt", "tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr")]

# profile row -> (member, slab); record slot -> (member, column of the member as (npts, -1)); unnamed slots hold 0
ROW_OF = {"P_U": ("U", 0), "P_V": ("U", 1), "P_T": ("X", 0), "P_S": ("X", 1),
          "P_US0": ("Us", 0), "P_VS0": ("Us", 1), "P_US1": ("Us", 2), "P_VS1": ("Us", 3),
          "P_TS0": ("Xs", 0), "P_SS0": ("Xs", 1), "P_TS1": ("Xs", 2), "P_SS1": ("Xs", 3),
          "P_UINIT": ("U_init", 0), "P_VINIT": ("U_init", 1)}
CS_OF = {"CS_F": ("f", 0), "CS_SSURF": ("Ssurf", 0), "CS_SREF": ("Sref", 0), "CS_SSREF": ("SSref", 0),
         "CS_OCDEPTH": ("ocdepth", 0), "CS_HMIXD0": ("hmixd", 0), "CS_HMIXD1": ("hmixd", 1), "CS_HMIX": ("hmix", 0),
         "CS_KMIX": ("kmix", 0), "CS_UREF": ("uref", 0), "CS_VREF": ("vref", 0), "CS_TREF": ("Tref", 0),
         "CS_RESET": ("reset_flag", 0), "CS_DAMPU": ("dampu_flag", 0), "CS_DAMPV": ("dampv_flag", 0),
         "CS_FREEZE": ("freeze_flag", 0), "CS_FCORR": ("fcorr", 0)}
CI_OF = {"CI_OLD": "old", "CI_NEW": "new_", "CI_JERLOV": "jerlov", "CI_INITFLAG": "l_initflag", "CI_LOCEAN": "l_ocean"}
DEFAULTS = {"CS_OCDEPTH": -10000.0, "CI_NEW": 1, "CI_JERLOV": 3, "CI_LOCEAN": 1}   # of a NULL member; the others 0

CSRC = os.path.join(cm.ROOT, "mckpp_f90_amd", "csrc")


def _enum(path, first):
    """The enumerators, in order, of the enum of `path` that begins with `first`"""
    src = re.sub(r"//[^\n]*", "", open(path).read())
    body = re.search(r"enum\s*\{\s*(%s\b[^}]*)\}" % first, src).group(1)
    return [w.split("=")[0].strip() for w in body.split(",") if w.strip()]


def _markers(a, member):
    """member * 1e6 + slab * 1e4 + level * 1e2 + point for an array (npts[, levels[, ...]]): the level is its second
    index, the slab the Fortran-order number of the others"""
    npts, nlev = a.shape[0], a.shape[1] if a.ndim > 1 else 1
    p, l, s = np.meshgrid(np.arange(npts), np.arange(nlev), np.arange(a.size // (npts * nlev)), indexing="ij")
    return (member * 1e6 + s * 1e4 + l * 1e2 + p).reshape(a.shape, order="F")


def _arrays(k3):
    return {n: a for n, a in vars(k3).items() if isinstance(a, np.ndarray) and n != "run_physics"}


def _marked(mk, layout, nz=NZ, npts=NPTS):
    kc, k3 = cm.make_hip_case(npts, nz, land_every=LAYOUTS[layout])
    for i, n in enumerate(UPLOADED):
        getattr(k3, n)[...] = _markers(getattr(k3, n), i + 1)
    pt = np.arange(npts)
    k3.old[:], k3.new_[:] = 100 + pt, 200 + pt
    k3.jerlov[:] = 1 + pt % 5
    k3.l_initflag[:] = pt % 2
    k3.l_ocean[:] = 2 * ((pt // 2) % 2)   # a LOGICAL that is true as 2: the record holds 1
    return kc, k3


def _blank(mk, kc, k3):
    """fields of k3's shape with a sentinel in every array"""
    out = mk.Kpp3dFields(k3.npts, kc)
    for a in _arrays(out).values():
        a[...] = ISENTINEL if a.dtype == np.int32 else SENTINEL
    return out


def _without(k3, names):
    """k3 as the library sees it when the members `names` are NULL pointers"""
    def as_c():
        s = type(k3).as_c(k3)
        for n in names:
            setattr(s, n, None)
        return s

    k3.as_c = as_c
    return k3


def _tabs(kc, jerlov):
    """swfrac(:,1:nzp1) and swdk_opt(:,0:nz) of the Jerlov types (swfrac_mod.F90:36-41, fluxes_mod.F90:104-107)"""
    rfac = np.array([0, 0.58, 0.62, 0.67, 0.77, 0.78])[jerlov][:, None]
    a1 = np.array([1, 0.35, 0.6, 1.0, 1.5, 1.4])[jerlov][:, None]
    a2 = np.array([1, 23.0, 20.0, 17.0, 14.0, 7.9])[jerlov][:, None]
    two = lambda z: rfac * np.exp(np.maximum(z / a1, -80.0)) + (1 - rfac) * np.exp(np.maximum(z / a2, -80.0))  # noqa: E731
    return two(kc.zm[None, :]), two(-kc.dm[None, :])


def _expected(mk, kc, k3, mask, tabs):
    """what a download of `mask` into blank fields must leave: the markers of the mask's groups at the resident points,
    the sentinel everywhere else"""
    A = mk.api
    want = _arrays(_blank(mk, kc, k3))
    src = _arrays(k3)
    res = np.nonzero(k3.run_physics)[0]
    for g, members in GROUPS.items():
        if mask & getattr(A, g):
            for n in members:
                want[n][res] = src[n][res]
    if mask & A.F_SCALARS:
        want["sflux"][res, 0:6, 4, 0] = src["sflux"][res, 0:6, 4, 0]
    if mask & A.F_DIAG:
        nz = kc.nz
        for n in DIAG_ROWS:
            arr, comp, lo, cnt = cm.DIAG_FIELDS[n]
            a = want[arr] if comp is None else want[arr][:, :, comp]
            a[res, 0:cnt(nz)] = 0.0
        if tabs:
            want["swfrac"][res], want["swdk_opt"][res] = (t[res] for t in _tabs(kc, k3.jerlov))
    return want


def _assert_download(mk, h, kc, k3, mask_name, tabs, what):
    mask = getattr(mk.api, mask_name)
    got = _blank(mk, kc, k3)
    h.download(got if tabs else _without(got, ["swfrac", "swdk_opt"]), mask)
    want = _expected(mk, kc, k3, mask, tabs)
    for n, a in _arrays(got).items():
        if n in ("swfrac", "swdk_opt"):   # the library's own exponential: what is pinned is the Jerlov slot and the level, and
            # neighbouring levels and types differ by more than a thousandth
            assert np.allclose(a, want[n], rtol=1e-9, atol=0), (what, mask_name, tabs, n)
        else:
            assert np.array_equal(a, want[n]), (what, mask_name, tabs, n, np.argwhere(a != want[n])[:4].tolist())


@pytest.mark.parametrize("shards", [0, 2], ids=["one_context", "two_shards"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_round_trip_by_group(mk, layout, shards):
    """Upload the markers; every group of mckpp_hip_download brings back its own members at the resident points and
    leaves every other array, and the land points, alone.  With swfrac / swdk_opt present an all-ocean context goes
    through the host loop over the records, without them through the records packed on the device."""
    kc, k3 = _marked(mk, layout)
    h = mk.MckppHipMulti(kc, [0] * shards) if shards else mk.MckppHip(kc)
    h.upload(k3)
    for mask_name in MASKS:
        for tabs in ((True, False) if mask_name in ("F_DIAG", "F_ALL") else (True,)):
            _assert_download(mk, h, kc, k3, mask_name, tabs, f"{layout}, {shards} shards")
    h.close()


def _restart_file(path):
    """(header fields, column map, planes [nprof][ncol][ld], cs [ncol][ncs], ci [ncol][nci]) of a restart file"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"MCKPPRS1"
    version, nz, ld, ncs, nci, nprof = (int(v) for v in np.frombuffer(raw, np.int32, 6, 8))
    npts, ncol = (int(v) for v in np.frombuffer(raw, np.int64, 2, 32))
    off = 48
    ipt = np.frombuffer(raw, np.int32, ncol, off); off += 4 * ncol
    planes = np.frombuffer(raw, np.float64, nprof * ncol * ld, off).reshape(nprof, ncol, ld); off += 8 * nprof * ncol * ld
    cs = np.frombuffer(raw, np.float64, ncol * ncs, off).reshape(ncol, ncs); off += 8 * ncol * ncs
    ci = np.frombuffer(raw, np.int32, ncol * nci, off).reshape(ncol, nci); off += 4 * ncol * nci
    assert off == len(raw) and version == 1
    return dict(nz=nz, ld=ld, ncs=ncs, nci=nci, nprof=nprof, npts=npts, ncol=ncol), ipt, planes, cs, ci


@pytest.mark.parametrize("null_optional", [False, True], ids=["all_members", "optional_members_null"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_slot_through_the_restart_file(mk, tmp_path, layout, null_optional):
    """Upload the markers and save_restart: every plane and every record slot of the file, in the order of the P_ / CS_ /
    CI_ enumerations, holds its member's markers - or, of a NULL member, the default.  This is what pins the upload of the
    members no download brings back.  The file loaded into a fresh context and saved again is the same bytes."""
    P = _enum(os.path.join(CSRC, "mckpp_runtime.cpp"), "P_U")
    CS = _enum(os.path.join(CSRC, "mckpp_device.h"), "CS_F")
    CI = _enum(os.path.join(CSRC, "mckpp_device.h"), "CI_OLD")
    assert P[-1] == "P_COUNT" and set(ROW_OF) == set(P[:-1])
    assert set(CS_OF) | {f"CS_SFLUX{m}" for m in range(1, 7)} | {"CS_SPARE1"} == set(CS)
    assert set(CI_OF) | {"CI_STATUS", "CI_NPASS", "CI_IPT"} == set(CI)
    kc, k3 = _marked(mk, layout)
    null = OPTIONAL if null_optional else []
    a = mk.MckppHip(kc)
    a.upload(_without(k3, null))
    a.save_restart(tmp_path / "a")
    hd, ipt, planes, cs, ci = _restart_file(tmp_path / "a")
    res = np.nonzero(k3.run_physics)[0]
    nzp1 = kc.nzp1
    assert hd == dict(nz=NZ, ld=64, ncs=len(CS), nci=len(CI), nprof=len(P) - 1 + 2, npts=NPTS, ncol=len(res))
    assert np.array_equal(ipt, res)
    for i, name in enumerate(P[:-1]):
        member, slab = ROW_OF[name]
        want = 0.0 if member in null else getattr(k3, member).reshape(NPTS, nzp1, -1, order="F")[res, :, slab]
        assert np.array_equal(planes[i, :, :nzp1], np.broadcast_to(want, (len(res), nzp1))), name
    assert not planes[:, :, nzp1:].any() and not planes[len(P) - 1:].any()   # the rows' padding; cp and rho before any step
    for j, name in enumerate(CS):
        if name.startswith("CS_SFLUX"):
            member, col = "sflux", int(name[-1]) - 1 + kc.nsflxs * 4   # sflux(:,m,5,0)
        else:
            member, col = CS_OF.get(name, (None, 0))
        if member is None or member in null:
            want = np.full(len(res), DEFAULTS.get(name, 0.0))
        else:
            want = getattr(k3, member).reshape(NPTS, -1, order="F")[res, col]
        assert np.array_equal(cs[:, j], want), name
    for j, name in enumerate(CI):
        member = CI_OF.get(name)
        if name == "CI_IPT":
            want = res
        elif member is None or member in null:
            want = np.full(len(res), DEFAULTS.get(name, 0))
        else:
            want = getattr(k3, member)[res]
            if name == "CI_LOCEAN":
                want = (want != 0).astype(np.int32)
        assert np.array_equal(ci[:, j], want), name
    a.close()
    b = mk.MckppHip(kc)
    b.load_restart(tmp_path / "a", npts=NPTS)
    b.save_restart(tmp_path / "b")
    b.close()
    assert open(tmp_path / "a", "rb").read() == open(tmp_path / "b", "rb").read()


def _prep_corrections(k3, ob):
    """relaxation and flux corrections with depth (as tests/test_options_gpu.py): all four correction rows are written"""
    n, nzp1 = k3.npts, k3.X.shape[1]
    z = np.arange(nzp1)[None, :]

    def both(name, arr):
        getattr(k3, name)[:, :] = arr
        ob.a[name][:, 1:nzp1 + 1] = arr

    both("ocnT_clim", np.asarray(k3.X[:, :, 0]) - 0.3)
    both("sal_clim", np.asarray(k3.X[:, :, 1]) + 0.05)
    r = np.full(n, 1.0 / (30 * 86400.0))
    k3.relax_ocnT[:] = r; ob["relax_ocnT"] = r
    k3.relax_sal[:] = 2 * r; ob["relax_sal"] = 2 * r
    both("fcorr_withz", 5.0 * np.exp(-z / 10.0) * np.linspace(-1, 1, n)[:, None])
    both("sfcorr_withz", 1e-7 * np.cos(z / 7.0) * np.ones((n, 1)))


@pytest.mark.parametrize("corrections", [False, True], ids=["default_physics", "correction_rows"])
def test_diagnostics_offsets_where_the_two_slab_extents_differ(mk, corrections):
    """The F_DIAG rows after init_ocean and one step under the bench forcing, bit for bit the oracle's.
    tests/test_parity_gpu.py compares all of them too (ALL_FIELDS), but with nztmax + 1 = nzp1 + 1; here the slabs of
    wU / wX are nztmax + 1 = nzp1 + 3 levels apart, so the slab stride and the level count cannot be taken for one
    another."""
    from oracle import orc

    ncol, nz = 28, 12
    sw = dict(L_RELAX_OCNT=1, L_RELAX_SAL=1, L_FCORR_WITHZ=1, L_SFCORR_WITHZ=1) if corrections else {}
    oc, ob, kc0, k30 = cm.make_both(ncol, nz, **sw)
    kc = mk.KppConstFields(nz, nztmax=nz + 3, dto=kc0.dto, zm=kc0.zm, hm=kc0.hm, dm=kc0.dm)
    mk.mckpp_physics_lookup(kc)
    for k in sw:
        setattr(kc, k, sw[k])
    k3 = mk.Kpp3dFields(ncol, kc)
    for n, a in _arrays(k30).items():
        if a.shape == getattr(k3, n).shape:
            getattr(k3, n)[...] = a
    if corrections:
        _prep_corrections(k3, ob)
    h = initialised(mk, kc, k3)
    orc.init_ocean(oc, ob, 0)
    ob["sflux"] = cm.synth.forcing(ncol, "bench")
    force_bench(h, k3)
    h.step(1)
    orc.physics_driver(oc, ob, 1)
    got = _blank(mk, kc, k3)
    h.download(got, mk.api.F_DIAG)
    h.close()
    fields = DIAG_ROWS + (["tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr"] if corrections else [])
    res = cm.compare(got, ob, nz, fields)
    for n in fields:
        print(n, res[n])
    bad = {k: v for k, v in res.items() if v[2] != 0}
    assert not bad, f"fields differing from the oracle (max_abs, max_rel, n_values): {bad}"
    assert np.all(got.wU[:, :, 2] == SENTINEL) and np.all(got.wXNT[:, :, 1] == SENTINEL)   # slabs no row belongs to
    assert np.all(got.wU[:, nz + 1:, :] == SENTINEL) and np.all(got.wX[:, nz + 1:, :] == SENTINEL)
    if corrections:
        assert all(np.any(ob.a[n] != 0) for n in fields[-4:])
    else:
        assert all(np.all(getattr(got, n) == SENTINEL) for n in ("tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr"))
