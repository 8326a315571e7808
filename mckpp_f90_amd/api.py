"""Host-side mirror of the reference's call surface over the C-ABI.

Names follow the reference so a parity test reads like the reference's own
driver (src/mckpp_ocean_model_3D.F90:23-58):

    kpp_const_fields = KppConstFields(nz=60)            # mckpp_initialize_namelist + geography
    mckpp_physics_lookup(kpp_const_fields)              # src/mckpp_physics_lookup_mod.F90:11
    kpp_3d_fields = Kpp3dFields(npts, kpp_const_fields) # mckpp_allocate_3d_fields
    ... fill U, X, f, Sref, sflux ...
    mckpp_initialize_ocean_model(kpp_3d_fields, kpp_const_fields)   # src/mckpp_initialize_ocean.F90:18
    mckpp_physics_driver(kpp_3d_fields, kpp_const_fields, ntime)    # src/mckpp_physics_driver_mod.F90:15

Arrays are numpy arrays in Fortran order with the reference's shapes
(src/mckpp_data_fields.F90:353-447), so `U[ipt, k-1, l-1]` is the reference's
`U(ipt,k,l)`; arrays with a 0 lower bound (rho, cp, difm, wU, ...) are indexed
with the reference index directly.  All compute happens in libmckpp_hip.so.

A new entry point of include/mckpp_hip.h takes two lines here: its signature in _SIGNATURES (twin=True when a
mckpp_hip_multi_ form with the same signature exists) and, for a handle function, one method on _Handle that calls
self._call(name, ...) - MckppHip and MckppHipMulti then both have it.  The device-array interface of
include/mckpp_hip_device.h has a table of its own, _SIGNATURES_DEVICE, and its methods are the mixin _DeviceArrays; so
have the zoomed output schedules of include/mckpp_hip_zoom.h: _SIGNATURES_ZOOM, and their methods are _WindowSchedules'.  The records of a schedule into device arrays
(include/mckpp_hip_device_records.h) are the fourth table, _SIGNATURES_RECORDS, and one more method of _DeviceArrays;
the state set or incremented in place (include/mckpp_hip_put.h) is the fifth, _SIGNATURES_PUT, and two more methods there;
records reduced over levels and points (include/mckpp_hip_reduce.h) are the sixth, _SIGNATURES_REDUCE, and three more;
the caller's vertical axes (include/mckpp_hip_vaxis.h) are the seventh, _SIGNATURES_VAXIS, and the mixin _VerticalAxes;
the caller's horizontal grids (include/mckpp_hip_hgrid.h) are the eighth, _SIGNATURES_HGRID, and the mixin _HorizontalGrids;
records out and state in on those grids (include/mckpp_hip_remap.h) are the ninth, _SIGNATURES_REMAP, and the mixin _Remap;
a caller grid and a caller axis in one call (include/mckpp_hip_hv.h) are the tenth, _SIGNATURES_HV, and the mixin _GridAxis;
completed records on a caller axis (include/mckpp_hip_vrecords.h) are the eleventh, _SIGNATURES_VRECORDS, and the mixin
_AxisRecords.
"""
import ctypes as C
import sys

import numpy as np

NI, NJ = 890, 48

F_PROFILES, F_SAVED, F_SCALARS, F_DIAG = 1, 2, 4, 8
F_RESTART = F_PROFILES | F_SAVED | F_SCALARS
F_ALL = 0xF

ST_ZERO_PIVOT, ST_LONG_ITER, ST_RETRIED, ST_FAILED, ST_DODGY = 1, 2, 4, 8, 16

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

_SWITCHES = [
    "LKPP", "LRI", "LDD", "L_SSref", "L_RELAX_SST", "L_RELAX_CALCONLY", "L_FCORR", "L_FCORR_WITHZ",
    "L_SFCORR", "L_SFCORR_WITHZ", "L_RELAX_SAL", "L_RELAX_OCNT", "L_NO_FREEZE", "L_NO_ISOTHERM",
    "L_DAMP_CURR", "clim_present",
]


class _ConstC(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("nz", "nztmax", "nsflxs", "njdt", "itermax")]
        + [(n, C.c_int32) for n in _SWITCHES]
        + [("iso_bot", C.c_int32), ("dt_uvdamp", C.c_int32), ("maxmodeadv", C.c_int32), ("L_ADVECT", C.c_int32)]
        + [(n, C.c_double) for n in ("hmixtolfrac", "dto", "grav", "vonk", "sice", "iso_thresh")]
        + [(n, _dp) for n in ("zm", "hm", "dm", "tri", "wmt", "wst")]
    )


_STATE_D = [
    "U", "X", "Us", "Xs", "U_init", "hmixd", "f", "ocdepth", "Sref", "SSref", "Ssurf", "hmix", "kmix",
    "Tref", "uref", "vref", "reset_flag", "dampu_flag", "dampv_flag", "freeze_flag", "sflux",
]
_STATE_I = ["old", "new_", "jerlov", "l_ocean", "l_initflag", "run_physics"]
_STATE_DIAG = [
    "rho", "cp", "buoy", "difm", "difs", "dift", "wU", "wX", "wXNT", "ghat", "Rig", "Shsq", "dbloc",
    "swfrac", "swdk_opt",
]
_STATE_EXT_D = ["relax_sst", "SST0", "fcorr_twod", "relax_sal", "relax_ocnT", "fcorr", "fcorr_withz", "sfcorr_withz",
                "ocnT_clim", "sal_clim", "tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr"]
_STATE_EXT_I = ["nmodeadv", "modeadv"]


class _StateC(C.Structure):
    _fields_ = (
        [("npts", C.c_int64)]
        + [(n, _dp) for n in _STATE_D]
        + [(n, _ip) for n in _STATE_I]
        + [(n, _dp) for n in _STATE_DIAG]
        + [(n, _dp) for n in _STATE_EXT_D]
        + [(n, _ip) for n in _STATE_EXT_I]
        + [("advection", _dp)]
    )


# output fields of mckpp_hip_window_* (MCKPP_OUT_* of include/mckpp_hip.h; the XIOS field ids of
# src/mckpp_xios_io.F90:74-210)
OUT_FIELDS = ("u", "v", "T", "S_anom", "hmix", "S", "B", "wu", "wv", "wT", "wS", "wB", "wTnt", "difm", "dift", "difs",
              "rho", "cp", "scorr", "Rig", "dbloc", "Shsq", "tinc_fcorr", "fcorr_z", "sinc_fcorr", "fcorr", "taux_in",
              "tauy_in", "solar_in", "nsolar_in", "PminusE_in", "freeze_flag", "comp_flag", "dampu_flag", "dampv_flag")
OUT = {n: i for i, n in enumerate(OUT_FIELDS)}
OP_MEAN, OP_MIN, OP_MAX, OP_INSTANT = 0, 1, 2, 3
# operations of an output schedule (mckpp_hip_window_schedule), one bit per op of window_record_fetch: 1 << op
WIN_MEAN, WIN_MIN, WIN_MAX, WIN_LAST = 1, 2, 4, 8
OP_LAST = 3
WIN_SCHEDULES = 4


def _win_field(f):
    """An OUT_* index or field name -> the index, or ValueError."""
    if isinstance(f, str):
        if f not in OUT:
            raise ValueError(f"unknown output field {f!r}")
        return OUT[f]
    i = int(f)
    if not 0 <= i < len(OUT_FIELDS):
        raise ValueError(f"unknown output field {f}")
    return i


def _win_args(fields, ops):
    """(fields, ops) of window_schedule as the int32 / uint32 arrays the library takes; ops is one mask for every field
    or one per field.  Unknown fields, empty or foreign masks and a field named twice are refused here."""
    f = [_win_field(x) for x in fields]
    o = [int(ops)] * len(f) if np.ndim(ops) == 0 else [int(x) for x in ops]
    if len(o) != len(f):
        raise ValueError(f"{len(f)} fields but {len(o)} operation masks")
    for fi, oi in zip(f, o):
        if oi == 0 or oi & ~0xF:
            raise ValueError(f"field {OUT_FIELDS[fi]}: operations {oi:#x} (a non-empty mask of WIN_MEAN, WIN_MIN, WIN_MAX, WIN_LAST)")
    if len(set(f)) != len(f):
        raise ValueError("a field named twice in one schedule")
    return np.ascontiguousarray(f, dtype=np.int32), np.ascontiguousarray(o, dtype=np.uint32)


def _win_check_fetch(scheds, sched, field, op):
    """the field and op of a record fetch against what schedule `sched` keeps (as this object set it)"""
    f = _win_field(field)
    if not 0 <= int(op) <= 3:
        raise ValueError(f"op {op} (OP_MEAN 0, OP_MIN 1, OP_MAX 2, OP_LAST 3)")
    kept = scheds.get(int(sched), {})
    if f not in kept:
        raise ValueError(f"field {OUT_FIELDS[f]} is not in output schedule {sched}")
    if not (kept[f] >> int(op)) & 1:
        raise ValueError(f"output schedule {sched} keeps no op {op} of field {OUT_FIELDS[f]} (operations {kept[f]:#x})")
    return f


class _Kept(dict):
    """What a schedule keeps, field -> operation mask, as _WindowSchedules records it; `zoom` is None, or
    (npoints, nlev) of a zoomed schedule: the point axis of its records and the levels of its 3-D fields."""
    zoom = None


def _win_zoom_args(points, levels, npts, nzp1):
    """(points, levels) of window_schedule_zoom as (the int32 array or None, lev0, nlev): a point outside the grid or
    given twice, an empty list and a level range outside the axis are refused here.  npts / nzp1 0: not known yet (no
    upload: the library refuses the call itself)."""
    pts = None
    if points is not None:
        pts = np.ascontiguousarray(points)
        if pts.size < 1:
            raise ValueError("zoom: an empty point list (None: every point)")
        if pts.ndim != 1 or pts.dtype.kind not in "iu":
            raise ValueError("zoom: points is a one-dimensional list of integer point numbers")
        bad = (pts < 0) | (pts >= npts) if npts else pts < 0
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"zoom: point {int(pts[i])} at position {i} is outside 0..{npts - 1 if npts else ''}")
        order = np.argsort(pts, kind="stable")
        same = np.nonzero(pts[order][1:] == pts[order][:-1])[0]
        if len(same):
            a, b = int(order[same[0]]), int(order[same[0] + 1])
            raise ValueError(f"zoom: point {int(pts[a])} twice, at positions {a} and {b}")
        pts = np.ascontiguousarray(pts, dtype=np.int32)
    lev0, nlev = (0, 0) if levels is None else (int(levels[0]), int(levels[1]))
    if nlev < 0 or lev0 < 0 or (nzp1 and lev0 + nlev > nzp1) or (nlev == 0 and lev0 != 0):
        raise ValueError(f"zoom: levels (lev0={lev0}, nlev={nlev}): a range within 0..{nzp1 or ''} ((0, 0) or None: the whole axis)")
    return pts, lev0, nlev


def _win_check_out(scheds, sched, field, out):
    """the array of a fetch from a zoomed schedule against the zoom's shape: out(npoints[, nlev])"""
    kept = scheds.get(int(sched))
    zoom = getattr(kept, "zoom", None)
    if zoom is None:
        return
    npoints, nlev = zoom
    two_d = OUT_FIELDS[field] == "hmix" or field >= OUT["fcorr"]
    want = npoints * (1 if two_d else nlev)
    if out.size != want:
        raise ValueError(f"output schedule {sched} is zoomed: a plane of {OUT_FIELDS[field]} is out({npoints}"
                         f"{'' if two_d else f', {nlev}'}), {want} values, not {out.size}")


def zoom_box(nx, ny, ibegin, ni, jbegin, nj):
    """mckpp_host_zoom_box: the point numbers (int32, i fastest) of the box of ni x nj points from (ibegin, jbegin),
    0-based, of an nx x ny grid - an XIOS zoom_domain as the `points` of window_schedule_zoom."""
    nx, ny, ibegin, ni, jbegin, nj = (int(v) for v in (nx, ny, ibegin, ni, jbegin, nj))
    pts = np.zeros(max(ni, 0) * max(nj, 0), dtype=np.int32)
    _chk(_lib().mckpp_host_zoom_box(nx, ny, ibegin, ni, jbegin, nj, pts.ctypes.data_as(_ip)))
    return pts


# element types of an export (mckpp_hip_window_export): MCKPP_EXP_* of mckpp_hip.h
EXP_OFF, EXP_F64, EXP_F32 = 0, 1, 2
_EXP_DTYPES = {"f8": EXP_F64, "f4": EXP_F32, None: EXP_OFF}
_EXP_NUMPY = {EXP_F64: np.dtype(np.float64), EXP_F32: np.dtype(np.float32)}


def _exp_dtype(dtype):
    """"f8", "f4" or None -> MCKPP_EXP_*, or ValueError."""
    if dtype is not None and not isinstance(dtype, str):
        raise ValueError(f"export dtype {dtype!r} (\"f8\", \"f4\" or None)")
    if dtype not in _EXP_DTYPES:
        raise ValueError(f"export dtype {dtype!r} (\"f8\", \"f4\" or None)")
    return _EXP_DTYPES[dtype]


def _exp_check_out(exports, sched, out):
    """the array of an export fetch against the export of schedule `sched` (as this object set it): its numpy dtype"""
    code = exports.get(int(sched))
    if code is None:
        raise ValueError(f"output schedule {sched} has no export")
    want = _EXP_NUMPY[code]
    if not isinstance(out, np.ndarray) or out.dtype != want:
        raise ValueError(f"the export of output schedule {sched} holds {want.name}, not {getattr(out, 'dtype', type(out).__name__)}")
    if not out.flags["F_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
        raise ValueError("the array of an export fetch must be writeable and contiguous in Fortran order")
    return want


def host_export_merge(npts, nlev, dtype, land_value, points, planes):
    """mckpp_host_export_merge: the shards' planes - planes[d] is (ncol_d, nlev) in Fortran order, column c of shard d
    at point points[d][c] - merged into out(npts, nlev) of `dtype` ("f8" or "f4"); points of no shard get land_value."""
    code = _exp_dtype(dtype)
    if code == EXP_OFF:
        raise ValueError("export dtype None: nothing to merge")
    want = _EXP_NUMPY[code]
    points, planes = list(points), list(planes)
    if len(planes) != len(points):
        raise ValueError(f"{len(points)} point lists but {len(planes)} planes")
    pts = [np.ascontiguousarray(p, dtype=np.int32) for p in points]
    pls = [np.asfortranarray(p, dtype=want).reshape((len(q), int(nlev)), order="F") for p, q in zip(planes, pts)]
    n = len(pts)
    ncol = (C.c_int64 * max(n, 1))(*[len(p) for p in pts])
    pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in pts])
    pl = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in pls])
    out = np.zeros((int(npts), int(nlev)), dtype=want, order="F")
    _chk(_lib().mckpp_host_export_merge(int(npts), int(nlev), code, float(land_value), n, ncol, pp, pl, out.ctypes.data))
    return out


# kinds of the ancillary record series (MCKPP_ANC_* of mckpp_hip.h)
(ANC_SST0, ANC_FCORR_TWOD, ANC_FCORR_WITHZ, ANC_SFCORR_WITHZ, ANC_OCNT_CLIM, ANC_SAL_CLIM, ANC_BOTTOM_TEMP,
 ANC_COUNT) = range(8)
ANC_3D = (ANC_FCORR_WITHZ, ANC_SFCORR_WITHZ, ANC_OCNT_CLIM, ANC_SAL_CLIM)


class _AncEpochC(C.Structure):
    """mckpp_anc_epoch_c"""
    _fields_ = [("rec_prev", C.c_int32), ("rec_next", C.c_int32), ("w_prev", C.c_double), ("w_next", C.c_double)]


def interp_weights(time, ndtupd, dto, spd=86400.0, period=0):
    """(prev_time, next_time, w_prev, w_next) of mckpp_boundary_interpolate_temp / _sal at model time `time` (days):
    mckpp_host_interp_weights, the reference's INTEGER times and its prev_time < 0 branch included."""
    lib = _lib()
    pt, nx, wp, wn = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
    lib.mckpp_host_interp_weights(float(time), int(ndtupd), float(dto), float(spd), int(period), C.byref(pt), C.byref(nx),
                                  C.byref(wp), C.byref(wn))
    return int(pt.value), int(nx.value), float(wp.value), float(wn.value)


class MckppHipError(RuntimeError):
    pass


def _sig(*argtypes, res=C.c_int, twin=False):
    return res, list(argtypes), twin


_H = C.c_void_p                     # mckpp_hip_handle, mckpp_hip_multi_handle
_i, _i32, _i64, _d = C.c_int, C.c_int32, C.c_int64, C.c_double
_i64p = C.POINTER(C.c_int64)
_constp, _statep = C.POINTER(_ConstC), C.POINTER(_StateC)

# Every function of include/mckpp_hip.h, once: (restype, argtypes, twin).  twin: the header also declares
# mckpp_hip_multi_<name> with the same return type and the same parameters after the handle; _signatures() spells it
# out.  tests/test_abi_cpu.py holds this table to the header, type by type.
_SIGNATURES = {
    "mckpp_hip_last_error": _sig(res=C.c_char_p),
    "mckpp_hip_build_id": _sig(res=C.c_char_p),
    "mckpp_hip_build_compiler": _sig(res=C.c_char_p),
    "mckpp_hip_device_count": _sig(),
    "mckpp_host_lookup": _sig(_d, _dp, _dp, res=None),
    "mckpp_host_tri": _sig(_i32, _i32, _d, _dp, _dp, _dp, res=None),
    "mckpp_host_interp_weights": _sig(_d, _i32, _d, _d, _i32, _ip, _ip, _dp, _dp, res=None),
    "mckpp_host_shard_mask": _sig(_i64, _ip, _i32, _i32, _ip, res=_i64),
    "mckpp_host_export_merge": _sig(_i64, _i32, _i32, _d, _i32, _i64p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.c_void_p),
    "mckpp_hip_init": _sig(_constp, _i, C.POINTER(_H)),
    "mckpp_hip_multi_init": _sig(_constp, _i32, _ip, C.POINTER(_H)),
    "mckpp_hip_finalize": _sig(_H, twin=True),
    "mckpp_hip_upload": _sig(_H, _statep, twin=True),
    "mckpp_hip_set_forcing": _sig(_H, _dp, twin=True),
    "mckpp_hip_fluxes": _sig(_H, _i, *[_dp] * 8, _i, _d, _d, twin=True),
    "mckpp_hip_set_flux_series": _sig(_H, _i, _i, _dp, twin=True),
    "mckpp_hip_run_forced": _sig(_H, _i, _i, _i, _i, _d, _d, twin=True),
    "mckpp_hip_flux_ring": _sig(_H, _i, twin=True),
    "mckpp_hip_flux_ring_put": _sig(_H, _i, _dp, twin=True),
    "mckpp_hip_flux_ring_records": _sig(_H, _ip, _ip, twin=True),
    "mckpp_hip_bottomtemp": _sig(_H, _dp, twin=True),
    "mckpp_hip_set_bottomtemp": _sig(_H, _dp, twin=True),
    "mckpp_hip_set_ancillary_series": _sig(_H, _i, _i, _i, _dp, twin=True),
    "mckpp_hip_ancillary_schedule": _sig(_H, _i, _i, _i, _i, _i, C.POINTER(_AncEpochC), twin=True),
    "mckpp_hip_update_ancillaries": _sig(_H, _statep, twin=True),
    "mckpp_hip_set_diagnostics": _sig(_H, _i, twin=True),
    "mckpp_hip_set_solver_mode": _sig(_H, _i, twin=True),
    "mckpp_hip_get_solver_mode": _sig(_H),
    "mckpp_hip_init_ocean": _sig(_H, _i, twin=True),
    "mckpp_hip_step": _sig(_H, _i, _i, twin=True),
    "mckpp_hip_vmix_pass": _sig(_H, _i),
    "mckpp_hip_vmix_only": _sig(_H, _i),
    "mckpp_hip_synchronize": _sig(_H, twin=True),
    "mckpp_hip_download": _sig(_H, _statep, C.c_uint32, twin=True),
    "mckpp_hip_release_host_arrays": _sig(_H, twin=True),
    "mckpp_hip_save_restart": _sig(_H, C.c_char_p, twin=True),
    "mckpp_hip_load_restart": _sig(_H, C.c_char_p, twin=True),
    "mckpp_hip_restart_schedule": _sig(_H, _i, _i, _i, twin=True),
    "mckpp_hip_restart_snapshots": _sig(_H, _i64p, _i64p, twin=True),
    "mckpp_hip_restart_snapshot_save": _sig(_H, _i64, C.c_char_p, twin=True),
    "mckpp_hip_restart_snapshot_release": _sig(_H, _i64, twin=True),
    "mckpp_hip_step_log": _sig(_H, _i64, _i, twin=True),
    "mckpp_hip_step_log_count": _sig(_H, _i64p, _i64p, _ip, twin=True),
    "mckpp_hip_step_log_fetch": _sig(_H, _i64, _ip, _ip, _ip, _ip, twin=True),
    "mckpp_hip_step_log_clear": _sig(_H, twin=True),
    "mckpp_hip_window_select": _sig(_H, _ip, _i32, twin=True),
    "mckpp_hip_window_reset": _sig(_H, twin=True),
    "mckpp_hip_window_accumulate": _sig(_H, twin=True),
    "mckpp_hip_window_fetch": _sig(_H, _i, _i, _dp, twin=True),
    "mckpp_hip_window_schedule": _sig(_H, _i, _i, _i, _i, _ip, C.POINTER(C.c_uint32), _i32, twin=True),
    "mckpp_hip_window_record_fetch": _sig(_H, _i, _i64, _i, _i, _dp, twin=True),
    "mckpp_hip_window_record_release": _sig(_H, _i, _i64, twin=True),
    "mckpp_hip_window_records": _sig(_H, _i, _i64p, _i64p, twin=True),
    "mckpp_hip_window_export": _sig(_H, _i, _i, _d, twin=True),
    "mckpp_hip_window_export_layout": _sig(_H, _i, _ip, _ip, _ip, _ip, _i64p, _i64p, twin=True),
    "mckpp_hip_window_export_fetch": _sig(_H, _i, _i64, _i, _i, C.c_void_p, twin=True),
    "mckpp_hip_window_export_fetch_record": _sig(_H, _i, _i64, C.c_void_p, _i64, twin=True),
    "mckpp_hip_status": _sig(_H, _ip, _i64p, _ip, twin=True),
    "mckpp_hip_ncolumns": _sig(_H, res=_i64, twin=True),
    "mckpp_hip_last_kernel_ms": _sig(_H, _dp, _ip),
    "mckpp_hip_last_launch_count": _sig(_H, res=_i32),
    "mckpp_hip_kernel_name": _sig(_H, res=C.c_char_p),
    "mckpp_hip_kernel_residency": _sig(_H, _ip, _ip, _ip, _i64p),
    "mckpp_hip_eos_batch": _sig(_H, _i64, *[_dp] * 7),
    "mckpp_hip_exp_batch": _sig(_H, _i64, _dp, _dp),
    "mckpp_hip_div_batch": _sig(_H, _i64, _dp, _dp, _dp),
    "mckpp_hip_multi_ndev": _sig(_H, res=_i32),
    "mckpp_hip_multi_ctx": _sig(_H, _i32, res=_H),
    "mckpp_hip_multi_gather": _sig(_H, _i32, _i32, _dp),
}


class _DevPlaneC(C.Structure):
    """mckpp_dev_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "lev0", "nlev", "dtype", "fill_land")] + \
               [("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_device.h, the device-array interface, in the same form; tests/test_device_arrays_cpu.py
# holds this table to that header.  Kept out of _signatures(), which describes mckpp_hip.h.
_voidpp = C.POINTER(C.c_void_p)     # const double *const fields[8]
_SIGNATURES_DEVICE = {
    "mckpp_hip_fluxes_dev": _sig(_H, _i, _voidpp, _i, _d, _d, C.c_void_p, twin=True),
    "mckpp_hip_flux_ring_put_dev": _sig(_H, _i, _voidpp, C.c_void_p, twin=True),
    "mckpp_hip_fetch_dev": _sig(_H, _i32, C.POINTER(_DevPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_dev_fence": _sig(_H, C.c_void_p, twin=True),
}


class _WinZoomC(C.Structure):
    """mckpp_win_zoom_c"""
    _fields_ = [("points", _ip), ("npoints", C.c_int64), ("lev0", C.c_int32), ("nlev", C.c_int32)]


# Every function of include/mckpp_hip_zoom.h, output schedules over chosen points and levels, in the same form;
# tests/test_window_zoom_cpu.py holds this table to that header.
_SIGNATURES_ZOOM = {
    "mckpp_hip_window_schedule_zoom": _sig(_H, _i, _i, _i, _i, _ip, C.POINTER(C.c_uint32), _i32, C.POINTER(_WinZoomC),
                                           twin=True),
    "mckpp_hip_window_zoom": _sig(_H, _i, _i64p, _ip, _ip, _i64p, twin=True),
    "mckpp_host_zoom_box": _sig(_i64, _i64, _i64, _i64, _i64, _i64, _ip),
}


class _DevRecordPlaneC(C.Structure):
    """mckpp_dev_record_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("sched", "field", "op", "lev0", "nlev", "dtype", "fill_land")] + \
               [("rec", C.c_int64), ("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_device_records.h, records of output schedules into device arrays, in the same
# form; tests/test_device_records_cpu.py holds this table to that header.
_SIGNATURES_RECORDS = {
    "mckpp_hip_records_dev": _sig(_H, _i32, C.POINTER(_DevRecordPlaneC), C.c_void_p, twin=True),
}


class _PutPlaneC(C.Structure):
    """mckpp_put_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "lev0", "nlev", "dtype", "op", "flags")] + \
               [("skip_value", C.c_double), ("in", C.c_void_p)]


# Every function of include/mckpp_hip_put.h, the prognostic state set or incremented in place, in the same form;
# tests/test_put_cpu.py holds this table to that header.
_SIGNATURES_PUT = {
    "mckpp_hip_put_dev": _sig(_H, _i32, C.POINTER(_PutPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_put_host": _sig(_H, _i32, C.POINTER(_PutPlaneC), twin=True),
}


class _ReducePlaneC(C.Structure):
    """mckpp_reduce_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("sched", "field", "op", "lev0", "nlev", "axis_op", "domain_op", "weighted")] + \
               [("rec", C.c_int64), ("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_reduce.h, records reduced over levels and points, in the same form;
# tests/test_reduce_cpu.py holds this table to that header.
_SIGNATURES_REDUCE = {
    "mckpp_hip_reduce_weights": _sig(_H, _dp, _dp, _dp, twin=True),
    "mckpp_hip_records_reduce_dev": _sig(_H, _i32, C.POINTER(_ReducePlaneC), C.c_void_p, twin=True),
    "mckpp_hip_records_reduce_host": _sig(_H, _i32, C.POINTER(_ReducePlaneC), twin=True),
    "mckpp_host_reduce_tree": _sig(_dp, _i64, res=_d),
}


class _VaxisPutPlaneC(C.Structure):
    """mckpp_vaxis_put_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "axis", "dtype", "op", "flags")] + \
               [("skip_value", C.c_double), ("in", C.c_void_p)]


class _VaxisProfilesC(C.Structure):
    """mckpp_vaxis_profiles_c"""
    _fields_ = [(n, C.c_int32) for n in ("axis_vel", "axis_temp", "axis_sal", "dtype")] + [("tk0", C.c_double)] + \
               [(n, C.c_void_p) for n in ("u", "v", "temp", "sal")]


class _VaxisDevPlaneC(C.Structure):
    """mckpp_vaxis_dev_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "axis", "dtype", "fill_land")] + \
               [("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_vaxis.h, the caller's vertical axes, in the same form; tests/test_vaxis_cpu.py
# holds this table to that header.
_SIGNATURES_VAXIS = {
    "mckpp_host_vaxis_map": _sig(_i32, _dp, _i32, _dp, _ip, _ip, _dp, _dp),
    "mckpp_hip_vaxis_define": _sig(_H, _i, _i32, _dp, twin=True),
    "mckpp_hip_vaxis_put_dev": _sig(_H, _i32, C.POINTER(_VaxisPutPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_vaxis_put_host": _sig(_H, _i32, C.POINTER(_VaxisPutPlaneC), twin=True),
    "mckpp_hip_vaxis_init_profiles_dev": _sig(_H, C.POINTER(_VaxisProfilesC), C.c_void_p, twin=True),
    "mckpp_hip_vaxis_init_profiles_host": _sig(_H, C.POINTER(_VaxisProfilesC), twin=True),
    "mckpp_hip_vaxis_fetch_dev": _sig(_H, _i32, C.POINTER(_VaxisDevPlaneC), C.c_void_p, twin=True),
}


class _HgridTableC(C.Structure):
    """mckpp_hgrid_table_c"""
    _fields_ = [("ptr", _i64p), ("idx", _ip), ("w", _dp)]


class _HgridPlaneC(C.Structure):
    """mckpp_hgrid_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "lev0", "nlev", "dtype", "grid", "norm", "fill_land")] + \
               [("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_hgrid.h, the caller's horizontal grids, in the same form; tests/test_hgrid_cpu.py
# holds this table to that header.
_hgtp, _u8p = C.POINTER(_HgridTableC), C.POINTER(C.c_ubyte)
_SIGNATURES_HGRID = {
    "mckpp_host_hgrid_check": _sig(C.c_char_p, _i64, _i64, _hgtp, C.c_char_p, _i64),
    "mckpp_host_hgrid_apply": _sig(_i64, _hgtp, _dp, _u8p, _i, _i, _d, _dp),
    "mckpp_host_hgrid_slices": _sig(_i64, _i64p, _hgtp, _u8p, _i64p, _ip, _ip, _dp, res=_i64),
    "mckpp_hip_hgrid_define": _sig(_H, _i, _i64, _hgtp, _hgtp, twin=True),
    "mckpp_hip_hgrid_info": _sig(_H, _i, _i64p, twin=True),
    "mckpp_hip_hgrid_fluxes_dev": _sig(_H, _i, _i, _voidpp, _i, _d, _d, C.c_void_p, twin=True),
    "mckpp_hip_hgrid_flux_ring_put_dev": _sig(_H, _i, _i, _voidpp, C.c_void_p, twin=True),
    "mckpp_hip_hgrid_fetch_dev": _sig(_H, _i32, C.POINTER(_HgridPlaneC), C.c_void_p, twin=True),
}


class _RemapRecordPlaneC(C.Structure):
    """mckpp_remap_record_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("sched", "field", "op", "lev0", "nlev", "dtype", "grid", "norm", "fill_land")] + \
               [("rec", C.c_int64), ("land_value", C.c_double), ("out", C.c_void_p)]


class _RemapPutPlaneC(C.Structure):
    """mckpp_remap_put_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "lev0", "nlev", "dtype", "op", "flags", "grid")] + \
               [("skip_value", C.c_double), ("in", C.c_void_p)]


# Every function of include/mckpp_hip_remap.h, records out and state in on the caller's horizontal grids, in the same
# form; tests/test_remap_cpu.py holds this table to that header.
_SIGNATURES_REMAP = {
    "mckpp_hip_remap_records_dev": _sig(_H, _i32, C.POINTER(_RemapRecordPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_remap_put_dev": _sig(_H, _i32, C.POINTER(_RemapPutPlaneC), C.c_void_p, twin=True),
}


class _HvPlaneC(C.Structure):
    """mckpp_hv_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "axis", "dtype", "grid", "norm", "fill_land")] + \
               [("land_value", C.c_double), ("out", C.c_void_p)]


class _HvPutPlaneC(C.Structure):
    """mckpp_hv_put_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("field", "axis", "dtype", "op", "flags", "grid")] + \
               [("skip_value", C.c_double), ("in", C.c_void_p)]


# Every function of include/mckpp_hip_hv.h, a caller grid and a caller axis in one call, in the same form;
# tests/test_hv_cpu.py holds this table to that header.
_SIGNATURES_HV = {
    "mckpp_hip_hv_fetch_dev": _sig(_H, _i32, C.POINTER(_HvPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_hv_put_dev": _sig(_H, _i32, C.POINTER(_HvPutPlaneC), C.c_void_p, twin=True),
}


class _VaxisRecordPlaneC(C.Structure):
    """mckpp_vaxis_record_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("sched", "field", "op", "axis", "dtype", "fill_land")] + \
               [("rec", C.c_int64), ("land_value", C.c_double), ("out", C.c_void_p)]


class _HvRecordPlaneC(C.Structure):
    """mckpp_hv_record_plane_c"""
    _fields_ = [(n, C.c_int32) for n in ("sched", "field", "op", "axis", "dtype", "grid", "norm", "fill_land")] + \
               [("rec", C.c_int64), ("land_value", C.c_double), ("out", C.c_void_p)]


# Every function of include/mckpp_hip_vrecords.h, completed records on a caller axis, in the same form;
# tests/test_vrecords_cpu.py holds this table to that header.
_SIGNATURES_VRECORDS = {
    "mckpp_host_vrecords_rule": _sig(_i32, _ip, _ip, _i32, _i32, _ip, _ip),
    "mckpp_hip_vrecords_vaxis_dev": _sig(_H, _i32, C.POINTER(_VaxisRecordPlaneC), C.c_void_p, twin=True),
    "mckpp_hip_vrecords_vaxis_host": _sig(_H, _i32, C.POINTER(_VaxisRecordPlaneC), twin=True),
    "mckpp_hip_vrecords_hv_dev": _sig(_H, _i32, C.POINTER(_HvRecordPlaneC), C.c_void_p, twin=True),
}


def _spelled(table):
    """C name -> (restype, argtypes) of a signature table with the multi_ twins spelled out."""
    out = {}
    for name, (res, argtypes, twin) in table.items():
        out[name] = (res, argtypes)
        if twin:
            out["mckpp_hip_multi_" + name[len("mckpp_hip_"):]] = (res, argtypes)
    return out


def _signatures():
    """C name -> (restype, argtypes) of every function of mckpp_hip.h: _SIGNATURES with the multi_ twins spelled out."""
    return _spelled(_SIGNATURES)


def _signatures_device():
    """... and of every function of mckpp_hip_device.h."""
    return _spelled(_SIGNATURES_DEVICE)


def _signatures_zoom():
    """... and of every function of mckpp_hip_zoom.h."""
    return _spelled(_SIGNATURES_ZOOM)


def _signatures_records():
    """... and of every function of mckpp_hip_device_records.h."""
    return _spelled(_SIGNATURES_RECORDS)


def _signatures_put():
    """... and of every function of mckpp_hip_put.h."""
    return _spelled(_SIGNATURES_PUT)


def _signatures_reduce():
    """... and of every function of mckpp_hip_reduce.h."""
    return _spelled(_SIGNATURES_REDUCE)


def _signatures_vaxis():
    """... and of every function of mckpp_hip_vaxis.h."""
    return _spelled(_SIGNATURES_VAXIS)


def _signatures_hgrid():
    """... and of every function of mckpp_hip_hgrid.h."""
    return _spelled(_SIGNATURES_HGRID)


def _signatures_remap():
    """... and of every function of mckpp_hip_remap.h."""
    return _spelled(_SIGNATURES_REMAP)


def _signatures_hv():
    """... and of every function of mckpp_hip_hv.h."""
    return _spelled(_SIGNATURES_HV)


def _signatures_vrecords():
    """... and of every function of mckpp_hip_vrecords.h."""
    return _spelled(_SIGNATURES_VRECORDS)


def _bind(lib):
    if getattr(lib, "_mckpp_bound", False):
        return lib
    # MCKPP_HIP_LIBRARY may name an older build (tools/export_rate.py --lib): a name it does not export is skipped -
    # everything else works with it, and a call of that name fails there by name
    for name, (res, argtypes) in {**_signatures(), **_signatures_device(), **_signatures_zoom(),
                                  **_signatures_records(), **_signatures_put(), **_signatures_reduce(),
                                  **_signatures_vaxis(), **_signatures_hgrid(), **_signatures_remap(),
                                  **_signatures_hv(), **_signatures_vrecords()}.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    lib._mckpp_bound = True
    return lib


def _lib():
    from . import load_library

    return _bind(load_library())


def build_compiler():
    return _lib().mckpp_hip_build_compiler().decode()


def build_id():
    """Identifier of the kernel sources the loaded library was built from."""
    return _lib().mckpp_hip_build_id().decode()


def _chk(rc):
    if rc != 0:
        raise MckppHipError(_lib().mckpp_hip_last_error().decode())


def _f(shape):
    return np.zeros(shape, dtype=np.float64, order="F")


class KppConstFields:
    """kpp_const_type, hot-path subset (src/mckpp_data_fields.F90:187-346), with the
    defaults of mckpp_initialize_namelist (src/mckpp_initialize_namelist_mod.F90:27-119)
    and the uniform/stretched grid of mckpp_initialize_geography
    (src/mckpp_initialize_geography_mod.F90:45-74)."""

    def __init__(self, nz, nztmax=None, dto=3600.0, dmax=200.0, zm=None, hm=None, dm=None):
        from . import synth

        self.nz, self.nzp1 = nz, nz + 1
        self.nztmax = nztmax if nztmax is not None else nz + 1
        self.nsflxs, self.njdt, self.itermax = 9, 1, 200
        self.hmixtolfrac = 0.1
        self.dto = float(dto)
        self.grav, self.vonk, self.sice = 9.816, 0.4, 4.0
        self.iso_bot, self.iso_thresh, self.dt_uvdamp = 2, 0.002, 360
        self.maxmodeadv = 6
        self.L_ADVECT = 0
        self.L_VARY_BOTTOM_TEMP = 0
        for s in _SWITCHES:
            setattr(self, s, 0)
        self.LKPP = self.LRI = self.L_SSref = 1
        if zm is None:
            z, h, d = synth.uniform_grid(nz, dmax)
            zm, hm, dm = z[1:nz + 2], h[1:nz + 2], d
        self.zm = np.ascontiguousarray(zm, dtype=np.float64)      # zm(1:nzp1)
        self.hm = np.ascontiguousarray(hm, dtype=np.float64)      # hm(1:nzp1)
        self.dm = np.ascontiguousarray(dm, dtype=np.float64)      # dm(0:nz)
        assert self.zm.shape == (nz + 1,) and self.hm.shape == (nz + 1,) and self.dm.shape == (nz + 1,)
        self.wmt = _f((NI + 2, NJ + 2))                           # wmt(0:891,0:49)
        self.wst = _f((NI + 2, NJ + 2))
        self.tri = _f((self.nztmax + 1, 2, 1))                    # tri(0:nztmax,0:1,ngrid)
        _lib().mckpp_host_tri(nz, self.nztmax, self.dto, self.zm.ctypes.data_as(_dp),
                              self.hm.ctypes.data_as(_dp), self.tri.ctypes.data_as(_dp))

    def as_c(self):
        c = _ConstC()
        for n in ("nz", "nztmax", "nsflxs", "njdt", "itermax", "iso_bot", "dt_uvdamp", "maxmodeadv", "L_ADVECT"):
            setattr(c, n, int(getattr(self, n)))
        for n in _SWITCHES:
            setattr(c, n, int(getattr(self, n)))
        for n in ("hmixtolfrac", "dto", "grav", "vonk", "sice", "iso_thresh"):
            setattr(c, n, float(getattr(self, n)))
        for n in ("zm", "hm", "dm", "tri", "wmt", "wst"):
            setattr(c, n, getattr(self, n).ctypes.data_as(_dp))
        return c


def mckpp_physics_lookup(kpp_const_fields):
    """src/mckpp_physics_lookup_mod.F90:11 - fill wmt, wst."""
    _lib().mckpp_host_lookup(kpp_const_fields.vonk, kpp_const_fields.wmt.ctypes.data_as(_dp),
                             kpp_const_fields.wst.ctypes.data_as(_dp))


class Kpp3dFields:
    """kpp_3d_type, hot-path subset, allocated like mckpp_allocate_3d_fields
    (src/mckpp_data_fields.F90:353-447)."""

    def __init__(self, npts, c):
        nz, nzp1, nzt = c.nz, c.nzp1, c.nztmax
        self.npts = npts
        self.U = _f((npts, nzp1, 2))
        self.X = _f((npts, nzp1, 2))
        self.Us = _f((npts, nzp1, 2, 2))
        self.Xs = _f((npts, nzp1, 2, 2))
        self.U_init = _f((npts, nzp1, 2))
        self.hmixd = _f((npts, 2))
        for n in ("f", "ocdepth", "Sref", "SSref", "Ssurf", "hmix", "kmix", "Tref", "uref", "vref",
                  "reset_flag", "dampu_flag", "dampv_flag", "freeze_flag"):
            setattr(self, n, _f((npts,)))
        self.ocdepth[:] = -10000.0
        self.sflux = _f((npts, c.nsflxs, 5, c.njdt + 1))
        self.old = np.zeros(npts, dtype=np.int32)
        self.new_ = np.ones(npts, dtype=np.int32)
        self.jerlov = np.full(npts, 3, dtype=np.int32)
        self.l_ocean = np.ones(npts, dtype=np.int32)
        self.l_initflag = np.zeros(npts, dtype=np.int32)
        self.run_physics = np.ones(npts, dtype=np.int32)
        self.rho = _f((npts, nzt + 2))
        self.cp = _f((npts, nzt + 2))
        self.buoy = _f((npts, nzt + 1))
        self.difm = _f((npts, nzt + 1))
        self.difs = _f((npts, nzt + 1))
        self.dift = _f((npts, nzt + 1))
        self.wU = _f((npts, nzt + 1, 3))
        self.wX = _f((npts, nzt + 1, 3))
        self.wXNT = _f((npts, nzt + 1, 2))
        self.ghat = _f((npts, nzt))
        self.Rig = _f((npts, nzp1))
        self.Shsq = _f((npts, nzp1))
        self.dbloc = _f((npts, nz))
        self.swfrac = _f((npts, nzp1))
        self.swdk_opt = _f((npts, nz + 1))
        self.bottom_temp = _f((npts,))
        for n in ("relax_sst", "SST0", "fcorr_twod", "relax_sal", "relax_ocnT", "fcorr"):
            setattr(self, n, _f((npts,)))
        for n in ("fcorr_withz", "sfcorr_withz", "ocnT_clim", "sal_clim", "tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr"):
            setattr(self, n, _f((npts, nzp1)))
        self.nmodeadv = np.zeros((npts, 2), dtype=np.int32, order="F")
        self.modeadv = np.zeros((npts, c.maxmodeadv, 2), dtype=np.int32, order="F")
        self.advection = _f((npts, c.maxmodeadv, 2))

    def as_c(self):
        s = _StateC()
        s.npts = self.npts
        for n in _STATE_D + _STATE_DIAG + _STATE_EXT_D + ["advection"]:
            a = getattr(self, n)
            assert a.flags["F_CONTIGUOUS"] and a.dtype == np.float64, n
            setattr(s, n, a.ctypes.data_as(_dp))
        for n in _STATE_I + _STATE_EXT_I:
            a = getattr(self, n)
            assert a.dtype == np.int32 and a.flags["F_CONTIGUOUS"], n
            setattr(s, n, a.ctypes.data_as(_ip))
        return s


# The five feature groups of _Handle below, each stated once for one context and for all shards of a multi handle:
# they reach the library through the handle's _call / _raw and know its point count as self._npts.
class _WindowSchedules:
    """Output windows accumulated inside the step launches (mckpp_hip_window_schedule and its kin).  The schedules this
    object set are kept here so that a fetch of a field or an op a schedule does not keep is refused before the library
    is called."""

    def _scheds(self):
        return self.__dict__.setdefault("_wsched", {})

    def window_schedule(self, sched, nt_origin, period, nrec, fields, ops):
        """Schedule `sched` (0..WIN_SCHEDULES-1): window w covers steps nt_origin + w*period .. + period-1, nrec records
        in a ring; fields are OUT_* indices or names, ops one WIN_* mask for all or one per field.  No fields: cancel."""
        f, o = _win_args(fields, ops)
        self._win_set("window_schedule", sched, (int(nt_origin), int(period), int(nrec)), f, o, (), None)

    def window_schedule_zoom(self, sched, nt_origin, period, nrec, fields, ops, points=None, levels=None):
        """window_schedule restricted to `points` - distinct 0-based point numbers of the 3-D ordering in any order, land
        allowed; None: every point - and to levels = (lev0, nlev) of each 3-D field's own axis (None: the whole axis).
        The records, the export and the fetches have the zoom's shape: out(len(points)[, nlev]), in list order."""
        f, o = _win_args(fields, ops)
        pts, lev0, nlev = _win_zoom_args(points, levels, self._npts, self._nzp1)
        z = _WinZoomC(pts.ctypes.data_as(_ip) if pts is not None else None, 0 if pts is None else len(pts), lev0, nlev)
        shape = (self._npts if pts is None else len(pts), nlev or self._nzp1)
        self._win_set("window_schedule_zoom", sched, (int(nt_origin), int(period), int(nrec)), f, o, (C.byref(z),), shape)

    def window_zoom(self, sched):
        """(npoints, lev0, nlev, ring_bytes) of schedule `sched`, zoomed or not: the point axis of its records, the level
        range of its 3-D fields, the device bytes of its record ring (all shards'; without the export)."""
        n, l0, nl, rb = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        self._call("window_zoom", int(sched), C.byref(n), C.byref(l0), C.byref(nl), C.byref(rb))
        return int(n.value), int(l0.value), int(nl.value), int(rb.value)

    def _win_set(self, name, sched, when, f, o, more, shape):
        """the call that sets or cancels a schedule, and this object's record of what the schedule keeps"""
        if self._raw(name, int(sched), *when, f.ctypes.data_as(_ip), o.ctypes.data_as(C.POINTER(C.c_uint32)), len(f),
                     *more) != 0:
            err = _lib().mckpp_hip_last_error().decode()
            a = C.c_int64()
            if self._raw("window_records", int(sched), C.byref(a), C.byref(a)) != 0:
                self._scheds().pop(int(sched), None)   # (a refused schedule leaves the one in place; memory that could
            raise MckppHipError(err)                    # not be had leaves none)
        self.__dict__.get("_wexport", {}).pop(int(sched), None)   # (a schedule set anew has no export)
        if len(f):
            kept = _Kept((int(a), int(b)) for a, b in zip(f, o))
            kept.zoom = shape
            self._scheds()[int(sched)] = kept
        else:
            self._scheds().pop(int(sched), None)

    def window_record_fetch(self, sched, rec, field, op, out):
        """Record `rec` of schedule `sched`: op OP_MEAN / OP_MIN / OP_MAX / OP_LAST of `field` into out(npts[, nzp1])
        (Fortran order; land points keep what out held)."""
        f = _win_check_fetch(self._scheds(), sched, field, op)
        assert out.flags["F_CONTIGUOUS"] and out.dtype == np.float64
        _win_check_out(self._scheds(), sched, f, out)
        self._hold(out)
        self._call("window_record_fetch", int(sched), int(rec), f, int(op), out.ctypes.data_as(_dp))
        return out

    def window_record_release(self, sched, upto_rec):
        """Release the records of `sched` up to and including upto_rec (their ring slots are free again)."""
        self._call("window_record_release", int(sched), int(upto_rec))

    def window_records(self, sched):
        """(first_kept, last_complete): records first_kept .. last_complete of `sched` can be fetched."""
        a, b = C.c_int64(), C.c_int64()
        self._call("window_records", int(sched), C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # The export of a schedule's records (mckpp_hip_window_export): every step-launch call packs the records it completed
    # into export slots in the host's layout, and a fetch is one copy behind the slot's event, on a stream of its own -
    # it runs while later launches do.  The exports this object set are kept here (like the schedules) so that an array
    # of the wrong type is refused before the library is called.
    def _exports(self):
        live = self.__dict__.setdefault("_wexport", {})
        for s in [s for s in live if s not in self._scheds()]:   # (cancelled with its schedule)
            del live[s]
        return live

    def window_export(self, sched, dtype, land_value=1e20):
        """Export schedule `sched` as "f8" (double) or "f4" (narrowed to float after the mean's division); None drops the
        export.  Land points of every plane hold land_value.  Records already complete are packed at once."""
        code = _exp_dtype(dtype)
        self._exports().pop(int(sched), None)
        self._call("window_export", int(sched), code, float(land_value))
        if code != EXP_OFF:
            self._exports()[int(sched)] = code

    def window_export_layout(self, sched):
        """(planes, record_bytes): planes is a list of (field, op, nlev, offset_bytes) in the order of a record - the
        schedule's fields in its order, the kept ops of each in the order mean, min, max, last."""
        n, rb = C.c_int32(), C.c_int64()
        self._call("window_export_layout", int(sched), C.byref(n), None, None, None, None, C.byref(rb))
        fld, op, nlev = (np.zeros(n.value, dtype=np.int32) for _ in range(3))
        off = np.zeros(n.value, dtype=np.int64)
        self._call("window_export_layout", int(sched), C.byref(n), fld.ctypes.data_as(_ip), op.ctypes.data_as(_ip),
                   nlev.ctypes.data_as(_ip), off.ctypes.data_as(_i64p), C.byref(rb))
        return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(fld, op, nlev, off)], int(rb.value)

    def window_export_fetch(self, sched, rec, field, op, out):
        """Plane (field, op) of record `rec` through the export into out(npts[, nzp1]) (Fortran order, float64 or float32
        as the export was set): what window_record_fetch gives into an array pre-filled with land_value."""
        f = _win_check_fetch(self._scheds(), sched, field, op)
        _exp_check_out(self._exports(), sched, out)
        _win_check_out(self._scheds(), sched, f, out)
        self._hold(out)
        self._call("window_export_fetch", int(sched), int(rec), f, int(op), out.ctypes.data)
        return out

    def window_export_fetch_record(self, sched, rec, out):
        """All of record `rec` through the export into the one-dimensional array `out` (at least record_bytes of
        window_export_layout, whose offsets locate the planes)."""
        _exp_check_out(self._exports(), sched, out)
        if out.ndim != 1:
            raise ValueError("the array of a whole-record fetch is one-dimensional")
        self._hold(out)
        self._call("window_export_fetch_record", int(sched), int(rec), out.ctypes.data, int(out.nbytes))
        return out


class _RestartSchedule:
    """Restart snapshots taken inside the step launches (mckpp_hip_restart_schedule and its kin).  restart_scheduled is
    (nt_origin, period, nslots) of the schedule this object set, or None."""
    restart_scheduled = None

    def restart_schedule(self, nt_origin, period, nslots):
        """Snapshot s is the state after step nt_origin + (s+1)*period - 1, kept in ring slot s % nslots.  Period 0:
        cancel.  (1, ndt_per_restart, n) is the reference's MOD(ntime, ndt_per_restart) == 0."""
        nt_origin, period, nslots = int(nt_origin), int(period), int(nslots)
        if period < 0:
            raise ValueError(f"restart_schedule: period={period} (0 cancels the schedule)")
        if period > 0 and (nt_origin < 1 or nslots < 1):
            raise ValueError(f"restart_schedule: nt_origin={nt_origin} nslots={nslots} (each at least 1)")
        self.restart_scheduled = None   # (the library drops the schedule in place before it sets the new one)
        self._call("restart_schedule", nt_origin, period, nslots)
        if period > 0:
            self.restart_scheduled = (nt_origin, period, nslots)

    def restart_snapshots(self):
        """(first_kept, last_complete): snapshots first_kept .. last_complete can be saved."""
        a, b = C.c_int64(), C.c_int64()
        self._call("restart_snapshots", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def restart_snapshot_save(self, snap, path):
        """Snapshot `snap` as the file save_restart would have written after the snapshot's step (a multi handle: one
        file per shard, <path>.<shard>of<ndev>).  Launches queued behind the snapshot's keep running meanwhile."""
        self._call("restart_snapshot_save", int(snap), str(path).encode())

    def restart_snapshot_release(self, upto_snap):
        """Release the snapshots up to and including upto_snap (their ring slots are free again)."""
        self._call("restart_snapshot_release", int(upto_snap))


class _StepLog:
    """The step log of the step launches (mckpp_hip_step_log and its kin).  step_logged is (capacity, min_passes) of
    the log this object set, or None."""
    step_logged = None

    def step_log(self, capacity, min_passes=0):
        """Every column-step of a step launch that ends with a non-zero status word, or with at least min_passes passes
        (0: status only), leaves a record, up to `capacity` of them (a multi handle: per shard).  Capacity 0: cancel."""
        capacity, min_passes = int(capacity), int(min_passes)
        if capacity < 0 or min_passes < 0:
            raise ValueError(f"step_log: capacity={capacity} min_passes={min_passes} (0 cancels the log / logs flagged "
                             "steps only)")
        self.step_logged = None   # (the library drops the log in place before it sets the new one)
        self._call("step_log", capacity, min_passes)
        if capacity > 0:
            self.step_logged = (capacity, min_passes)

    def step_log_count(self):
        """(n_events, n_stored, status_or) since the log was set or cleared; status_or covers the events that found no
        room too."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
        self._call("step_log_count", C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def step_log_fetch(self):
        """The stored records as int32 arrays (nt, point, status, npasses), sorted by (nt, point); point is the 0-based
        index in the caller's 3-D ordering, as status() numbers its words."""
        n = self.step_log_count()[1]
        out = [np.zeros(n, np.int32) for _ in range(4)]
        self._call("step_log_fetch", n, *[a.ctypes.data_as(_ip) for a in out])
        return tuple(out)

    def step_log_clear(self):
        """Keep the log; the event count and the OR of the status words are zero again."""
        self._call("step_log_clear")


class _AncillarySeries:
    """Ancillary record series and their schedules (mckpp_hip_set_ancillary_series, mckpp_hip_ancillary_schedule)."""
    interp_weights = staticmethod(interp_weights)

    def set_ancillary_series(self, kind, rec0, records):
        """records[nrec, npts] (ANC_SST0, ANC_FCORR_TWOD, ANC_BOTTOM_TEMP) or records[nrec, nzp1, npts] (the others) become
        the kind's resident records, number rec0 of the run first; None or an empty array frees them."""
        kind = int(kind)
        if records is None or len(records) == 0:
            self._call("set_ancillary_series", kind, int(rec0), 0, None)
            return
        r = np.ascontiguousarray(records, dtype=np.float64)
        if r.ndim != (3 if kind in ANC_3D else 2) or r.shape[-1] != self._npts:
            raise ValueError(f"set_ancillary_series: kind {kind} takes records[nrec{', nzp1' if kind in ANC_3D else ''}, "
                             f"npts={self._npts}], got {r.shape}")
        self._hold(r)
        self._call("set_ancillary_series", kind, int(rec0), int(r.shape[0]), r.ctypes.data_as(_dp))

    def ancillary_schedule(self, kind, nt_origin, cadence, epochs, epoch0=0):
        """Step nt is in epoch (nt - nt_origin) // cadence; epochs[i] describes epoch epoch0 + i: a record number (the
        record as it is), or (rec_prev, rec_next, w_prev, w_next) for record[rec_next]*w_next + record[rec_prev]*w_prev
        (ANC_OCNT_CLIM and ANC_SAL_CLIM only).  None or no epochs: cancel the kind's schedule."""
        ep = list(epochs) if epochs is not None else []
        arr = (_AncEpochC * max(1, len(ep)))()
        for i, e in enumerate(ep):
            if np.ndim(e) == 0:
                arr[i] = _AncEpochC(int(e), -1, 0.0, 0.0)
            else:
                arr[i] = _AncEpochC(int(e[0]), int(e[1]), float(e[2]), float(e[3]))
        self._call("ancillary_schedule", int(kind), int(nt_origin), int(cadence), int(epoch0), len(ep), arr)


class _FluxRing:
    """The flux-record ring (mckpp_hip_flux_ring and its kin)."""

    def flux_ring(self, nslots):
        """A ring of `nslots` flux-record slots on the device, empty; 0 cancels it.  Drops a set_flux_series series."""
        self._call("flux_ring", int(nslots))

    def flux_ring_put(self, rec, fields):
        """fields[8, npts] (taux, tauy, swf, lwf, lhf, shf, rain, snow) is record `rec` of the run; records arrive in
        order.  Returns without waiting for the device: `fields` may be rewritten at once."""
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.ndim != 2 or f.shape[0] != 8:
            raise ValueError(f"flux_ring_put: a record is fields[8, npts], got {f.shape}")
        if self._npts and f.shape[1] != self._npts:   # (before an upload the library refuses the call itself)
            raise ValueError(f"flux_ring_put: a record is fields[8, npts={self._npts}], got {f.shape}")
        self._call("flux_ring_put", int(rec), f.ctypes.data_as(_dp))

    def flux_ring_records(self):
        """(first, last) resident records: the last min(nslots, records put); (-1, -1): the ring is empty."""
        a, b = C.c_int(), C.c_int()
        self._call("flux_ring_records", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)


# output fields with one value per point (the others have nzp1 levels: mckpp_hip_window_fetch's axes)
_OUT_2D = frozenset([OUT["hmix"]]) | frozenset(range(OUT["fcorr"], len(OUT_FIELDS)))
_DEV_TYPESTR = {"<f8": EXP_F64, "<f4": EXP_F32}


def _dev_array(a, what, count, typestrs=("<f8",)):
    """(address, typestr) of the device array `a` - anything exposing __cuda_array_interface__, which torch's ROCm tensors
    do - after the checks the library cannot make: element type, C-contiguity, element count.  ValueError otherwise; a
    host array is refused here."""
    try:
        cai = None if isinstance(a, np.ndarray) else a.__cuda_array_interface__
    except (AttributeError, TypeError):     # (a torch tensor in host memory has the attribute, and raises TypeError)
        cai = None
    if cai is None:
        raise ValueError(f"{what}: a host array ({type(a).__module__}.{type(a).__name__}); the call takes arrays in device "
                         "memory that expose __cuda_array_interface__ (the methods without _dev take host arrays)")
    shape, typestr = tuple(int(n) for n in cai["shape"]), cai["typestr"]
    if typestr not in typestrs:
        raise ValueError(f"{what}: element type {typestr}, the call takes {' or '.join(typestrs)}")
    itemsize, strides = int(typestr[2:]), cai.get("strides")
    if strides is not None:
        want, step = [], itemsize
        for n in reversed(shape):
            want.insert(0, step)
            step *= max(n, 1)
        if any(n > 1 and int(s) != w for n, s, w in zip(shape, strides, want)):
            raise ValueError(f"{what}: not C-contiguous (shape {shape}, strides {tuple(strides)})")
    if int(np.prod(shape, dtype=np.int64)) != count:
        raise ValueError(f"{what}: shape {shape}, the call takes {count} elements")
    return int(cai["data"][0]), typestr


def _dev_stream(stream):
    """A caller's stream as the void * the library takes: an integer handle, an object with torch's cuda_stream, or
    None - torch's current stream where torch is loaded and has initialised its device, else the null stream."""
    if stream is None:
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_initialized():
            return C.c_void_p(None)
        stream = torch.cuda.current_stream()
    if isinstance(stream, int):
        return C.c_void_p(stream or None)
    if not hasattr(stream, "cuda_stream"):
        raise ValueError(f"stream {stream!r}: an integer hipStream_t, an object with .cuda_stream, or None")
    return C.c_void_p(int(stream.cuda_stream) or None)


# mckpp_hip_put_dev / _put_host (MCKPP_PUT_* of mckpp_hip_put.h): the operations, the flag bits, the state fields
PUT_SET, PUT_ADD = 0, 1
PUT_SKIP, PUT_TIME_LEVELS = 1, 2
_PUT_OPS = {"set": PUT_SET, "add": PUT_ADD, PUT_SET: PUT_SET, PUT_ADD: PUT_ADD}
_PUT_FIELDS = {OUT["u"]: "u", OUT["v"]: "v", OUT["T"]: "T", OUT["S_anom"]: "S", OUT["S"]: "S"}   # field -> what it writes


def _host_plane(a, what, count):
    """(address, typestr) of the numpy array `a` handed to put_host: float64 or float32, C-contiguous, `count` elements.
    ValueError otherwise; an array in device memory is refused here."""
    if not isinstance(a, np.ndarray):
        kind = "an array in device memory" if hasattr(a, "__cuda_array_interface__") else "no numpy array"
        raise ValueError(f"{what}: {kind} ({type(a).__module__}.{type(a).__name__}); put_host takes numpy arrays (put_dev "
                         "takes arrays in device memory)")
    typestr = a.dtype.str
    if typestr not in _DEV_TYPESTR:
        raise ValueError(f"{what}: element type {typestr}, the call takes {' or '.join(_DEV_TYPESTR)}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{what}: not C-contiguous (shape {a.shape}, strides {a.strides})")
    if a.size != count:
        raise ValueError(f"{what}: shape {a.shape}, the call takes {count} elements")
    return a.ctypes.data, typestr


# mckpp_hip_records_reduce_dev / _host (MCKPP_RED_* of mckpp_hip_reduce.h): the reductions, the bits of `weighted`
RED_NONE, RED_SUM, RED_AVERAGE, RED_MIN, RED_MAX = range(5)
RED_W_LEVELS, RED_W_POINTS = 1, 2
_RED_OPS = {"none": RED_NONE, "sum": RED_SUM, "average": RED_AVERAGE, "min": RED_MIN, "max": RED_MAX}


def _red_op(op):
    if isinstance(op, str) and op in _RED_OPS:
        return _RED_OPS[op]
    if isinstance(op, (int, np.integer)) and not isinstance(op, bool) and 0 <= int(op) <= 4:
        return int(op)
    raise ValueError(f"reduction {op!r} (\"none\", \"sum\", \"average\", \"min\", \"max\", or RED_NONE .. RED_MAX)")


def host_reduce_tree(terms):
    """The sum of `terms` in the order the device reduces a domain in (include/mckpp_hip_reduce.h, c): what a run with
    one process per GPU calls on its gathered terms to get the double a single handle delivers.  No GPU."""
    a = np.ascontiguousarray(terms, dtype=np.float64).ravel()
    return float(_lib().mckpp_host_reduce_tree(a.ctypes.data_as(_dp), a.size))


class _DeviceArrays:
    """The device-array interface (include/mckpp_hip_device.h): forcing from arrays in device memory, output fields into
    them, ordered by events on the caller's stream and never by a host wait.  Arrays handed to fluxes_dev or
    flux_ring_put_dev must stay unchanged until a dev_fence on the stream that next writes them (fence=True queues it at
    once on `stream`), or until synchronize()."""

    def _hold_dev(self, obj):
        """Keep a device array referenced while the library's queued kernels may touch it: the last 64 handed over (a
        coupled loop makes fresh ones every interval, and the fence orders their reuse on the device; _hold would end
        such a loop's 64th call with release_host_arrays, which waits for the device)."""
        held = self.__dict__.setdefault("_dev_held", [])
        held.append(obj)
        del held[:-64]

    def _dev_fields(self, who, fields):
        """fields as the (void *)[8] the library takes: eight arrays of npts, or one of (8, npts)"""
        n = self._npts
        if not isinstance(fields, (list, tuple)):
            base, _ = _dev_array(fields, f"{who}: fields", 8 * n)
            ptrs = [base + 8 * n * m for m in range(8)]
        else:
            if len(fields) != 8:
                raise ValueError(f"{who}: {len(fields)} fields; a record is taux, tauy, swf, lwf, lhf, shf, rain, snow")
            ptrs = [_dev_array(a, f"{who}: fields[{m}]", n)[0] for m, a in enumerate(fields)]
        self._hold_dev(fields)
        return (C.c_void_p * 8)(*ptrs)

    def fluxes_dev(self, ntime, fields, l_rest=0, flsn=334000.0, el=2.5e6, stream=None, fence=True):
        """fluxes() with the eight fields in device memory, produced on `stream`: the library's stream waits for what
        `stream` has queued, on the device.  fence: `stream` then waits for the library's read, so that its next kernels
        may rewrite the arrays."""
        ptrs, s = self._dev_fields("fluxes_dev", fields), _dev_stream(stream)
        self._call("fluxes_dev", int(ntime), ptrs, int(l_rest), float(flsn), float(el), s)
        if fence:
            self._call("dev_fence", s)

    def flux_ring_put_dev(self, rec, fields, stream=None, fence=False):
        """flux_ring_put() from device arrays produced on `stream`; host puts and device puts may alternate."""
        ptrs, s = self._dev_fields("flux_ring_put_dev", fields), _dev_stream(stream)
        self._call("flux_ring_put_dev", int(rec), ptrs, s)
        if fence:
            self._call("dev_fence", s)

    def fetch_dev(self, planes, stream=None, land_value=1e20, fill_land=True):
        """Output fields as they stand on the device - window_fetch(field, OP_INSTANT)'s values - into device arrays, one
        launch for all planes; `stream` waits for the delivery on the device.  A plane is (field, out, lev0, nlev): levels
        lev0 .. lev0 + nlev - 1 (0-based) of the field into out, nlev * npts elements, points fastest - a tensor of shape
        (nlev, npts) - of float64 or float32; (field, out) is the levels from 0 that out has room for.  fill_land: the
        points that are no resident column get land_value, otherwise they keep what out held."""
        n, arr = self._npts, (_DevPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            if len(p) not in (2, 4):
                raise ValueError(f"fetch_dev: planes[{k}] is (field, out) or (field, out, lev0, nlev)")
            f, out = _win_field(p[0]), p[1]
            axis = 1 if f in _OUT_2D else self._nzp1
            if len(p) == 4:
                lev0, nlev = int(p[2]), int(p[3])
            else:
                shape = getattr(out, "shape", ())
                lev0, nlev = 0, (int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0)
            if lev0 < 0 or nlev < 1 or lev0 + nlev > axis:
                raise ValueError(f"fetch_dev: planes[{k}]: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, whose "
                                 f"axis has {axis}")
            ptr, typestr = _dev_array(out, f"fetch_dev: planes[{k}] out", nlev * n, tuple(_DEV_TYPESTR))
            arr[k] = _DevPlaneC(f, lev0, nlev, _DEV_TYPESTR[typestr], int(bool(fill_land)), float(land_value), ptr)
            self._hold_dev(out)
        self._call("fetch_dev", len(planes), arr, _dev_stream(stream))

    def records_dev(self, planes, stream=None, land_value=1e20, fill_land=True):
        """Completed records of output schedules - window_record_fetch's values - into device arrays, one launch for all
        planes (include/mckpp_hip_device_records.h); `stream` waits for the delivery on the device.  A plane is
        (sched, rec, field, op, out, lev0, nlev): op OP_MEAN / OP_MIN / OP_MAX / OP_LAST of `field` in record `rec` of
        schedule `sched`, levels lev0 .. lev0 + nlev - 1 (0-based) of the levels the schedule keeps, into out, nlev *
        npoints elements, points fastest - a tensor of shape (nlev, npoints), npoints the record's point axis - of
        float64 or float32; (sched, rec, field, op, out) is the levels from 0 that out has room for.  fill_land: the
        positions that are no row of the record get land_value, otherwise they keep what out held.  The delivery is on
        the context's stream: window_record_release and the next launch may follow at once."""
        arr = (_DevRecordPlaneC * max(1, len(planes)))()
        if len(planes) > 64:
            raise ValueError(f"records_dev: {len(planes)} planes, at most 64 in one call")
        for k, p in enumerate(planes):
            who = f"records_dev: planes[{k}]"
            if len(p) not in (5, 7):
                raise ValueError(f"{who} is (sched, rec, field, op, out) or (sched, rec, field, op, out, lev0, nlev)")
            sched, rec, op, out = int(p[0]), int(p[1]), int(p[3]), p[4]
            try:
                f = _win_check_fetch(self._scheds(), sched, p[2], op)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            if rec < 0:
                raise ValueError(f"{who}: record {rec}")
            zoom = self._scheds()[sched].zoom
            n, axis = zoom if zoom is not None else (self._npts, self._nzp1)
            if f in _OUT_2D:
                axis = 1
            if len(p) == 7:
                lev0, nlev = int(p[5]), int(p[6])
            else:
                shape = getattr(out, "shape", ())
                lev0, nlev = 0, (int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0)
            if lev0 < 0 or nlev < 1 or lev0 + nlev > axis:
                raise ValueError(f"{who}: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, of which output "
                                 f"schedule {sched} keeps {axis}")
            ptr, typestr = _dev_array(out, f"{who} out", nlev * n, tuple(_DEV_TYPESTR))
            arr[k] = _DevRecordPlaneC(sched, f, op, lev0, nlev, _DEV_TYPESTR[typestr], int(bool(fill_land)), rec,
                                      float(land_value), ptr)
            self._hold_dev(out)
        self._call("records_dev", len(planes), arr, _dev_stream(stream))

    def _put_table(self, who, planes, op, time_levels, skip, array):
        """the planes of put_dev / put_host as the table the library takes, after every check that needs no library;
        array(a, what, count) -> (address, typestr) is the form's own check of a plane's array"""
        if op not in _PUT_OPS or isinstance(op, bool):
            raise ValueError(f"{who}: op {op!r} (\"set\" or \"add\")")
        flags, skip_value = (PUT_TIME_LEVELS if time_levels else 0), 0.0
        if skip is not None:
            flags, skip_value = flags | PUT_SKIP, float(skip)
            if skip_value != skip_value:
                raise ValueError(f"{who}: skip is NaN, which no element compares equal to")
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{who}: {len(planes)} planes, at most 64 in one call")
        n, arr, seen = self._npts, (_PutPlaneC * max(1, len(planes)))(), []
        for k, p in enumerate(planes):
            if not 2 <= len(p) <= 4:
                raise ValueError(f"{who}: planes[{k}] is (field, array), (field, array, lev0) or (field, array, lev0, nlev)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: planes[{k}]: {e}") from None
            if f not in _PUT_FIELDS:
                raise ValueError(f"{who}: planes[{k}]: field {OUT_FIELDS[f]} is an output of the step, not state (u, v, T, "
                                 "S_anom, S)")
            a, lev0 = p[1], (int(p[2]) if len(p) > 2 else 0)
            if len(p) > 3:
                nlev = int(p[3])
            else:
                shape = getattr(a, "shape", ())
                nlev = int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0
            if lev0 < 0 or nlev < 1 or lev0 + nlev > self._nzp1:
                raise ValueError(f"{who}: planes[{k}]: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, whose axis "
                                 f"has {self._nzp1}")
            for j, (g, a0, a1) in enumerate(seen):
                if g == _PUT_FIELDS[f] and lev0 < a1 and a0 < lev0 + nlev:
                    raise ValueError(f"{who}: planes[{k}] and planes[{j}] write {g} at overlapping levels {lev0} .. "
                                     f"{lev0 + nlev - 1} and {a0} .. {a1 - 1}: the planes of a call have no order")
            seen.append((_PUT_FIELDS[f], lev0, lev0 + nlev))
            ptr, typestr = array(a, f"{who}: planes[{k}] array", nlev * n)
            arr[k] = _PutPlaneC(f, lev0, nlev, _DEV_TYPESTR[typestr], _PUT_OPS[op], flags, skip_value, ptr)
        return len(planes), arr

    def put_dev(self, planes, op="set", time_levels=False, skip=None, stream=None, fence=False):
        """U, V, T, S of the resident state set (op "set") or incremented ("add") in place from device arrays produced on
        `stream`, one launch for all planes (include/mckpp_hip_put.h): fetch_dev's inverse.  A plane is (field, array[,
        lev0[, nlev]]): the array's nlev * npts elements, points fastest - a tensor of shape (nlev, npts) - of float64 or
        float32, for levels lev0 .. lev0 + nlev - 1 (0-based) of field u, v, T, S_anom or S; lev0 defaults to 0, nlev to
        what the array holds.  time_levels: the two saved time levels of the field take the same operation.  skip: an
        element equal to this value leaves its state element untouched.  No two planes of a call may write the same
        levels of a field.  Nothing is cancelled: schedules, exports, rings and series stay as they are.  The arrays
        must stay unchanged until a dev_fence on the stream that next writes them (fence=True queues it on `stream`)."""
        planes = list(planes)
        n, arr = self._put_table("put_dev", planes, op, time_levels, skip,
                                 lambda a, what, count: _dev_array(a, what, count, tuple(_DEV_TYPESTR)))
        s = _dev_stream(stream)
        for p in planes:
            self._hold_dev(p[1])
        self._call("put_dev", n, arr, s)
        if fence:
            self._call("dev_fence", s)

    def put_host(self, planes, op="set", time_levels=False, skip=None):
        """put_dev from numpy arrays of float64 or float32, shape (nlev, npts); returns when the state is written."""
        n, arr = self._put_table("put_host", planes, op, time_levels, skip, _host_plane)
        self._call("put_host", n, arr)

    def reduce_weights(self, point_w=None, level_w=None, iface_w=None):
        """The weights of records_reduce_dev / _host (include/mckpp_hip_reduce.h): point_w, npts values by point number
        of the 3-D ordering; level_w, nzp1 values for fields on the level axis (hm, for a heat content); iface_w, nzp1
        for fields on the interface axis.  None: not set; a call replaces all three.  Every weight is finite and >= 0.
        The handle keeps them until they are replaced: upload and load_restart leave them alone."""
        ptrs = []
        for name, w, n in (("point_w", point_w, self._npts), ("level_w", level_w, self._nzp1), ("iface_w", iface_w, self._nzp1)):
            if w is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(w, dtype=np.float64)
            if a.ndim != 1 or a.size != n:
                raise ValueError(f"reduce_weights: {name} has shape {a.shape}, the call takes {n} values")
            ptrs.append(a)
        self._call("reduce_weights", *[None if a is None else a.ctypes.data_as(_dp) for a in ptrs])

    def _reduce_table(self, who, planes, land_value, array):
        """the planes of records_reduce_dev / _host as the table the library takes, after every check that needs no
        library; array(a, what, count) -> address is the form's own check of a plane's result array"""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{who}: {len(planes)} planes, at most 64 in one call")
        arr = (_ReducePlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            at = f"{who}: planes[{k}]"
            if len(p) not in (7, 8, 10):
                raise ValueError(f"{at} is (sched, rec, field, op, out, axis_op, domain_op[, weighted[, lev0, nlev]])")
            sched, rec, op, out = int(p[0]), int(p[1]), int(p[3]), p[4]
            try:
                f = _win_check_fetch(self._scheds(), sched, p[2], op)
                axis_op, domain_op = _red_op(p[5]), _red_op(p[6])
            except ValueError as e:
                raise ValueError(f"{at}: {e}") from None
            if rec < 0:
                raise ValueError(f"{at}: record {rec}")
            if axis_op == RED_NONE and domain_op == RED_NONE:
                raise ValueError(f"{at}: axis_op and domain_op are both none: a plane that is not reduced is records_dev's")
            weighted = int(p[7]) if len(p) > 7 else 0
            if weighted & ~3:
                raise ValueError(f"{at}: weighted {weighted} (RED_W_LEVELS 1, RED_W_POINTS 2)")
            zoom = self._scheds()[sched].zoom
            n, axis = zoom if zoom is not None else (self._npts, self._nzp1)
            if f in _OUT_2D:
                axis = 1
            lev0, nlev = (int(p[8]), int(p[9])) if len(p) == 10 else (0, axis)
            if lev0 < 0 or nlev < 1 or lev0 + nlev > axis:
                raise ValueError(f"{at}: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, of which output "
                                 f"schedule {sched} keeps {axis}")
            count = n if domain_op == RED_NONE else nlev if axis_op == RED_NONE else 1
            arr[k] = _ReducePlaneC(sched, f, op, lev0, nlev, axis_op, domain_op, weighted, rec, float(land_value),
                                   array(out, f"{at} out", count))
        return len(planes), arr

    def records_reduce_dev(self, planes, stream=None, land_value=1e20):
        """Completed records of output schedules reduced over their levels, their points or both, into device arrays
        (include/mckpp_hip_reduce.h states the arithmetic and its order); ordered like records_dev: `stream` waits for
        the delivery on the device, window_record_release and the next launch may follow at once.  A plane is (sched,
        rec, field, op, out, axis_op, domain_op[, weighted[, lev0, nlev]]): the plane records_dev names by sched, rec,
        field, op, lev0, nlev - default: every level the schedule keeps -, reduced by axis_op over its levels and by
        domain_op over its points ("none", "sum", "average", "min", "max" or RED_*; not both none), with the weights of
        reduce_weights where `weighted` has RED_W_LEVELS / RED_W_POINTS.  out: float64 in device memory - npoints
        elements (domain_op none), nlev (axis_op none), or one.  land_value: what an element without a row, or an
        average without weight, is."""
        held = []

        def array(a, what, count):
            held.append(a)
            return _dev_array(a, what, count)[0]

        n, arr = self._reduce_table("records_reduce_dev", planes, land_value, array)
        for a in held:
            self._hold_dev(a)
        self._call("records_reduce_dev", n, arr, _dev_stream(stream))

    def records_reduce_host(self, planes, land_value=1e20):
        """records_reduce_dev into numpy arrays of float64; returns when they hold the results."""
        def array(a, what, count):
            ptr, typestr = _host_plane(a, what, count)
            if typestr != "<f8":
                raise ValueError(f"{what}: element type {typestr}, the call takes <f8")
            return ptr

        n, arr = self._reduce_table("records_reduce_host", planes, land_value, array)
        self._call("records_reduce_host", n, arr)

    def dev_fence(self, stream=None):
        """`stream` waits, on the device, for every read of caller arrays this handle has queued so far."""
        self._call("dev_fence", _dev_stream(stream))


# the caller's vertical axes (MCKPP_VAXES, MCKPP_VAXIS_* of mckpp_hip_vaxis.h)
VAXES, VAXIS_LEVELS_MAX = 8, 1024
VAXIS_ABOVE, VAXIS_BELOW, VAXIS_BRACKET = 0, 1, 2
# output fields on the interface axis 0..nz, which no axis of heights like zm describes
_OUT_INTERFACE = frozenset(OUT[n] for n in ("wu", "wv", "wT", "wS", "wB", "wTnt", "difm", "dift", "difs"))


def host_vaxis_map(zs, zt):
    """(branch, kin, t, dz) of the vertical interpolation from the source levels zs onto the targets zt, both heights,
    strictly decreasing: mckpp_host_vaxis_map, the table a caller's axis carries (include/mckpp_hip_vaxis.h).  No GPU."""
    zs = np.ascontiguousarray(zs, dtype=np.float64).ravel()
    zt = np.ascontiguousarray(zt, dtype=np.float64).ravel()
    branch, kin = np.zeros(zt.size, dtype=np.int32), np.zeros(zt.size, dtype=np.int32)
    t, dz = np.zeros(zt.size), np.zeros(zt.size)
    rc = _lib().mckpp_host_vaxis_map(zs.size, zs.ctypes.data_as(_dp), zt.size, zt.ctypes.data_as(_dp), branch.ctypes.data_as(_ip),
                                     kin.ctypes.data_as(_ip), t.ctypes.data_as(_dp), dz.ctypes.data_as(_dp))
    if rc != 0:
        raise ValueError("host_vaxis_map: an axis has fewer than two source levels, no target, a value that is not finite, "
                         "or does not strictly decrease")
    return branch, kin, t, dz


class _VerticalAxes:
    """The caller's vertical axes (include/mckpp_hip_vaxis.h): state in, the reference's initial profiles and fields out
    on levels that are not the model's.  An array on axis a is (n_a, npts): points fastest, the whole axis."""

    def _vaxes(self):
        return self.__dict__.setdefault("_vaxis_n", {})

    def _vaxis(self, who, axis):
        """the number of levels of a defined axis"""
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or int(axis) not in self._vaxes():
            raise ValueError(f"{who}: axis {axis!r} is not defined (vaxis_define; axes are 0 .. {VAXES - 1})")
        return self._vaxes()[int(axis)]

    def vaxis_define(self, axis, z):
        """Caller axis `axis` (0 .. VAXES - 1): the heights z, at least two, finite and strictly decreasing like zm; None
        or an empty z drops the axis.  The handle keeps it over upload and load_restart."""
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= int(axis) < VAXES:
            raise ValueError(f"vaxis_define: axis {axis!r} (0 .. {VAXES - 1})")
        a = np.zeros(0) if z is None else np.ascontiguousarray(z, dtype=np.float64)
        if a.ndim != 1 or a.size == 1 or a.size > VAXIS_LEVELS_MAX:
            raise ValueError(f"vaxis_define: z has shape {a.shape}; an axis has 2 .. {VAXIS_LEVELS_MAX} levels (none drops it)")
        if not np.isfinite(a).all():
            raise ValueError("vaxis_define: z holds a value that is not finite")
        if a.size and not (a[1:] < a[:-1]).all():
            raise ValueError("vaxis_define: z does not strictly decrease (an axis holds heights, like zm)")
        self._call("vaxis_define", int(axis), a.size, a.ctypes.data_as(_dp))
        if a.size:
            self._vaxes()[int(axis)] = int(a.size)
        else:
            self._vaxes().pop(int(axis), None)

    def _vaxis_put_table(self, who, planes, op, time_levels, skip, array):
        """the planes of vaxis_put_dev / _put_host as the table the library takes, after every check that needs no library"""
        if op not in _PUT_OPS or isinstance(op, bool):
            raise ValueError(f"{who}: op {op!r} (\"set\" or \"add\")")
        flags, skip_value = (PUT_TIME_LEVELS if time_levels else 0), 0.0
        if skip is not None:
            flags, skip_value = flags | PUT_SKIP, float(skip)
            if skip_value != skip_value:
                raise ValueError(f"{who}: skip is NaN, which no element compares equal to")
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{who}: {len(planes)} planes, at most 64 in one call")
        n, arr, seen = self._npts, (_VaxisPutPlaneC * max(1, len(planes)))(), []
        for k, p in enumerate(planes):
            if len(p) != 3:
                raise ValueError(f"{who}: planes[{k}] is (field, axis, array)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: planes[{k}]: {e}") from None
            if f not in _PUT_FIELDS:
                raise ValueError(f"{who}: planes[{k}]: field {OUT_FIELDS[f]} is an output of the step, not state (u, v, T, "
                                 "S_anom, S)")
            nax = self._vaxis(f"{who}: planes[{k}]", p[1])
            if _PUT_FIELDS[f] in seen:
                raise ValueError(f"{who}: planes[{k}] and planes[{seen.index(_PUT_FIELDS[f])}] write {_PUT_FIELDS[f]}: a plane "
                                 "writes the whole profile, and the planes of a call have no order")
            seen.append(_PUT_FIELDS[f])
            ptr, typestr = array(p[2], f"{who}: planes[{k}] array", nax * n)
            arr[k] = _VaxisPutPlaneC(f, int(p[1]), _DEV_TYPESTR[typestr], _PUT_OPS[op], flags, skip_value, ptr)
        return len(planes), arr

    def vaxis_put_dev(self, planes, op="set", time_levels=False, skip=None, stream=None, fence=False):
        """put_dev from arrays on caller axes: a plane is (field, axis, array), the array's n_axis * npts elements - a
        tensor of shape (n_axis, npts) - of float64 or float32, and writes every model level of u, v, T, S_anom or S with
        the interpolated value (include/mckpp_hip_vaxis.h).  op, time_levels, stream and fence are put_dev's; skip: a
        model level stays untouched if an input value it is interpolated from equals this value."""
        planes = list(planes)
        n, arr = self._vaxis_put_table("vaxis_put_dev", planes, op, time_levels, skip,
                                       lambda a, what, count: _dev_array(a, what, count, tuple(_DEV_TYPESTR)))
        s = _dev_stream(stream)
        for p in planes:
            self._hold_dev(p[2])
        self._call("vaxis_put_dev", n, arr, s)
        if fence:
            self._call("dev_fence", s)

    def vaxis_put_host(self, planes, op="set", time_levels=False, skip=None):
        """vaxis_put_dev from numpy arrays of float64 or float32, shape (n_axis, npts); returns when the state is written."""
        n, arr = self._vaxis_put_table("vaxis_put_host", planes, op, time_levels, skip, _host_plane)
        self._call("vaxis_put_host", n, arr)

    def _vaxis_profiles(self, who, u, v, temp, sal, axis_vel, axis_temp, axis_sal, tk0, array):
        tk0 = float(tk0)
        if not np.isfinite(tk0):
            raise ValueError(f"{who}: tk0 is not finite")
        ptrs, types = [], set()
        for name, a, axis in (("u", u, axis_vel), ("v", v, axis_vel), ("temp", temp, axis_temp), ("sal", sal, axis_sal)):
            nax = self._vaxis(f"{who}: {name}", axis)
            ptr, typestr = array(a, f"{who}: {name}", nax * self._npts)
            ptrs.append(ptr)
            types.add(typestr)
        if len(types) != 1:
            raise ValueError(f"{who}: u, v, temp and sal have element types {sorted(types)}; the call takes one")
        return _VaxisProfilesC(int(axis_vel), int(axis_temp), int(axis_sal), _DEV_TYPESTR[types.pop()], tk0, *ptrs)

    def vaxis_init_profiles_dev(self, u, v, temp, sal, axis_vel, axis_temp, axis_sal, tk0=273.15, stream=None):
        """The reference's initial profiles (mckpp_initialize_ocean_profiles) from device arrays on caller axes: u, v on
        axis_vel, temp on axis_temp, sal on axis_sal, each (n_axis, npts) of one element type.  Writes U, V, U_init, T
        (less tk0 everywhere if any resident value lies strictly between 200 and 400), X2 = S - Sref, Sref, SSref,
        Tref and Ssurf of the resident columns; upload comes before it, init_ocean after.  Returns when it is done."""
        p = self._vaxis_profiles("vaxis_init_profiles_dev", u, v, temp, sal, axis_vel, axis_temp, axis_sal, tk0,
                                 lambda a, what, count: _dev_array(a, what, count, tuple(_DEV_TYPESTR)))
        self._call("vaxis_init_profiles_dev", C.byref(p), _dev_stream(stream))

    def vaxis_init_profiles_host(self, u, v, temp, sal, axis_vel, axis_temp, axis_sal, tk0=273.15):
        """vaxis_init_profiles_dev from numpy arrays."""
        p = self._vaxis_profiles("vaxis_init_profiles_host", u, v, temp, sal, axis_vel, axis_temp, axis_sal, tk0, _host_plane)
        self._call("vaxis_init_profiles_host", C.byref(p))

    def vaxis_fetch_dev(self, planes, stream=None, land_value=1e20, fill_land=True):
        """fetch_dev onto caller axes: a plane is (field, axis, out), out of n_axis * npts elements - a tensor of shape
        (n_axis, npts) - of float64 or float32, and takes the field as it stands, interpolated from the model's levels
        (include/mckpp_hip_vaxis.h).  Fields on the levels 1..nzp1 only: two-dimensional fields and those on the
        interface axis are refused.  stream, land_value and fill_land are fetch_dev's."""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"vaxis_fetch_dev: {len(planes)} planes, at most 64 in one call")
        n, arr = self._npts, (_VaxisDevPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"vaxis_fetch_dev: planes[{k}]"
            if len(p) != 3:
                raise ValueError(f"{who} is (field, axis, out)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            if f in _OUT_2D:
                raise ValueError(f"{who}: field {OUT_FIELDS[f]} is two-dimensional: it has no vertical axis to interpolate")
            if f in _OUT_INTERFACE:
                raise ValueError(f"{who}: field {OUT_FIELDS[f]} lives on the interface axis 0..nz, not on the levels a "
                                 "caller's axis is interpolated from")
            nax = self._vaxis(who, p[1])
            ptr, typestr = _dev_array(p[2], f"{who} out", nax * n, tuple(_DEV_TYPESTR))
            arr[k] = _VaxisDevPlaneC(f, int(p[1]), _DEV_TYPESTR[typestr], int(bool(fill_land)), float(land_value), ptr)
            self._hold_dev(p[2])
        self._call("vaxis_fetch_dev", len(planes), arr, _dev_stream(stream))


# the caller's horizontal grids (MCKPP_HGRIDS, MCKPP_HGRID_NORM_* of mckpp_hip_hgrid.h)
HGRIDS = 4
HGRID_NORM_NONE, HGRID_NORM_USED = 0, 1
_HGRID_NORMS = {"none": HGRID_NORM_NONE, "used": HGRID_NORM_USED}


class _HgridTable:
    """A weight table as the library takes it: the three CSR arrays of the right element types, kept alive, and the
    mckpp_hgrid_table_c that points at them.  `table` is a (ptr, idx, w) triple or anything with the CSR attributes
    indptr, indices and data (scipy is not needed).  Only the shapes are checked here: the values are the library's to
    check (mckpp_host_hgrid_check), so that its messages are the ones a caller sees."""

    def __init__(self, who, table, nrows):
        if hasattr(table, "indptr") and hasattr(table, "indices") and hasattr(table, "data"):
            table = (table.indptr, table.indices, table.data)
        if not isinstance(table, (tuple, list)) or len(table) != 3:
            raise ValueError(f"{who}: a table is a (ptr, idx, w) triple or an object with indptr, indices and data")
        self.ptr = np.ascontiguousarray(table[0], dtype=np.int64)
        self.idx = np.ascontiguousarray(table[1], dtype=np.int32)
        self.w = np.ascontiguousarray(table[2], dtype=np.float64)
        if self.ptr.ndim != 1 or self.ptr.size != nrows + 1:
            raise ValueError(f"{who}: ptr has shape {self.ptr.shape}; the table has {nrows} rows, so ptr has {nrows + 1} elements")
        if self.idx.ndim != 1 or self.w.ndim != 1 or self.idx.size != self.w.size:
            raise ValueError(f"{who}: idx has shape {self.idx.shape} and w {self.w.shape}; they hold an element per entry")
        if self.idx.size < int(self.ptr.max(initial=0)):
            raise ValueError(f"{who}: ptr names entry {int(self.ptr.max()) - 1}, idx and w hold {self.idx.size}")
        self.c = _HgridTableC(self.ptr.ctypes.data_as(_i64p), self.idx.ctypes.data_as(_ip), self.w.ctypes.data_as(_dp))


def host_hgrid_check(name, table, nrows, nsrc):
    """None if `table` of nrows rows over source indices 0 .. nsrc - 1 passes the checks of hgrid_define, else the
    refusal's text, which names the table, the row and the entry: mckpp_host_hgrid_check.  No GPU."""
    t = _HgridTable("host_hgrid_check", table, nrows)
    msg = C.create_string_buffer(256)
    rc = _lib().mckpp_host_hgrid_check(str(name).encode(), int(nrows), int(nsrc), C.byref(t.c), msg, 256)
    return None if rc == 0 else msg.value.decode()


def host_hgrid_apply(table, x, nrows, used=None, norm=None, fill=True, land_value=1e20, out=None):
    """One level through a weight table exactly as include/mckpp_hip_hgrid.h states the arithmetic:
    mckpp_host_hgrid_apply, the yardstick of the device's results.  x: the source values; used: per source index whether
    entries reading it are used (None: all); norm None: the in direction; "none" / "used": the out direction, where a
    row without a used entry gets land_value (fill) or keeps what `out` held.  Returns the nrows values.  No GPU."""
    t = _HgridTable("host_hgrid_apply", table, nrows)
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    if t.idx.size and (int(t.idx.min()) < 0 or int(t.idx.max()) >= x.size):
        raise ValueError(f"host_hgrid_apply: an index outside the {x.size} source values")
    u = None
    if used is not None:
        u = np.ascontiguousarray(used, dtype=np.uint8).ravel()
        if u.size != x.size:
            raise ValueError(f"host_hgrid_apply: used has {u.size} elements, x has {x.size}")
    res = np.zeros(nrows) if out is None else np.ascontiguousarray(out, dtype=np.float64).ravel().copy()
    if res.size != nrows:
        raise ValueError(f"host_hgrid_apply: out has {res.size} elements, the table has {nrows} rows")
    rc = _lib().mckpp_host_hgrid_apply(int(nrows), C.byref(t.c), x.ctypes.data_as(_dp), None if u is None else u.ctypes.data_as(_u8p),
                                       -1 if norm is None else _hgrid_norm("host_hgrid_apply", norm), int(bool(fill)),
                                       float(land_value), res.ctypes.data_as(_dp))
    if rc != 0:
        raise ValueError("host_hgrid_apply: refused")
    return res


def host_hgrid_slices(table, nrows, rows=None, keep=None):
    """(slice_off, len, idx, w): the device layout - a sliced ELL, 64 rows per slice - of the listed rows (None: all) of
    `table` without the entries whose source index `keep` (None: none dropped) does not mark:
    mckpp_host_hgrid_slices.  No GPU."""
    t = _HgridTable("host_hgrid_slices", table, nrows)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).ravel()
    if r is not None and r.size and (int(r.min()) < 0 or int(r.max()) >= nrows):
        raise ValueError(f"host_hgrid_slices: a listed row outside the table's {nrows}")
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8).ravel()
    if k is not None and t.idx.size and int(t.idx.max()) >= k.size:
        raise ValueError(f"host_hgrid_slices: keep has {k.size} elements, the table names index {int(t.idx.max())}")
    nlist = nrows if r is None else r.size
    off, ln = np.zeros((nlist + 63) // 64 + 1, dtype=np.int64), np.zeros(max(nlist, 1), dtype=np.int32)
    args = (nlist, None if r is None else r.ctypes.data_as(_i64p), C.byref(t.c), None if k is None else k.ctypes.data_as(_u8p),
            off.ctypes.data_as(_i64p), ln.ctypes.data_as(_ip))
    padded = int(_lib().mckpp_host_hgrid_slices(*args, None, None))
    if padded < 0:
        raise ValueError("host_hgrid_slices: refused")
    idx, w = np.zeros(max(padded, 1), dtype=np.int32), np.zeros(max(padded, 1))
    _lib().mckpp_host_hgrid_slices(*args, idx.ctypes.data_as(_ip), w.ctypes.data_as(_dp))
    return off, ln[:nlist], idx[:padded], w[:padded]


def _hgrid_norm(who, norm):
    if isinstance(norm, str) and norm in _HGRID_NORMS:
        return _HGRID_NORMS[norm]
    if isinstance(norm, (int, np.integer)) and not isinstance(norm, bool):
        return int(norm)   # (an unknown number is the library's to refuse, by planes[k])
    raise ValueError(f"{who}: norm {norm!r} (\"none\", \"used\", or HGRID_NORM_NONE, HGRID_NORM_USED)")


class _HorizontalGrids:
    """The caller's horizontal grids (include/mckpp_hip_hgrid.h): forcing in from arrays on a caller's grid and fields
    out onto it, by remap weights the caller brings as CSR tables.  An array on grid g is (n_g,) or (nlev, n_g)."""

    def _hgrids(self):
        return self.__dict__.setdefault("_hgrid_n", {})

    def _hgrid(self, who, grid):
        """the number of points of a defined grid"""
        if isinstance(grid, bool) or not isinstance(grid, (int, np.integer)) or int(grid) not in self._hgrids():
            raise ValueError(f"{who}: grid {grid!r} is not defined (hgrid_define; grids are 0 .. {HGRIDS - 1})")
        return self._hgrids()[int(grid)]

    def hgrid_define(self, grid, n, table_in=None, table_out=None):
        """Caller grid `grid` (0 .. HGRIDS - 1) of n points.  table_in (caller -> model): npts rows over the caller's
        points; table_out (model -> caller): n rows over the model's points; each a (ptr, idx, w) CSR triple or an object
        with indptr, indices and data, or None - that direction is then refused when used.  n = 0 drops the grid.  After
        the first upload or load_restart; the handle keeps the grid over later ones."""
        if isinstance(grid, bool) or not isinstance(grid, (int, np.integer)) or not 0 <= int(grid) < HGRIDS:
            raise ValueError(f"hgrid_define: grid {grid!r} (0 .. {HGRIDS - 1})")
        n = int(n)
        if n < 0:
            raise ValueError(f"hgrid_define: n={n}")
        if n and not self._npts:
            raise ValueError("hgrid_define: upload the state first: the tables are checked against the grid's size")
        tin = None if n == 0 or table_in is None else _HgridTable("hgrid_define: table_in", table_in, self._npts)
        tout = None if n == 0 or table_out is None else _HgridTable("hgrid_define: table_out", table_out, n)
        self._call("hgrid_define", int(grid), n, None if tin is None else C.byref(tin.c), None if tout is None else C.byref(tout.c))
        if n:
            self._hgrids()[int(grid)] = n
        else:
            self._hgrids().pop(int(grid), None)

    def hgrid_info(self, grid):
        """n, the entries (nnz_in, nnz_out; -1: no such table), the padded sizes of the device tables for the present
        resident state (padded_in, padded_out) and the longest row of either table, as a dict."""
        self._hgrid("hgrid_info", grid)
        info = (C.c_int64 * 6)()
        self._call("hgrid_info", int(grid), info)
        return dict(zip(("n", "nnz_in", "nnz_out", "padded_in", "padded_out", "longest_row"), (int(v) for v in info)))

    def _hgrid_fields(self, who, grid, fields):
        """fields as the (void *)[8] the library takes: eight arrays of n, or one of (8, n)"""
        n = self._hgrid(who, grid)
        if not isinstance(fields, (list, tuple)):
            base, _ = _dev_array(fields, f"{who}: fields", 8 * n)
            ptrs = [base + 8 * n * m for m in range(8)]
        else:
            if len(fields) != 8:
                raise ValueError(f"{who}: {len(fields)} fields; a record is taux, tauy, swf, lwf, lhf, shf, rain, snow")
            ptrs = [_dev_array(a, f"{who}: fields[{m}]", n)[0] for m, a in enumerate(fields)]
        self._hold_dev(fields)
        return (C.c_void_p * 8)(*ptrs)

    def hgrid_fluxes_dev(self, grid, ntime, fields, l_rest=0, flsn=334000.0, el=2.5e6, stream=None, fence=True):
        """fluxes_dev() with the eight fields on caller grid `grid` (n points each): every resident column's values are
        the sums of its row of the grid's in table."""
        ptrs, s = self._hgrid_fields("hgrid_fluxes_dev", grid, fields), _dev_stream(stream)
        self._call("hgrid_fluxes_dev", int(grid), int(ntime), ptrs, int(l_rest), float(flsn), float(el), s)
        if fence:
            self._call("dev_fence", s)

    def hgrid_flux_ring_put_dev(self, grid, rec, fields, stream=None, fence=False):
        """flux_ring_put_dev() likewise; host puts, device puts and remapped puts may alternate within one ring."""
        ptrs, s = self._hgrid_fields("hgrid_flux_ring_put_dev", grid, fields), _dev_stream(stream)
        self._call("hgrid_flux_ring_put_dev", int(grid), int(rec), ptrs, s)
        if fence:
            self._call("dev_fence", s)

    def hgrid_fetch_dev(self, planes, stream=None, norm="none", land_value=1e20, fill_land=True):
        """fetch_dev onto caller grids: a plane is (field, grid, out) or (field, grid, out, lev0, nlev), out of nlev * n
        elements - a tensor of shape (nlev, n) - of float64 or float32.  norm "none": a caller point's value is the
        weighted sum over the resident points of its row of the grid's out table; "used": divided by the sum of those
        weights.  A caller point with no resident point in its row gets land_value (fill_land), or keeps what out held."""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"hgrid_fetch_dev: {len(planes)} planes, at most 64 in one call")
        nrm = _hgrid_norm("hgrid_fetch_dev", norm)
        arr = (_HgridPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"hgrid_fetch_dev: planes[{k}]"
            if len(p) not in (3, 5):
                raise ValueError(f"{who} is (field, grid, out) or (field, grid, out, lev0, nlev)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            n, out = self._hgrid(who, p[1]), p[2]
            axis = 1 if f in _OUT_2D else self._nzp1
            if len(p) == 5:
                lev0, nlev = int(p[3]), int(p[4])
            else:
                shape = getattr(out, "shape", ())
                lev0, nlev = 0, (int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0)
            if lev0 < 0 or nlev < 1 or lev0 + nlev > axis:
                raise ValueError(f"{who}: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, whose axis has {axis}")
            ptr, typestr = _dev_array(out, f"{who} out", nlev * n, tuple(_DEV_TYPESTR))
            arr[k] = _HgridPlaneC(f, lev0, nlev, _DEV_TYPESTR[typestr], int(p[1]), nrm, int(bool(fill_land)), float(land_value), ptr)
            self._hold_dev(out)
        self._call("hgrid_fetch_dev", len(planes), arr, _dev_stream(stream))


class _Remap:
    """Records out and state in on the caller's horizontal grids (include/mckpp_hip_remap.h): records_dev and put_dev
    through the weight tables of hgrid_define.  An array on grid g is (n_g,) or (nlev, n_g)."""

    def remap_records_dev(self, planes, stream=None, norm="none", land_value=1e20, fill_land=True):
        """records_dev onto caller grids: a plane is (sched, rec, field, op, grid, out) or (sched, rec, field, op, grid,
        out, lev0, nlev) - op OP_MEAN / OP_MIN / OP_MAX / OP_LAST of `field` in record `rec` of schedule `sched`, levels
        lev0 .. lev0 + nlev - 1 of the levels the schedule keeps (default: from 0, as many as out has room for), into
        out, a tensor of shape (nlev, n) of float64 or float32 on grid `grid`.  A caller point's value is the weighted sum
        over the points of its row of the grid's out table that are rows of the record - the resident columns, or a
        zoom's listed resident columns -, with norm "used" divided by the sum of those weights; a caller point with no
        such point gets land_value (fill_land), or keeps what out held.  The delivery is on the context's stream:
        window_record_release and the next launch may follow at once."""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"remap_records_dev: {len(planes)} planes, at most 64 in one call")
        nrm = _hgrid_norm("remap_records_dev", norm)
        arr = (_RemapRecordPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"remap_records_dev: planes[{k}]"
            if len(p) not in (6, 8):
                raise ValueError(f"{who} is (sched, rec, field, op, grid, out) or (sched, rec, field, op, grid, out, lev0, nlev)")
            sched, rec, op, out = int(p[0]), int(p[1]), int(p[3]), p[5]
            try:
                f = _win_check_fetch(self._scheds(), sched, p[2], op)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            if rec < 0:
                raise ValueError(f"{who}: record {rec}")
            n = self._hgrid(who, p[4])
            zoom = self._scheds()[sched].zoom
            axis = 1 if f in _OUT_2D else (zoom[1] if zoom is not None else self._nzp1)
            shape = tuple(getattr(out, "shape", ()))
            if len(p) == 8:
                lev0, nlev = int(p[6]), int(p[7])
            else:
                lev0, nlev = 0, (int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0)
            if lev0 < 0 or nlev < 1 or lev0 + nlev > axis:
                raise ValueError(f"{who}: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, of which output "
                                 f"schedule {sched} keeps {axis}")
            if shape not in ((nlev, n), (nlev * n,)):
                raise ValueError(f"{who}: out has shape {shape}; {nlev} levels on grid {int(p[4])} are ({nlev}, {n})")
            ptr, typestr = _dev_array(out, f"{who} out", nlev * n, tuple(_DEV_TYPESTR))
            arr[k] = _RemapRecordPlaneC(sched, f, op, lev0, nlev, _DEV_TYPESTR[typestr], int(p[4]), nrm, int(bool(fill_land)),
                                        rec, float(land_value), ptr)
            self._hold_dev(out)
        self._call("remap_records_dev", len(planes), arr, _dev_stream(stream))

    def remap_put_dev(self, planes, op="set", time_levels=False, skip=None, stream=None, fence=False):
        """put_dev from caller grids: a plane is (field, grid, array) or (field, grid, array, lev0) - the array a tensor
        of shape (nlev, n) of float64 or float32 on grid `grid`, for levels lev0 .. lev0 + nlev - 1 of field u, v, T,
        S_anom or S.  Every resident column's value at a level is the sum of its row of the grid's in table over that
        level of the array; op, time_levels and the surface references are put_dev's.  skip: a state element is left
        untouched if any entry of its column's row reads this value at its level.  A resident column whose row is empty
        is left untouched.  Nothing is cancelled.  The arrays must stay unchanged until a dev_fence on the stream that
        next writes them (fence=True queues it on `stream`)."""
        who = "remap_put_dev"
        if op not in _PUT_OPS or isinstance(op, bool):
            raise ValueError(f"{who}: op {op!r} (\"set\" or \"add\")")
        flags, skip_value = (PUT_TIME_LEVELS if time_levels else 0), 0.0
        if skip is not None:
            flags, skip_value = flags | PUT_SKIP, float(skip)
            if skip_value != skip_value:
                raise ValueError(f"{who}: skip is NaN, which no element compares equal to")
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{who}: {len(planes)} planes, at most 64 in one call")
        arr, seen = (_RemapPutPlaneC * max(1, len(planes)))(), []
        for k, p in enumerate(planes):
            if len(p) not in (3, 4):
                raise ValueError(f"{who}: planes[{k}] is (field, grid, array) or (field, grid, array, lev0)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: planes[{k}]: {e}") from None
            if f not in _PUT_FIELDS:
                raise ValueError(f"{who}: planes[{k}]: field {OUT_FIELDS[f]} is an output of the step, not state (u, v, T, "
                                 "S_anom, S)")
            n, a, lev0 = self._hgrid(f"{who}: planes[{k}]", p[1]), p[2], (int(p[3]) if len(p) > 3 else 0)
            shape = tuple(getattr(a, "shape", ()))
            nlev = int(np.prod(shape, dtype=np.int64)) // n if n and len(shape) else 0
            if lev0 < 0 or nlev < 1 or lev0 + nlev > self._nzp1:
                raise ValueError(f"{who}: planes[{k}]: levels {lev0} .. {lev0 + nlev - 1} of field {OUT_FIELDS[f]}, whose axis "
                                 f"has {self._nzp1}")
            if shape not in ((nlev, n), (nlev * n,)):
                raise ValueError(f"{who}: planes[{k}]: the array has shape {shape}; levels on grid {int(p[1])} are (nlev, {n})")
            for j, (g, a0, a1) in enumerate(seen):
                if g == _PUT_FIELDS[f] and lev0 < a1 and a0 < lev0 + nlev:
                    raise ValueError(f"{who}: planes[{k}] and planes[{j}] write {g} at overlapping levels {lev0} .. "
                                     f"{lev0 + nlev - 1} and {a0} .. {a1 - 1}: the planes of a call have no order")
            seen.append((_PUT_FIELDS[f], lev0, lev0 + nlev))
            ptr, typestr = _dev_array(a, f"{who}: planes[{k}] array", nlev * n, tuple(_DEV_TYPESTR))
            arr[k] = _RemapPutPlaneC(f, lev0, nlev, _DEV_TYPESTR[typestr], _PUT_OPS[op], flags, int(p[1]), skip_value, ptr)
        s = _dev_stream(stream)
        for p in planes:
            self._hold_dev(p[2])
        self._call("remap_put_dev", len(planes), arr, s)
        if fence:
            self._call("dev_fence", s)


class _GridAxis:
    """A caller grid and a caller axis in one call (include/mckpp_hip_hv.h): fields out and state in on points and levels
    that are both not the model's, through the tables of hgrid_define and vaxis_define.  An array on grid g and axis a
    is (n_a, n_g): points fastest, the whole axis."""

    def hv_fetch_dev(self, planes, stream=None, norm="none", land_value=1e20, fill_land=True):
        """fetch_dev onto a caller grid and a caller axis: a plane is (field, grid, axis, out), out a tensor of shape
        (n_axis, n_grid) of float64 or float32.  Vertical first: every resident column's profile is interpolated onto
        the axis as vaxis_fetch_dev does; then every caller point's value at a caller level is hgrid_fetch_dev's of those
        - norm, land_value and fill_land are its.  Two-dimensional fields and those on the interface axis are refused."""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"hv_fetch_dev: {len(planes)} planes, at most 64 in one call")
        nrm = _hgrid_norm("hv_fetch_dev", norm)
        arr = (_HvPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"hv_fetch_dev: planes[{k}]"
            if len(p) != 4:
                raise ValueError(f"{who} is (field, grid, axis, out)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
            if f in _OUT_2D:
                raise ValueError(f"{who}: field {OUT_FIELDS[f]} is two-dimensional: it has no vertical axis to interpolate")
            if f in _OUT_INTERFACE:
                raise ValueError(f"{who}: field {OUT_FIELDS[f]} lives on the interface axis 0..nz, not on the levels a "
                                 "caller's axis is interpolated from")
            n, nax, out = self._hgrid(who, p[1]), self._vaxis(who, p[2]), p[3]
            shape = tuple(getattr(out, "shape", ()))
            if shape not in ((nax, n), (nax * n,)):
                raise ValueError(f"{who}: out has shape {shape}; axis {int(p[2])} on grid {int(p[1])} is ({nax}, {n})")
            ptr, typestr = _dev_array(out, f"{who} out", nax * n, tuple(_DEV_TYPESTR))
            arr[k] = _HvPlaneC(f, int(p[2]), _DEV_TYPESTR[typestr], int(p[1]), nrm, int(bool(fill_land)), float(land_value), ptr)
            self._hold_dev(out)
        self._call("hv_fetch_dev", len(planes), arr, _dev_stream(stream))

    def hv_put_dev(self, planes, op="set", time_levels=False, skip=None, stream=None, fence=False):
        """put_dev from a caller grid and a caller axis: a plane is (field, grid, axis, array), the array a tensor of
        shape (n_axis, n_grid) of float64 or float32, and writes every model level of u, v, T, S_anom or S.  Horizontal
        first: a resident column's value at a caller level is the sum of its row of the grid's in table over that level
        of the array; the model levels are then interpolated from those sums as vaxis_put_dev does.  op, time_levels,
        stream and fence are put_dev's.  skip: a state element stays untouched if any entry of its column's row reads
        this value at a caller level its model level is interpolated from.  A resident column whose row is empty is
        left untouched.  Nothing is cancelled."""
        who = "hv_put_dev"
        if op not in _PUT_OPS or isinstance(op, bool):
            raise ValueError(f"{who}: op {op!r} (\"set\" or \"add\")")
        flags, skip_value = (PUT_TIME_LEVELS if time_levels else 0), 0.0
        if skip is not None:
            flags, skip_value = flags | PUT_SKIP, float(skip)
            if skip_value != skip_value:
                raise ValueError(f"{who}: skip is NaN, which no element compares equal to")
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{who}: {len(planes)} planes, at most 64 in one call")
        arr, seen = (_HvPutPlaneC * max(1, len(planes)))(), []
        for k, p in enumerate(planes):
            if len(p) != 4:
                raise ValueError(f"{who}: planes[{k}] is (field, grid, axis, array)")
            try:
                f = _win_field(p[0])
            except ValueError as e:
                raise ValueError(f"{who}: planes[{k}]: {e}") from None
            if f not in _PUT_FIELDS:
                raise ValueError(f"{who}: planes[{k}]: field {OUT_FIELDS[f]} is an output of the step, not state (u, v, T, "
                                 "S_anom, S)")
            n, nax, a = self._hgrid(f"{who}: planes[{k}]", p[1]), self._vaxis(f"{who}: planes[{k}]", p[2]), p[3]
            if _PUT_FIELDS[f] in seen:
                raise ValueError(f"{who}: planes[{k}] and planes[{seen.index(_PUT_FIELDS[f])}] write {_PUT_FIELDS[f]}: a plane "
                                 "writes the whole profile, and the planes of a call have no order")
            seen.append(_PUT_FIELDS[f])
            shape = tuple(getattr(a, "shape", ()))
            if shape not in ((nax, n), (nax * n,)):
                raise ValueError(f"{who}: planes[{k}]: the array has shape {shape}; axis {int(p[2])} on grid {int(p[1])} is "
                                 f"({nax}, {n})")
            ptr, typestr = _dev_array(a, f"{who}: planes[{k}] array", nax * n, tuple(_DEV_TYPESTR))
            arr[k] = _HvPutPlaneC(f, int(p[2]), _DEV_TYPESTR[typestr], _PUT_OPS[op], flags, int(p[1]), skip_value, ptr)
        s = _dev_stream(stream)
        for p in planes:
            self._hold_dev(p[3])
        self._call("hv_put_dev", len(planes), arr, s)
        if fence:
            self._call("dev_fence", s)


def host_vrecords_rule(branch, kin, lev0, nlev):
    """Does an axis whose out table is (branch, kin) - host_vaxis_map(zm, z)'s - read kept model levels only, the kept
    levels being lev0 .. lev0 + nlev - 1?  None if so, else (caller level, model level): the first caller level that reads
    a level outside them and the first such level it reads.  mckpp_host_vrecords_rule
    (include/mckpp_hip_vrecords.h).  No GPU."""
    branch = np.ascontiguousarray(branch, dtype=np.int32).ravel()
    kin = np.ascontiguousarray(kin, dtype=np.int32).ravel()
    j, lev = C.c_int32(-1), C.c_int32(-1)
    rc = _lib().mckpp_host_vrecords_rule(branch.size if branch.size == kin.size else 0, branch.ctypes.data_as(_ip),
                                         kin.ctypes.data_as(_ip), int(lev0), int(nlev), C.byref(j), C.byref(lev))
    if rc < 0:
        raise ValueError("host_vrecords_rule: branch and kin are one table of at least one caller level, and nlev >= 1")
    return None if rc == 0 else (int(j.value), int(lev.value))


class _AxisRecords:
    """Completed records of output schedules on a caller axis (include/mckpp_hip_vrecords.h): records_dev and
    remap_records_dev through the out table of vaxis_define.  Record value first - a mean divided by the period -, then
    the vertical interpolation, then - on a caller grid - the row sum.  An array is (n_axis, npoints) or (n_axis, n_grid):
    points fastest, the whole axis."""

    def _axis_record(self, who, p, naxis):
        """what a plane tuple (sched, rec, field, op, ...) says of its record, its field and its axis, checked:
        (sched, rec, field, op, axis, n_axis, npoints of the schedule's records)"""
        sched, rec, op = int(p[0]), int(p[1]), int(p[3])
        try:
            f = _win_field(p[2])
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if f in _OUT_2D:
            raise ValueError(f"{who}: field {OUT_FIELDS[f]} is two-dimensional: it has no vertical axis to interpolate")
        if f in _OUT_INTERFACE:
            raise ValueError(f"{who}: field {OUT_FIELDS[f]} lives on the interface axis 0..nz, not on the levels a "
                             "caller's axis is interpolated from")
        try:
            _win_check_fetch(self._scheds(), sched, f, op)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if rec < 0:
            raise ValueError(f"{who}: record {rec}")
        zoom = self._scheds()[sched].zoom
        return sched, rec, f, op, int(naxis), self._vaxis(who, naxis), (zoom[0] if zoom is not None else self._npts)

    def _vaxis_record_table(self, name, planes, land_value, fill_land, array):
        """the planes of vaxis_records_dev / _host as the table the library takes; array(a, what, count) ->
        (address, typestr) is the form's own check of a plane's array"""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"{name}: {len(planes)} planes, at most 64 in one call")
        arr = (_VaxisRecordPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"{name}: planes[{k}]"
            if len(p) != 6:
                raise ValueError(f"{who} is (sched, rec, field, op, axis, out)")
            sched, rec, f, op, axis, nax, n = self._axis_record(who, p, p[4])
            out = p[5]
            shape = tuple(getattr(out, "shape", ()))
            if hasattr(out, "shape") and shape not in ((nax, n), (nax * n,)):
                raise ValueError(f"{who}: out has shape {shape}; axis {axis} at the {n} points of schedule {sched}'s records "
                                 f"is ({nax}, {n})")
            ptr, typestr = array(out, f"{who} out", nax * n)
            arr[k] = _VaxisRecordPlaneC(sched, f, op, axis, _DEV_TYPESTR[typestr], int(bool(fill_land)), rec,
                                        float(land_value), ptr)
        return len(planes), arr

    def vaxis_records_dev(self, planes, stream=None, land_value=1e20, fill_land=True):
        """records_dev onto caller axes: a plane is (sched, rec, field, op, axis, out) - op OP_MEAN / OP_MIN / OP_MAX /
        OP_LAST of the three-dimensional `field` in record `rec` of schedule `sched`, interpolated from the model levels
        the schedule keeps onto axis `axis`, into out, a tensor of shape (n_axis, npoints) of float64 or float32, npoints
        the record's point axis.  The record's value comes first (the mean is sum / period), the interpolation second:
        a record of minima gives the interpolation of the minima.  A schedule with a level zoom serves an axis whose
        every caller level reads kept levels only; the library refuses any other by name.  land_value, fill_land and
        the ordering are records_dev's: window_record_release and the next launch may follow at once."""
        held = []

        def array(a, what, count):
            held.append(a)
            return _dev_array(a, what, count, tuple(_DEV_TYPESTR))

        n, arr = self._vaxis_record_table("vaxis_records_dev", planes, land_value, fill_land, array)
        for a in held:
            self._hold_dev(a)
        self._call("vrecords_vaxis_dev", n, arr, _dev_stream(stream))

    def vaxis_records_host(self, planes, land_value=1e20, fill_land=True):
        """vaxis_records_dev into numpy arrays of float64 or float32; returns when they hold the planes (XIOS's
        interpolate_axis for a host output path)."""
        def array(a, what, count):
            ptr, typestr = _host_plane(a, what, count)
            self._hold(a)     # (the library pins the arrays it copies into, as window_record_fetch's)
            return ptr, typestr

        n, arr = self._vaxis_record_table("vaxis_records_host", planes, land_value, fill_land, array)
        self._call("vrecords_vaxis_host", n, arr)

    def hv_records_dev(self, planes, stream=None, norm="none", land_value=1e20, fill_land=True):
        """remap_records_dev onto caller axes: a plane is (sched, rec, field, op, grid, axis, out), out a tensor of shape
        (n_axis, n_grid) of float64 or float32.  Vertical first, at the record's rows, as vaxis_records_dev does; then every
        caller point's value at a caller level is remap_records_dev's of those - the used entries are the rows of the
        record, norm, land_value and fill_land are hgrid_fetch_dev's."""
        planes = list(planes)
        if len(planes) > 64:
            raise ValueError(f"hv_records_dev: {len(planes)} planes, at most 64 in one call")
        nrm = _hgrid_norm("hv_records_dev", norm)
        arr = (_HvRecordPlaneC * max(1, len(planes)))()
        for k, p in enumerate(planes):
            who = f"hv_records_dev: planes[{k}]"
            if len(p) != 7:
                raise ValueError(f"{who} is (sched, rec, field, op, grid, axis, out)")
            sched, rec, f, op, axis, nax, _ = self._axis_record(who, p, p[5])
            n, out = self._hgrid(who, p[4]), p[6]
            shape = tuple(getattr(out, "shape", ()))
            if shape not in ((nax, n), (nax * n,)):
                raise ValueError(f"{who}: out has shape {shape}; axis {axis} on grid {int(p[4])} is ({nax}, {n})")
            ptr, typestr = _dev_array(out, f"{who} out", nax * n, tuple(_DEV_TYPESTR))
            arr[k] = _HvRecordPlaneC(sched, f, op, axis, _DEV_TYPESTR[typestr], int(p[4]), nrm, int(bool(fill_land)), rec,
                                     float(land_value), ptr)
            self._hold_dev(out)
        self._call("vrecords_hv_dev", len(planes), arr, _dev_stream(stream))


class _Handle(_WindowSchedules, _RestartSchedule, _StepLog, _AncillarySeries, _FluxRing, _DeviceArrays, _VerticalAxes,
              _HorizontalGrids, _Remap, _GridAxis, _AxisRecords):
    """What one device context and several GPUs behind one handle have in common: everything but how they are made.
    Method `name` is the C function self._pre + name applied to the handle self._h."""
    _pre = "mckpp_hip_"
    _npts = 0   # points of the resident state (3-D ordering, land included); 0 before upload / load_restart
    _nzp1 = 0   # grid points of a column (the vertical axis of the 3-D output fields)

    def _open(self, kpp_const_fields, *args):
        self._nzp1 = int(kpp_const_fields.nzp1)
        self._h = C.c_void_p()
        # The library pins (hipHostRegister) every large host array it transfers from or into and keeps the
        # registration until release_host_arrays() / close(): an array must not be freed while it is registered (a new
        # array at the same address would be transferred through stale page mappings).  So every array - or object
        # holding arrays - handed to upload / download / set_forcing / gather / window_fetch stays referenced here
        # for exactly that long.
        self._held = {}
        cc = kpp_const_fields.as_c()   # (the library copies what it points to: the constants are not kept)
        _chk(getattr(_lib(), self._pre + "init")(C.byref(cc), *args, C.byref(self._h)))

    def _raw(self, name, *args):
        """self._pre + name on the handle: what it returns."""
        return getattr(_lib(), self._pre + name)(self._h, *args)

    def _call(self, name, *args):
        """self._pre + name on the handle; a non-zero return code raises MckppHipError with the library's text."""
        _chk(self._raw(name, *args))

    def _hold(self, obj):
        """Keep `obj` referenced while the library may have it pinned.  Arrays are keyed by their address range (the
        library pins arrays of at least 256 KiB only: smaller ones are not kept), objects holding arrays by identity;
        a loop that hands over fresh arrays step after step is bounded: at 64 entries everything is unpinned and
        released first (a caller that wants no re-pinning reuses its arrays, or calls release_host_arrays() itself)."""
        if isinstance(obj, np.ndarray):
            if obj.nbytes < 256 * 1024:
                return
            key = (obj.ctypes.data, obj.nbytes)
        else:
            key = id(obj)
        if key not in self._held and len(self._held) >= 64:
            self.release_host_arrays()
        self._held[key] = obj

    def close(self):
        if self._h:
            self._raw("finalize")
            self._h = C.c_void_p()
        self._held = {}
        self.__dict__.pop("_dev_held", None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_host_arrays(self):
        """Un-pin the caller's arrays this handle registered (before they are freed while the handle lives);
        the references this object holds on them go with the registrations."""
        self._call("release_host_arrays")
        self._held = {}

    def _new_state(self, npts):
        """after upload / load_restart: they cancel every output schedule, the restart schedule and the step log"""
        self._npts = npts
        self._scheds().clear()
        self.restart_scheduled = None
        self.step_logged = None

    def upload(self, kpp_3d_fields):
        self._hold(kpp_3d_fields)
        s = kpp_3d_fields.as_c()
        self._call("upload", C.byref(s))
        self._new_state(kpp_3d_fields.npts)

    def download(self, kpp_3d_fields, mask=F_ALL):
        self._hold(kpp_3d_fields)
        s = kpp_3d_fields.as_c()
        self._call("download", C.byref(s), int(mask))

    def update_ancillaries(self, kpp_3d_fields):
        """Re-upload what mckpp_boundary_update rewrites between steps (optional-physics inputs only)."""
        self._hold(kpp_3d_fields)
        s = kpp_3d_fields.as_c()
        self._call("update_ancillaries", C.byref(s))

    def save_restart(self, path):
        """The restart set into `path` (a multi handle: one file per shard, <path>.<shard>of<ndev>)."""
        self._call("save_restart", str(path).encode())

    def load_restart(self, path, npts=None):
        """The restart set of save_restart.  npts: the points of the state the file was written from, for a handle that
        has had no upload of as many points (a multi handle needs that upload anyway: it deals the columns)."""
        self._call("load_restart", str(path).encode())
        self._new_state(self._npts if npts is None else npts)

    def set_forcing(self, sflux):
        assert sflux.flags["F_CONTIGUOUS"]
        self._hold(sflux)
        self._call("set_forcing", sflux.ctypes.data_as(_dp))

    def fluxes(self, ntime, taux, tauy, swf, lwf, lhf, shf, rain, snow, l_rest=0, flsn=334000.0, el=2.5e6):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (taux, tauy, swf, lwf, lhf, shf, rain, snow)]
        self._call("fluxes", int(ntime), *[a.ctypes.data_as(_dp) for a in arrs], int(l_rest), float(flsn), float(el))

    def set_flux_series(self, rec0, fields):
        """fields[nrec, 8, npts]: taux, tauy, swf, lwf, lhf, shf, rain, snow at successive flux updates; record 0 of the
        array is flux update rec0 of the run."""
        f = np.ascontiguousarray(fields, dtype=np.float64)
        assert f.ndim == 3 and f.shape[1] == 8 and f.shape[2] == self._npts
        self._hold(f)
        self._call("set_flux_series", int(rec0), int(f.shape[0]), f.ctypes.data_as(_dp))

    def run_forced(self, nt_first, nsteps, ndtocn, l_rest=0, flsn=334000.0, el=2.5e6):
        self._call("run_forced", int(nt_first), int(nsteps), int(ndtocn), int(l_rest), float(flsn), float(el))

    def bottomtemp(self, bottom_temp):
        bt = np.ascontiguousarray(bottom_temp, dtype=np.float64)
        assert bt.shape == (self._npts,)
        self._call("bottomtemp", bt.ctypes.data_as(_dp))

    def set_bottomtemp(self, bottom_temp):
        """bottom_temp(npts) becomes resident: from now on every step launch ends each column-step with the
        L_VARY_BOTTOM_TEMP override (src/mckpp_physics_overrides.F90:12-24); None cancels it.  Do not also call
        bottomtemp(): it is refused while a field is resident."""
        if bottom_temp is None:
            self._call("set_bottomtemp", None)
            return
        bt = np.ascontiguousarray(bottom_temp, dtype=np.float64)
        assert bt.shape == (self._npts,)
        self._call("set_bottomtemp", bt.ctypes.data_as(_dp))

    def window_reset(self):
        self._call("window_reset")

    def window_accumulate(self):
        self._call("window_accumulate")

    def window_select(self, fields):
        """Choose the OUT_* fields window_accumulate reduces (resets the window)."""
        f = np.ascontiguousarray(fields, dtype=np.int32)
        self._call("window_select", f.ctypes.data_as(_ip), len(f))

    def window_fetch(self, field, op, out):
        assert out.flags["F_CONTIGUOUS"] and out.dtype == np.float64
        self._hold(out)
        self._call("window_fetch", int(field), int(op), out.ctypes.data_as(_dp))
        return out

    def set_diagnostics(self, on):
        self._call("set_diagnostics", int(on))

    def set_solver_mode(self, mode):
        """0: tridmat's order of operations (default); 1: two-ended elimination (mckpp_hip_set_solver_mode)."""
        self._call("set_solver_mode", int(mode))

    def init_ocean(self, ntime=0):
        self._call("init_ocean", int(ntime))

    def step(self, ntime, nsteps=1):
        self._call("step", int(ntime), int(nsteps))

    def synchronize(self):
        self._call("synchronize")

    def status(self):
        st = np.zeros(self._npts, dtype=np.int32)
        npass = np.zeros(self._npts, dtype=np.int32)
        nf = C.c_int64(0)
        self._call("status", st.ctypes.data_as(_ip), C.byref(nf), npass.ctypes.data_as(_ip))
        return st, int(nf.value), npass

    @property
    def ncolumns(self):
        return int(self._raw("ncolumns"))


class MckppHip(_Handle):
    """One device context (mckpp_hip_init ... mckpp_hip_finalize)."""

    def __init__(self, kpp_const_fields, device=0):
        self._open(kpp_const_fields, int(device))

    @property
    def solver_mode(self):
        return int(self._raw("get_solver_mode"))

    def vmix_pass(self, ntime):
        self._call("vmix_pass", int(ntime))

    def vmix_only(self, ntime):
        self._call("vmix_only", int(ntime))

    def last_kernel_ms(self):
        ms = C.c_double(0)
        nl = C.c_int32(0)
        self._call("last_kernel_ms", C.byref(ms), C.byref(nl))
        return ms.value, nl.value

    def last_launch_count(self):
        """kernel launches of the last step/init/vmix_pass call (step(nt, n > 1) is one launch for all n steps)"""
        return int(self._raw("last_launch_count"))

    def kernel_residency(self):
        """(blocks per CU asked for, blocks per CU that fit, threads per block, LDS bytes per block)"""
        b, m, t = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        l = C.c_int64(0)
        self._call("kernel_residency", C.byref(b), C.byref(m), C.byref(t), C.byref(l))
        return b.value, m.value, t.value, l.value

    @property
    def kernel_name(self):
        return self._raw("kernel_name").decode()

    def eos_batch(self, s, t, p):
        n = len(s)
        out = [np.zeros(n) for _ in range(4)]
        self._call("eos_batch", n, *[np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_dp) for a in (s, t, p)],
                   *[o.ctypes.data_as(_dp) for o in out])
        return out

    def div_batch(self, num, den):
        num = np.ascontiguousarray(num, dtype=np.float64)
        den = np.ascontiguousarray(den, dtype=np.float64)
        q = np.zeros((4, len(num)))
        self._call("div_batch", len(num), num.ctypes.data_as(_dp), den.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
        return q

    def exp_batch(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._call("exp_batch", len(x), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp))
        return y


class MckppHipMulti(_Handle):
    """Several GPUs behind one handle (mckpp_hip_multi_*): columns dealt round-robin to the devices."""
    _pre = "mckpp_hip_multi_"

    def __init__(self, kpp_const_fields, devices):
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self._open(kpp_const_fields, len(dev), dev.ctypes.data_as(_ip))

    def gather(self, field, root, out):
        """field 0 U, 1 V, 2 T, 3 S -> out(npts, nzp1) Fortran order; 4 hmix -> out(npts)."""
        assert out.flags["F_CONTIGUOUS"] and out.dtype == np.float64
        self._hold(out)
        self._call("gather", int(field), int(root), out.ctypes.data_as(_dp))


def host_shard_mask(run_physics, ndev, dev):
    """run_physics mask of shard dev of ndev (mckpp_host_shard_mask; host only)."""
    rp = np.ascontiguousarray(run_physics, dtype=np.int32)
    out = np.zeros(len(rp), dtype=np.int32)
    n = _lib().mckpp_host_shard_mask(len(rp), rp.ctypes.data_as(_ip), int(ndev), int(dev), out.ctypes.data_as(_ip))
    if n < 0:
        raise MckppHipError("mckpp_host_shard_mask: bad arguments")
    return out, int(n)


# ---------------------------------------------------------------------------
# The reference's call surface.  The reference operates on module globals; the
# Python mirror passes them explicitly and keeps the device context on the
# const-fields object (one context per kpp_const_fields, created on first use;
# the context holds no reference back, so it dies with its constants).
# ---------------------------------------------------------------------------
def _ctx(kpp_3d_fields, kpp_const_fields, device=0):
    ctx = getattr(kpp_const_fields, "_hip_ctx", None)
    if ctx is None:
        ctx = MckppHip(kpp_const_fields, device)
        kpp_const_fields._hip_ctx = ctx
        ctx._resident = None
    if ctx._resident is not kpp_3d_fields:
        ctx.upload(kpp_3d_fields)
        ctx._resident = kpp_3d_fields
    return ctx


def mckpp_initialize_ocean_model(kpp_3d_fields, kpp_const_fields, ntime=0, device=0, download=True):
    """src/mckpp_initialize_ocean.F90:18 (tri() is already set by KppConstFields)."""
    ctx = _ctx(kpp_3d_fields, kpp_const_fields, device)
    ctx.init_ocean(ntime)
    if download:
        ctx.download(kpp_3d_fields, F_ALL)
    return ctx


def mckpp_physics_driver(kpp_3d_fields, kpp_const_fields, ntime, device=0, download=True, new_forcing=True):
    """src/mckpp_physics_driver_mod.F90:15 - one ocnstep + check_profile per run_physics column."""
    ctx = _ctx(kpp_3d_fields, kpp_const_fields, device)
    if new_forcing:
        ctx.set_forcing(kpp_3d_fields.sflux)
    ctx.step(ntime, 1)
    if kpp_const_fields.L_VARY_BOTTOM_TEMP:     # src/mckpp_physics_driver_mod.F90:67-71
        ctx.bottomtemp(kpp_3d_fields.bottom_temp)
    if download:
        ctx.download(kpp_3d_fields, F_ALL)
    return ctx
