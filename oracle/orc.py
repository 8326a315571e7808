"""ctypes front-end for the CPU oracle (oracle/liboracle.so) and, when built,
the compiled reference pieces (oracle/_ref/libmckpp_ref.so: EOS, cpsw, z121;
oracle/_ref/libmckpp_ref_step{,_pexp}.so: the reference's whole physics step, and its
own init, flux assembly and time loop served from an in-memory flux file).

TEST INFRASTRUCTURE ONLY: imported by tests/, bench.py's cpu_baseline leg and
__graft_entry__.smoke().  The product package never imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MCKPP_ORACLE_LIBRARY names another build of the oracle (the instrumented one of tools/oracle_coverage.py)
LIB = os.environ.get("MCKPP_ORACLE_LIBRARY") or os.path.join(HERE, "liboracle.so")
REFLIB = os.path.join(HERE, "_ref", "libmckpp_ref.so")
REFSTEPLIB = {0: os.path.join(HERE, "_ref", "libmckpp_ref_step.so"),        # EXP = libm exp (the reference's build)
              1: os.path.join(HERE, "_ref", "libmckpp_ref_step_pexp.so")}  # EXP = the portable exp (exp_mode=1)

NI, NJ = 890, 48
TABLE_SHAPE = (NJ + 2, NI + 2)  # C-order view of Fortran wmt(0:891,0:49)

ST_ZERO_PIVOT, ST_LONG_ITER, ST_RETRIED, ST_FAILED, ST_DODGY = 1, 2, 4, 8, 16
# bits of a batch's `paths` word (ORC_PATH_* of mckpp_oracle.h): which branches a column took during its last step,
# OR-ed over all its passes and retries
PATHS = {name: 1 << i for i, name in enumerate((
    "HBL_SEAFLOOR", "HBL_SECOND_MIN", "HBL_NO_HIT", "HBL_MONOB", "HBL_EKMAN", "HBL_RI", "TRAP_U", "TRAP_TJUMP",
    "TRAP_RMS_U", "TRAP_RMS_V", "TRAP_RMS_T", "TRAP_RMS_S", "ITER_DEEPER_AT_ITERMAX", "DD_FINGER", "DD_DIFFCONV"))}
# ORC_PATH_TRAP_V_ALONE: the trap fired at a level on |V| >= 10 where |U| < 10.  Not in PATHS, which is the list the
# seeded regime sweep has to take every member of.
PATH_TRAP_V_ALONE = 1 << 15


def build(force=False):
    """Compile liboracle.so (and _ref when the reference is mounted)."""
    if force or not os.path.exists(LIB) or (
        os.path.getmtime(LIB) < os.path.getmtime(os.path.join(HERE, "mckpp_oracle.c"))
    ):
        subprocess.check_call(["make", "-C", HERE, "liboracle.so"], stdout=subprocess.DEVNULL)
    own = [os.path.join(HERE, f) for f in ("ref_step_shim.F90", "netcdf_standin.F90", "Makefile")]
    libs = [REFLIB] + list(REFSTEPLIB.values())
    if os.path.isdir("/root/reference/src") and not (
            all(map(os.path.exists, libs))
            and min(map(os.path.getmtime, REFSTEPLIB.values())) >= max(map(os.path.getmtime, own))):
        subprocess.check_call(["make", "-C", HERE, "ref"], stdout=subprocess.DEVNULL)


class OrcConst(C.Structure):
    _fields_ = [
        ("nz", C.c_int), ("itermax", C.c_int), ("hmixtolfrac", C.c_double),
        ("dto", C.c_double), ("grav", C.c_double), ("vonk", C.c_double), ("sice", C.c_double),
        ("LKPP", C.c_int), ("LRI", C.c_int), ("LDD", C.c_int), ("L_SSref", C.c_int),
        ("L_RELAX_SST", C.c_int), ("L_RELAX_CALCONLY", C.c_int), ("L_FCORR", C.c_int),
        ("L_FCORR_WITHZ", C.c_int), ("L_SFCORR", C.c_int), ("L_SFCORR_WITHZ", C.c_int),
        ("L_RELAX_SAL", C.c_int), ("L_RELAX_OCNT", C.c_int),
        ("L_NO_FREEZE", C.c_int), ("L_NO_ISOTHERM", C.c_int), ("L_DAMP_CURR", C.c_int),
        ("clim_present", C.c_int), ("iso_bot", C.c_int), ("iso_thresh", C.c_double),
        ("dt_uvdamp", C.c_int), ("exp_mode", C.c_int), ("solver_mode", C.c_int),
        ("zm", C.POINTER(C.c_double)), ("hm", C.POINTER(C.c_double)), ("dm", C.POINTER(C.c_double)),
        ("tri0", C.POINTER(C.c_double)), ("tri1", C.POINTER(C.c_double)),
        ("wmt", C.POINTER(C.c_double)), ("wst", C.POINTER(C.c_double)),
    ]


_lib = None
_ref = None


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.orc_exp_portable.restype = C.c_double
        L.orc_exp_portable.argtypes = [C.c_double]
        L.orc_cpsw.restype = C.c_double
        L.orc_cpsw.argtypes = [C.c_double] * 3
        L.orc_abk80.argtypes = [C.c_double] * 3 + [C.POINTER(C.c_double)] * 5
        L.orc_abk80_batch.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 7
        L.orc_cpsw_batch.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 4
        L.orc_z121.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.orc_lookup.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.orc_lookup_mode.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        L.orc_conv_probe.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 6
        L.orc_conv_literals.argtypes = [C.POINTER(C.c_double)]
        L.orc_conv_unary.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 5
        L.orc_conv_swfrac.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int] + [C.POINTER(C.c_double)] * 2
        L.orc_conv_jerlov.argtypes = [C.c_int, C.POINTER(C.c_double)]
        L.orc_conv_binary.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 14
        L.orc_conv_casts.argtypes = [C.c_int, C.POINTER(C.c_double)] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_double)]
        L.orc_wscale.argtypes = [C.POINTER(OrcConst)] + [C.c_double] * 4 + [C.POINTER(C.c_double)] * 2
        L.orc_swfrac.restype = C.c_double
        L.orc_swfrac.argtypes = [C.POINTER(OrcConst), C.c_double, C.c_double, C.c_int]
        L.orc_swdk.restype = C.c_double
        L.orc_swdk.argtypes = [C.POINTER(OrcConst), C.c_double, C.c_int]
        L.orc_tridcof.argtypes = [C.POINTER(OrcConst), C.POINTER(C.c_double), C.c_int] + [C.POINTER(C.c_double)] * 3
        L.orc_tridmat.restype = C.c_int
        L.orc_tridmat.argtypes = [C.POINTER(C.c_double)] * 5 + [C.c_int] + [C.POINTER(C.c_double)] * 2
        L.orc_tridmat_2e.restype = C.c_int
        L.orc_tridmat_2e.argtypes = [C.POINTER(C.c_double)] * 5 + [C.c_int] + [C.POINTER(C.c_double)] * 2
        L.orc_make_grid_uniform.argtypes = [C.c_int, C.c_double] + [C.POINTER(C.c_double)] * 3
        L.orc_make_tri.argtypes = [C.POINTER(OrcConst)]
        L.orc_coriolis.restype = C.c_double
        L.orc_coriolis.argtypes = [C.c_double]
        L.orc_batch_new.restype = C.c_void_p
        L.orc_batch_new.argtypes = [C.c_long, C.c_int]
        L.orc_batch_free.argtypes = [C.c_void_p]
        L.orc_batch_set.restype = C.c_int
        L.orc_batch_set.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        for fn in ("orc_init_ocean", "orc_physics_driver", "orc_vmix_batch", "orc_vmix_only_batch"):
            getattr(L, fn).argtypes = [C.POINTER(OrcConst), C.c_void_p, C.c_int, C.c_int]
        L.orc_bottomtemp.argtypes = [C.POINTER(OrcConst), C.c_void_p, C.POINTER(C.c_double)]
        L.orc_fluxes.argtypes = [C.POINTER(OrcConst), C.c_void_p, C.c_int] + [C.POINTER(C.c_double)] * 8 + [C.c_int, C.c_double, C.c_double]
        _lib = L
    return _lib


PROBELIB = os.path.join(HERE, "_ref", "libconv_probe.so")
_probe = None


def conv_probe():
    """amdflang build of oracle/conv_probe.F90 (own source; needs the compiler only), or None."""
    global _probe
    if _probe is None:
        if os.path.exists("/opt/rocm/bin/amdflang") and (
                not os.path.exists(PROBELIB) or os.path.getmtime(PROBELIB) < os.path.getmtime(os.path.join(HERE, "conv_probe.F90"))):
            subprocess.check_call(["make", "-C", HERE, "probe"], stdout=subprocess.DEVNULL)
        if not os.path.exists(PROBELIB):
            return None
        P = C.CDLL(PROBELIB)
        P.conv_probe_powers.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 6
        P.conv_probe_literals.argtypes = [C.POINTER(C.c_double)]
        if hasattr(P, "conv_probe_unary"):   # (a library built from the round-4 source has only the two above)
            P.conv_probe_unary.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 5
            P.conv_probe_swfrac.argtypes = [C.c_int, C.POINTER(C.c_double)] + [C.c_double] * 4 + [C.POINTER(C.c_double)] * 2
            P.conv_probe_binary.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 14
            P.conv_probe_casts.argtypes = [C.c_int, C.POINTER(C.c_double)] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_double)]
        _probe = P
    return _probe


def have_ref():
    build()
    return os.path.exists(REFLIB)


def ref():
    """Compiled reference EOS + z121 (only available where /root/reference was)."""
    global _ref
    if _ref is None:
        R = C.CDLL(REFLIB)
        R.ref_cpsw.restype = C.c_double
        R.ref_cpsw.argtypes = [C.c_double] * 3
        R.ref_abk80.argtypes = [C.c_double] * 3 + [C.POINTER(C.c_double)] * 5
        R.ref_abk80_batch.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 7
        R.ref_cpsw_batch.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 4
        R.ref_z121.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _ref = R
    return _ref


def have_ref_step():
    """True where oracle/_ref holds both builds of the reference's physics step."""
    build()
    return all(os.path.exists(p) for p in REFSTEPLIB.values())


_ref_step = {}


def _ref_step_lib(exp_mode, fresh=False):
    """The reference library for exp_mode.  fresh: loaded anew, its module variables as at program start (the
    reference's flux reader allocates its table of file times once per run, src/mckpp_read_fluxes_mod.F90:47)."""
    if fresh and exp_mode in _ref_step:
        import _ctypes

        _ctypes.dlclose(_ref_step.pop(exp_mode)._handle)
    if exp_mode not in _ref_step:
        R = C.CDLL(REFSTEPLIB[exp_mode])
        R.ref_loop_config.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double)]
        R.ref_loop_flux_file.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        R.ref_loop_init.argtypes = []
        R.ref_loop_tri.argtypes = [C.POINTER(C.c_double)] * 2
        R.ref_loop_run.argtypes = [C.c_int, C.c_int]
        R.ref_step_setup.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 6
        R.ref_step_xfer.restype = C.c_int
        R.ref_step_xfer.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int]
        R.ref_step_run.argtypes = [C.c_int, C.c_int]
        _ref_step[exp_mode] = R
    return _ref_step[exp_mode]


# switches of kpp_const_fields in the order of ref_step_setup's sw(1:16) (oracle/ref_step_shim.F90)
_REF_SWITCHES = ["LKPP", "LRI", "LDD", "L_SSref", "L_RELAX_SST", "L_RELAX_CALCONLY", "L_FCORR", "L_FCORR_WITHZ",
                 "L_SFCORR", "L_SFCORR_WITHZ", "L_RELAX_SAL", "L_RELAX_OCNT", "L_NO_FREEZE", "L_NO_ISOTHERM",
                 "L_DAMP_CURR"]


def _ref_layout(nz):
    """batch field -> (reference field, component index tuple after the level axis, first Fortran index, count);
    the reference allocates with nztmax = nz + 1 (as the library's KppConstFields)."""
    nzp1, nzt = nz + 1, nz + 1
    m = {}
    for nm, ref, l in (("U", "U", 0), ("V", "U", 1), ("T", "X", 0), ("S", "X", 1), ("U_init", "U_init", 0),
                       ("V_init", "U_init", 1)):
        m[nm] = (ref, (l,), 1, nzp1)
    for t in (0, 1):
        for nm, ref, l in (("Us", "Us", 0), ("Vs", "Us", 1), ("Ts", "Xs", 0), ("Ss", "Xs", 1)):
            m[f"{nm}{t}"] = (ref, (l, t), 1, nzp1)
    for nm in ("Rig", "Shsq", "swfrac", "tinc_fcorr", "sinc_fcorr", "fcorr_withz", "sfcorr_withz", "scorr",
               "ocnTcorr", "sal_clim", "ocnT_clim"):
        m[nm] = (nm, (), 1, nzp1)
    m["dbloc"] = ("dbloc", (), 1, nz)
    m["swdk_opt"] = ("swdk_opt", (), 0, nz + 1)
    m["rho"] = ("rho", (), 0, nzt + 2)
    m["cp"] = ("cp", (), 0, nzt + 2)
    m["buoy"] = ("buoy", (), 1, nzt + 1)
    for nm in ("difm", "difs", "dift"):
        m[nm] = (nm, (), 0, nzt + 1)
    m["ghat"] = ("ghat", (), 1, nzt)
    m["wU1"], m["wU2"] = ("wU", (0,), 0, nzt + 1), ("wU", (1,), 0, nzt + 1)
    m["wX1"], m["wX2"], m["wX3"] = ("wX", (0,), 0, nzt + 1), ("wX", (1,), 0, nzt + 1), ("wX", (2,), 0, nzt + 1)
    m["wXNT1"] = ("wXNT", (0,), 0, nzt + 1)
    return m


_REF_SHAPES = {"U": (2,), "X": (2,), "U_init": (2,), "Us": (2, 2), "Xs": (2, 2), "wU": (3,), "wX": (3,), "wXNT": (2,)}
_REF_SCALARS = ["f", "Ssurf", "Sref", "SSref", "ocdepth", "hmix", "kmix", "uref", "vref", "Tref", "reset_flag",
                "dampu_flag", "dampv_flag", "freeze_flag", "fcorr", "relax_sst", "SST0", "fcorr_twod", "relax_sal",
                "relax_ocnT"]
_REF_INTS = {"old": "old", "newi": "new", "jerlov": "jerlov", "l_initflag": "l_initflag", "l_ocean": "l_ocean"}


class _RefFields:
    """The columns of a Batch in the compiled reference's kpp_3d_fields (after ref_step_setup) and back."""

    def __init__(self, R, const, batch):
        self.R, self.nz, self.ncol, self.batch = R, const.nz, batch.ncol, batch
        nz, ncol = self.nz, self.ncol
        nzp1, nzt = nz + 1, nz + 1
        self.lay = _ref_layout(nz)
        full = {"U": (nzp1,), "X": (nzp1,), "U_init": (nzp1,), "Us": (nzp1,), "Xs": (nzp1,), "Rig": (nzp1,),
                "Shsq": (nzp1,), "dbloc": (nz,), "rho": (nzt + 2,), "cp": (nzt + 2,), "buoy": (nzt + 1,),
                "swfrac": (nzp1,), "swdk_opt": (nz + 1,), "difm": (nzt + 1,), "difs": (nzt + 1,), "dift": (nzt + 1,),
                "wU": (nzt + 1,), "wX": (nzt + 1,), "wXNT": (nzt + 1,), "ghat": (nzt,)}
        for nm in ("tinc_fcorr", "sinc_fcorr", "fcorr_withz", "sfcorr_withz", "scorr", "ocnTcorr", "sal_clim",
                   "ocnT_clim"):
            full[nm] = (nzp1,)
        self.arrays = {r: np.zeros((ncol,) + lv + _REF_SHAPES.get(r, ())) for r, lv in full.items()}

    def xfer(self, name, arr, put):
        a = np.asfortranarray(arr, dtype=np.float64)
        flat = a.reshape(-1, order="F")
        rc = self.R.ref_step_xfer(name.encode(), len(name), _dp(flat), flat.size, 1 if put else 0)
        if rc != 0:
            raise RuntimeError(f"ref_step_xfer({name}): {rc}")
        return flat.reshape(a.shape, order="F")

    def put(self, run_physics=None, bottom_temp=None):
        batch, ncol = self.batch, self.ncol
        for b, (r, comp, lo, n) in self.lay.items():
            self.arrays[r][(slice(None), slice(None)) + comp] = batch.a[b][:, lo:lo + n]
        for r, a in self.arrays.items():
            self.xfer(r, a, True)
        for nm in _REF_SCALARS:
            self.xfer(nm, batch[nm], True)
        for b, r in _REF_INTS.items():
            self.xfer(r, batch[b], True)
        self.xfer("hmixd", batch["hmixd"], True)
        self.xfer("nmodeadv", batch["nmodeadv"], True)
        self.xfer("modeadv", batch["modeadv"].transpose(0, 2, 1), True)
        self.xfer("advection", batch["advection"].transpose(0, 2, 1), True)
        self.xfer("run_physics", np.ones(ncol) if run_physics is None else run_physics, True)
        if bottom_temp is not None:
            self.xfer("bottom_temp", bottom_temp, True)

    def put_sflux(self, sf):
        sflux = np.zeros((self.ncol, 9, 5, 2))
        sflux[:, 0:6, 4, 0] = sf
        self.xfer("sflux", sflux, True)

    def get_sflux(self):
        return np.ascontiguousarray(self.xfer("sflux", np.zeros((self.ncol, 9, 5, 2)), False)[:, 0:6, 4, 0])

    def get(self, sflux):
        """A Batch of what kpp_3d_fields holds now (fields the reference has no counterpart for - talpha, sbeta,
        status, npasses - stay zero), with `sflux` as its forcing rows."""
        ob = self.batch.copy()
        ob["sflux"] = sflux
        for nm in ("talpha", "sbeta", "status", "npasses", "paths"):
            ob[nm] = 0
        got = {r: self.xfer(r, a, False) for r, a in self.arrays.items()}
        for b, (r, comp, lo, n) in self.lay.items():
            ob.a[b][:, lo:lo + n] = got[r][(slice(None), slice(None)) + comp]
        for nm in _REF_SCALARS:
            ob[nm] = self.xfer(nm, np.zeros(self.ncol), False)
        for b, r in _REF_INTS.items():
            ob[b] = self.xfer(r, np.zeros(self.ncol), False)
        ob["hmixd"] = self.xfer("hmixd", np.zeros((self.ncol, 2)), False)
        return ob


def _ref_setup(R, const, ncol, vary_bottom_temp=False, tri=True):
    """ref_step_setup with the grid, constants and switches of `const`; tri=False hands the reference zeros for
    tri(:,0:1,1), so that whatever the step then uses is what the reference's own init computed."""
    c, nz = const.c, const.nz
    nzp1 = nz + 1
    sw = (C.c_int * 16)(*([int(getattr(c, k)) for k in _REF_SWITCHES] + [int(bool(vary_bottom_temp))]))
    iv = (C.c_int * 4)(c.itermax, c.iso_bot, c.dt_uvdamp, c.clim_present)
    rv = np.array([c.hmixtolfrac, c.dto, c.grav, c.vonk, c.sice, c.iso_thresh])
    zm, hm = np.ascontiguousarray(const.zm[1:nzp1 + 1]), np.ascontiguousarray(const.hm[1:nzp1 + 1])
    dm, t0, t1 = (np.ascontiguousarray(a[0:nz + 1]) for a in (const.dm, const.tri0, const.tri1))
    if not tri:
        t0, t1 = np.zeros(nz + 1), np.zeros(nz + 1)
    R.ref_step_setup(nz, ncol, sw, iv, _dp(rv), _dp(zm), _dp(hm), _dp(dm), _dp(t0), _dp(t1))


def ref_step(const, batch, forcing, exp_mode=1, ntime0=1, run_physics=None, bottom_temp=None, vary_bottom_temp=False):
    """Run the compiled reference's own mckpp_physics_driver() on the columns of `batch` (left unchanged), one step
    per entry of `forcing` (a list of sflux(1:6) arrays [ncol, 6], set before each step), with the grid, constants
    and switches of `const` and EXP from libm (exp_mode=0) or the portable exp (exp_mode=1).  Returns one Batch per
    step holding what the reference's kpp_3d_fields carries after it (fields the reference has no counterpart for -
    talpha, sbeta, status, npasses - stay zero)."""
    R = _ref_step_lib(exp_mode)
    _ref_setup(R, const, batch.ncol, vary_bottom_temp)
    rf = _RefFields(R, const, batch)
    rf.put(run_physics, bottom_temp)
    out = []
    for i, sf in enumerate(forcing):
        rf.put_sflux(sf)
        R.ref_step_run(int(ntime0 + i), 1)
        out.append(rf.get(sf))
    return out


# the flux fields of a record in the order of the in-memory file (oracle/netcdf_standin.F90); a record as
# mckpp_hip_set_flux_series takes it has `snow` as an eighth row, which the reference's reader never reads
REF_FLUX_FILE_FIELDS = ("taux", "tauy", "swf", "lwf", "lhf", "shf", "precip")
_ref_loop_state = {}


def ref_flux_file_times(nrec, ndtocn, dto, startt=0.0, spd=86400.0):
    """Time coordinate of a flux file whose record r (0-based) belongs to steps r*ndtocn + 1 .. (r+1)*ndtocn.
    The reference's reader wants record `pos` within 0.01*dtsec/spd of time + 0.5*ndtocn*dto/spd (its method 1,
    src/mckpp_time_control.F90:121-133), and takes pos = NINT((time - times[0]) * spd / (dto*ndtocn)) + 1 (:153-161).
    With the times exactly at the middle of their intervals that argument is r - 0.5, a tie for NINT which rounding
    noise decides (and which for r = 0 goes to -1, one entry before the array); the times here lie a quarter of
    that tolerance before the middle, which makes the argument r - 0.5 + 0.0025/ndtocn and NINT of it r.  The reader
    also refuses a time to read beyond the file's last one (:95-109), which the middle of the last interval then is:
    ref_init ends the file with one more record, of NaN, that no step of the run reads."""
    mid = startt + (np.arange(nrec) + 0.5) * ndtocn * dto / spd
    return mid - 0.0025 * dto / spd


def ref_init(const, batch, exp_mode=1, run_physics=None, flux_records=None, ndtocn=1, startt=0.0, l_rest=0,
             flsn=334000.0, el=2.5e6, spd=86400.0):
    """The compiled reference's own start of a run on the columns of `batch` (raw profiles, left unchanged):
    mckpp_initialize_time(), mckpp_initialize_fluxes() and mckpp_initialize_ocean_model(), the reference computing
    tri(:,0:1,1) itself.  `flux_records` [nrec, 8 or 7, ncol] (the rows of mckpp_hip_set_flux_series; record r is for
    steps r*ndtocn+1 ..) become the in-memory flux file the reference's reader is served from; None is a run without a
    flux file (l_fluxdata = .FALSE.).  l_ocean is the batch's, run_physics as given.  Returns (Batch after init,
    tri0, tri1); ref_loop(...) then steps this run, on the same exp_mode."""
    R = _ref_step_lib(exp_mode, fresh=True)
    ncol = batch.ncol
    _ref_setup(R, const, ncol, tri=False)
    rf = _RefFields(R, const, batch)
    rf.put(run_physics)
    lv = (C.c_int * 2)(int(flux_records is not None), int(bool(l_rest)))
    rv = np.array([flsn, el, startt, spd, const.c.dto, 100.0, -10.0])
    R.ref_loop_config(lv, int(ndtocn), _dp(rv))
    if flux_records is not None:
        rec = np.asarray(flux_records, dtype=np.float64)
        assert rec.ndim == 3 and rec.shape[1] in (7, 8) and rec.shape[2] == ncol
        rec = np.concatenate([rec[:, 0:7, :], np.full((1, 7, ncol), np.nan)])     # (see ref_flux_file_times)
        times = ref_flux_file_times(rec.shape[0], ndtocn, const.c.dto, startt, spd)
        # flux(nx, ny = 1, ntimes, 7) in Fortran order: column fastest, then record, then field
        flat = np.ascontiguousarray(rec.transpose(1, 0, 2)).reshape(-1)
        R.ref_loop_flux_file(rec.shape[0], _dp(times), _dp(flat))
    R.ref_loop_init()
    t0, t1 = np.zeros(const.nz + 1), np.zeros(const.nz + 1)
    R.ref_loop_tri(_dp(t0), _dp(t1))
    _ref_loop_state[exp_mode] = rf
    return rf.get(rf.get_sflux()), t0, t1


def ref_loop(nt_first, n, exp_mode=1):
    """Steps nt_first .. nt_first+n-1 of the run ref_init started, by the body of the reference's time loop
    (mckpp_update_time, mckpp_fluxes at the update steps - the record its own mckpp_get_update_time picks -,
    mckpp_physics_driver).  Returns one Batch per step, its sflux rows what the reference holds after the step."""
    R, rf = _ref_step_lib(exp_mode), _ref_loop_state[exp_mode]
    out = []
    for nt in range(nt_first, nt_first + n):
        R.ref_loop_run(int(nt), 1)
        out.append(rf.get(rf.get_sflux()))
    return out


# ---------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------
class Const:
    """Owns the numpy buffers behind an OrcConst (Fortran-indexed arrays)."""

    def __init__(self, nz, dto=3600.0, dmax=200.0, exp_mode=0, zm=None, hm=None, dm=None, half_pow_mode=0, **sw):
        L = lib()
        self.nz, self.nzp1 = nz, nz + 1
        n = nz + 4
        self.zm = np.zeros(n)
        self.hm = np.zeros(n)
        self.dm = np.zeros(n)
        self.tri0 = np.zeros(n)
        self.tri1 = np.zeros(n)
        self.wmt = np.zeros(TABLE_SHAPE)
        self.wst = np.zeros(TABLE_SHAPE)
        if zm is None:
            L.orc_make_grid_uniform(nz, dmax, _dp(self.zm), _dp(self.hm), _dp(self.dm))
        else:  # caller-supplied grid, Fortran-indexed (zm[1..nzp1], hm[1..nzp1], dm[0..nz])
            self.zm[: len(zm)] = zm
            self.hm[: len(hm)] = hm
            self.dm[: len(dm)] = dm
        c = OrcConst()
        c.nz = nz
        c.itermax = 200            # initialize_namelist_mod.F90:31
        c.hmixtolfrac = 0.1        # :32
        c.dto = dto
        c.grav, c.vonk, c.sice = 9.816, 0.4, 4.0   # :96-102
        c.LKPP, c.LRI, c.LDD, c.L_SSref = 1, 1, 0, 1  # :111-119
        c.iso_bot, c.iso_thresh, c.dt_uvdamp = 2, 0.002, 360
        c.exp_mode = exp_mode
        for k, v in sw.items():
            if not hasattr(c, k):
                raise KeyError(k)
            setattr(c, k, v)
        c.zm, c.hm, c.dm = _dp(self.zm), _dp(self.hm), _dp(self.dm)
        c.tri0, c.tri1 = _dp(self.tri0), _dp(self.tri1)
        c.wmt, c.wst = _dp(self.wmt), _dp(self.wst)
        self.c = c
        self.half_pow_mode = half_pow_mode
        L.orc_lookup_mode(c.vonk, c.wmt, c.wst, int(half_pow_mode))
        L.orc_make_tri(C.byref(c))

    @property
    def ptr(self):
        return C.byref(self.c)


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
LEVEL_FIELDS = [
    "U", "V", "T", "S", "Us0", "Us1", "Vs0", "Vs1", "Ts0", "Ts1", "Ss0", "Ss1", "U_init", "V_init",
    "swfrac", "swdk_opt", "rho", "cp", "buoy", "talpha", "sbeta", "difm", "difs", "dift", "ghat",
    "wU1", "wU2", "wX1", "wX2", "wX3", "wXNT1", "Rig", "dbloc", "Shsq",
    "tinc_fcorr", "sinc_fcorr", "ocnTcorr", "scorr", "fcorr_withz", "sfcorr_withz", "ocnT_clim", "sal_clim",
]
SCALAR_FIELDS = [
    "f", "Ssurf", "Sref", "SSref", "ocdepth", "hmix", "kmix", "uref", "vref", "Tref",
    "reset_flag", "dampu_flag", "dampv_flag", "freeze_flag", "fcorr",
    "relax_sst", "SST0", "fcorr_twod", "relax_sal", "relax_ocnT",
]
INT_FIELDS = ["old", "newi", "jerlov", "l_initflag", "l_ocean", "status", "npasses", "paths"]


class Batch:
    """Level-fastest batch of columns: arrays [ncol, ld], Fortran index = column index."""

    def __init__(self, ncol, nz, fields=None):
        self.ncol, self.nz, self.nzp1 = ncol, nz, nz + 1
        self.ld = nz + 4
        self.a = {}
        want = set(fields) if fields is not None else None
        for n in LEVEL_FIELDS:
            if want is None or n in want:
                self.a[n] = np.zeros((ncol, self.ld))
        for n in SCALAR_FIELDS:
            if want is None or n in want:
                self.a[n] = np.zeros(ncol)
        for n in INT_FIELDS:
            if want is None or n in want:
                self.a[n] = np.zeros(ncol, dtype=np.int32)
        self.a["nmodeadv"] = np.zeros((ncol, 2), dtype=np.int32)
        self.a["modeadv"] = np.zeros((ncol, 2, 6), dtype=np.int32)
        self.a["advection"] = np.zeros((ncol, 2, 6))
        self.a["sflux"] = np.zeros((ncol, 6))
        self.a["hmixd"] = np.zeros((ncol, 2))
        self.a["ocdepth"] = np.full(ncol, -10000.0)
        self.a["jerlov"] = np.full(ncol, 3, dtype=np.int32)
        self.a["l_ocean"] = np.ones(ncol, dtype=np.int32)
        self.a["newi"] = np.ones(ncol, dtype=np.int32)
        self._h = None

    def __getitem__(self, k):
        return self.a[k]

    def __setitem__(self, k, v):
        self.a[k][...] = v

    def copy(self):
        b = Batch.__new__(Batch)
        b.ncol, b.nz, b.nzp1, b.ld = self.ncol, self.nz, self.nzp1, self.ld
        b.a = {k: v.copy() for k, v in self.a.items()}
        b._h = None
        return b

    def handle(self):
        L = lib()
        h = L.orc_batch_new(self.ncol, self.ld)
        for k, v in self.a.items():
            assert v.flags["C_CONTIGUOUS"]
            rc = L.orc_batch_set(h, k.encode(), v.ctypes.data_as(C.c_void_p))
            assert rc == 0, k
        return h


def _run(fn, const, batch, ntime, nthreads):
    L = lib()
    h = batch.handle()
    try:
        getattr(L, fn)(const.ptr, h, int(ntime), int(nthreads))
    finally:
        L.orc_batch_free(h)


def init_ocean(const, batch, ntime=0, nthreads=0):
    _run("orc_init_ocean", const, batch, ntime, nthreads)


def physics_driver(const, batch, ntime, nthreads=0):
    _run("orc_physics_driver", const, batch, ntime, nthreads)


def vmix_batch(const, batch, ntime, nthreads=0):
    _run("orc_vmix_batch", const, batch, ntime, nthreads)


def vmix_only(const, batch, ntime, nthreads=0):
    _run("orc_vmix_only_batch", const, batch, ntime, nthreads)


def bottomtemp(const, batch, bottom_temp):
    L = lib()
    h = batch.handle()
    bt = np.ascontiguousarray(bottom_temp, dtype=np.float64)
    try:
        L.orc_bottomtemp(const.ptr, h, _dp(bt))
    finally:
        L.orc_batch_free(h)


def fluxes(const, batch, ntime, taux, tauy, swf, lwf, lhf, shf, rain, snow, l_rest=0, flsn=334000.0, el=2.5e6):
    L = lib()
    h = batch.handle()
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (taux, tauy, swf, lwf, lhf, shf, rain, snow)]
    try:
        L.orc_fluxes(const.ptr, h, int(ntime), *[_dp(a) for a in arrs], int(l_rest), float(flsn), float(el))
    finally:
        L.orc_batch_free(h)
