"""Calls that the library refuses by its own argument checks, on a live context and through a one-shard multi handle:
each returns -1 with the text the entry point had before it went through the guard (mckpp_own.h, `entry`) - the texts
below were recorded by running this file against the library of the commit before - and leaves the context as it was:
three steps afterwards are bit for bit those of a twin that was never refused anything.  None of the calls launches a
kernel; what the guard does with an exception is tests/entry_guard_main.cpp's business."""
import numpy as np
import pytest

import common as cm
from harness import force_bench, initialised, mk  # noqa: F401

pytestmark = pytest.mark.gpu

NPTS, NZ = 13, 12
ALL_FIELDS = cm.PROFILE_FIELDS + cm.SCALAR_FIELDS + ["hmixd0", "hmixd1"] + list(cm.DIAG_FIELDS.keys())
RHO = 16   # api.OUT["rho"]: not among the window fields selected by default

# entry point (without its prefix) -> the text on a context, the text through the one-shard multi handle (where the
# call is the same call on every shard, the shard's text)
REFUSED = {
    "step": ("mckpp_hip_step: nsteps=-1",) * 2,
    "set_solver_mode": ("mckpp_hip_set_solver_mode: unknown solver mode (0: the reference's order, 1: two-ended)",) * 2,
    "step_log_fetch": ("mckpp_hip_step_log_fetch: no step log is set", "mckpp_hip_multi_step_log_fetch: no step log is set"),
    "window_record_fetch": ("mckpp_hip_window_record_fetch: schedule 0 is not set",
                            "mckpp_hip_multi_window_record_fetch: schedule 0 is not set"),
    "restart_snapshot_save": ("mckpp_hip_restart_snapshot_save: no restart schedule is set",) * 2,
    "flux_ring_put": ("mckpp_hip_flux_ring_put: no flux ring is set (mckpp_hip_flux_ring)",) * 2,
    "window_fetch": (f"mckpp_hip_window_fetch: field {RHO} is not among the selected window fields",) * 2,
}


def _refuse_everything(mk, h, multi, tmp_path):
    A = mk.api
    assert A.OUT["rho"] == RHO
    out = np.zeros((NPTS, NZ + 1), order="F")
    dp = out.ctypes.data_as(A._dp)
    rec = np.zeros((8, NPTS))
    args = {
        "step": (1, -1),
        "set_solver_mode": (7,),
        "step_log_fetch": (0, None, None, None, None),
        "window_record_fetch": (0, 0, A.OUT["T"], A.OP_MEAN, dp),
        "restart_snapshot_save": (0, str(tmp_path / "snapshot").encode()),
        "flux_ring_put": (0, rec.ctypes.data_as(A._dp)),
        "window_fetch": (RHO, A.OP_MIN, dp),
    }
    assert set(args) == set(REFUSED)
    for name, a in args.items():
        assert h._raw(name, *a) == -1, name
        text = A._lib().mckpp_hip_last_error().decode()
        print(("multi " if multi else "") + name, "->", text)
        assert text == REFUSED[name][multi], name
        assert text.startswith(("mckpp_hip_" + name, "mckpp_hip_multi_" + name)), name
    assert not (tmp_path / "snapshot").exists() and not out.any()


def _field(k3, name):
    if name in cm.SCALAR_FIELDS:
        return np.asarray(getattr(k3, name))
    if name.startswith("hmixd"):
        return np.asarray(k3.hmixd[:, int(name[-1])])
    return np.asarray(cm.hip_field(k3, name, NZ)[0])


def _three_steps(h, k3):
    force_bench(h, k3)
    h.step(1, 3)
    h.download(k3)
    st, nf, npass = h.status()
    return dict({n: _field(k3, n).copy() for n in ALL_FIELDS}, status=np.array(st), npasses=np.array(npass))


def test_refused_calls_keep_their_texts_and_leave_the_context_alone(mk, tmp_path):
    made = []
    for shards in (0, 1, 0):   # the context, the one-shard multi handle, the untouched twin
        kc, k3 = cm.make_hip_case(NPTS, NZ)
        made.append((initialised(mk, kc, k3, shards), k3))
    (ctx, k3c), (multi, k3m), (twin, k3t) = made
    _refuse_everything(mk, ctx, 0, tmp_path)
    _refuse_everything(mk, multi, 1, tmp_path)
    want = _three_steps(twin, k3t)
    assert np.isfinite(want["T"]).all() and (want["npasses"] > 0).all()
    for what, h, k3 in (("context", ctx, k3c), ("one-shard multi handle", multi, k3m)):
        got = _three_steps(h, k3)
        for n in want:
            assert np.array_equal(got[n], want[n], equal_nan=True), (what, n)
    for h, _ in made:
        h.close()
        assert not h._h
