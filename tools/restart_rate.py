"""Restart snapshots inside the launch against cutting the run at every restart (include/mckpp_hip.h,
mckpp_hip_restart_schedule).

The same N model steps with a restart every P steps, each form from the same settled state in a fresh context, real
files written to one directory (and removed after each run), on 1e5 x 60 and 1e5 x 100:
  (a) ONE mckpp_hip_run_forced of all steps, no restarts;
  (b) the form without a schedule: run_forced(P) + save_restart, N / P times;
  (c) restart_schedule with two slots: launches of P steps queued one ahead, restart_snapshot_save of the previous
      snapshot while the next launch runs, then restart_snapshot_release;
  (c_kernel) ONE run_forced of all steps under the schedule (N / P slots, nothing saved): the kernel's own cost of the
      snapshot copies, for the comparison with (a).
Per form: wall time end to end, ms per step from the kernel events ((c): of c_kernel - the events of a call are reused
by the next one, so a pipelined run cannot read them without waiting), the time inside the save calls.  One JSON line
per shape and repeat.
Usage: python tools/restart_rate.py [--steps 288] [--period 72] [--settle 60] [--ncol 100000] [--repeats 3]
                                    [--levels 60 100] [--dir DIR]"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)

import common as cm  # noqa: E402
import mckpp_f90_amd as mk  # noqa: E402


def run(form, ncol, nz, ntotal, settle, steps, period, outdir):
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    kc, k3 = cm.make_hip_case(len(idx), nz, index=idx, ntotal=ntotal)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(len(idx), "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(len(idx), settle + 1, steps, kc.dto, "bench", idx))
    nt0, nrst = settle + 1, steps // period
    files = [os.path.join(outdir, f"restart_{form}_{k}") for k in range(nrst)]
    if form == "c":
        ctx.restart_schedule(nt0, period, 2)
    if form == "c_kernel":
        ctx.restart_schedule(nt0, period, nrst)
    ctx.synchronize()
    kernel_ms, save_s = 0.0, 0.0
    t0 = time.perf_counter()
    if form in ("a", "c_kernel"):
        ctx.run_forced(nt0, steps, 1)
        kernel_ms = ctx.last_kernel_ms()[0]
    elif form == "b":
        for k in range(nrst):
            ctx.run_forced(nt0 + k * period, period, 1)
            kernel_ms += ctx.last_kernel_ms()[0]
            t1 = time.perf_counter()
            ctx.save_restart(files[k])
            save_s += time.perf_counter() - t1
    else:
        ctx.run_forced(nt0, period, 1)
        for k in range(1, nrst + 1):
            if k < nrst:
                ctx.run_forced(nt0 + k * period, period, 1)   # queued behind the launch whose snapshot is saved now
            t1 = time.perf_counter()
            ctx.restart_snapshot_save(k - 1, files[k - 1])
            save_s += time.perf_counter() - t1
            ctx.restart_snapshot_release(k - 1)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    nbytes = 0
    for f in files:
        if os.path.exists(f):
            nbytes += os.path.getsize(f)
            os.remove(f)
    ctx.close()
    del ctx, k3, kc
    gc.collect()
    return {"wall_s": wall, "kernel_ms_per_step": kernel_ms / steps if kernel_ms else None, "save_s": save_s,
            "file_bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=288)
    ap.add_argument("--period", type=int, default=72)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[60, 100])
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    assert a.steps % a.period == 0
    outdir = tempfile.mkdtemp(prefix="restart_rate_", dir=a.dir)
    for nz in a.levels:
        for rep in range(a.repeats):
            r = {f: run(f, a.ncol, nz, 100000, a.settle, a.steps, a.period, outdir) for f in ("a", "b", "c", "c_kernel")}
            ld = 64 * ((nz + 3 + 63) // 64)
            print(json.dumps({"shape": f"{a.ncol} x {nz}", "steps": a.steps, "period": a.period, "repeat": rep,
                              "a_no_restarts": r["a"], "b_cut_and_save_restart": r["b"], "c_schedule_two_slots": r["c"],
                              "c_kernel_one_launch_under_schedule": r["c_kernel"],
                              "c_wall_over_b_wall": r["c"]["wall_s"] / r["b"]["wall_s"],
                              "c_kernel_minus_a_ms_per_step": r["c_kernel"]["kernel_ms_per_step"] - r["a"]["kernel_ms_per_step"],
                              "snapshot_bytes_copied_per_step": 2 * 8 * (14 * ld + 24 + 4) * a.ncol / a.period,
                              "dir": outdir, "build": mk.api.build_id()}), flush=True)
    os.rmdir(outdir)


if __name__ == "__main__":
    main()
