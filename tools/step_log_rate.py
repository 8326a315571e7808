"""What the step log costs a forced run (include/mckpp_hip.h, mckpp_hip_step_log).

The same N model steps in ONE mckpp_hip_run_forced from the same settled state, on 1e5 x 60 and 1e5 x 100, each form in
a fresh context:
  (a) without a log;
  (b) with a status-only log (min_passes = 0);
  (c) with min_passes = 13 (every column-step of 13 passes or more is an event).
The log has room for every column-step of the run, so nothing overflows.  Per form: kernel ms per step from the
kernel events, n_events, and the time inside step_log_count + step_log_fetch (the count waits for the stream: it is
called after a synchronise, so that the wait for the launch is not part of it).  One JSON line per shape and repeat.
Every (shape, repeat) runs in a child process of its own under a time limit; after a child that fails or runs out of
time nothing more is started.
Usage: python tools/step_log_rate.py [--steps 288] [--settle 60] [--ncol 100000] [--repeats 3] [--levels 60 100]
                                     [--min-passes 13] [--timeout 240]"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMS = (("a_no_log", None), ("b_status_only", 0), ("c_min_passes", -1))   # (-1: --min-passes)


def run(mk, cm, np, min_passes, ncol, nz, ntotal, settle, steps):
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    kc, k3 = cm.make_hip_case(len(idx), nz, index=idx, ntotal=ntotal)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(len(idx), "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(len(idx), settle + 1, steps, kc.dto, "bench", idx))
    if min_passes is not None:
        ctx.step_log(len(idx) * steps, min_passes)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.run_forced(settle + 1, steps, 1)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    out = {"wall_s": wall, "kernel_ms_per_step": ctx.last_kernel_ms()[0] / steps, "launches": ctx.last_launch_count()}
    if min_passes is not None:
        t1 = time.perf_counter()
        n_events, n_stored, status_or = ctx.step_log_count()
        t2 = time.perf_counter()
        rec = ctx.step_log_fetch()
        t3 = time.perf_counter()
        out.update({"min_passes": min_passes, "n_events": n_events, "n_stored": n_stored, "status_or": status_or,
                    "count_s": t2 - t1, "fetch_s": t3 - t2, "count_plus_fetch_s": t3 - t1,
                    "flagged": int((rec[2] != 0).sum()), "most_passes": int(rec[3].max()) if n_stored else 0})
    ctx.close()
    del ctx, k3, kc
    gc.collect()
    return out


def child(a, nz, rep):
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)

    import common as cm
    import mckpp_f90_amd as mk

    r = {name: run(mk, cm, np, a.min_passes if mp == -1 else mp, a.ncol, nz, 100000, a.settle, a.steps) for name, mp in FORMS}
    ka = r["a_no_log"]["kernel_ms_per_step"]
    print(json.dumps({"shape": f"{a.ncol} x {nz}", "steps": a.steps, "repeat": rep, **r,
                      "b_minus_a_ms_per_step": r["b_status_only"]["kernel_ms_per_step"] - ka,
                      "c_minus_a_ms_per_step": r["c_min_passes"]["kernel_ms_per_step"] - ka,
                      "build": mk.api.build_id()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=288)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[60, 100])
    ap.add_argument("--min-passes", type=int, default=13)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a (shape, repeat) child may take")
    ap.add_argument("--child", type=int, nargs=2, metavar=("LEVELS", "REPEAT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, *a.child)
        return 0
    for nz in a.levels:
        for rep in range(a.repeats):
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--settle", str(a.settle), "--ncol",
                   str(a.ncol), "--min-passes", str(a.min_passes), "--child", str(nz), str(rep)]
            try:
                rc = subprocess.run(cmd, timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps({"shape": f"{a.ncol} x {nz}", "repeat": rep, "error": f"no result in {a.timeout} s"}), flush=True)
                return 1
            if rc != 0:   # (a fault on the device: nothing more is started on it)
                print(json.dumps({"shape": f"{a.ncol} x {nz}", "repeat": rep, "error": f"exit status {rc}"}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
