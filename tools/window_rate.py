"""Output windows inside the launch against the per-step form (include/mckpp_hip.h, mckpp_hip_window_schedule).

The same model steps three ways, each from the same settled state in a fresh context, on configs[3]'s long-run shape
(1e5 x 100, model steps 61 onward) and on the 60-level headline shape:
  (a) mckpp_hip_run_forced of all steps, no output;
  (b) today's form with output: run_forced(nt, 1) + window_accumulate (T, S, hmix) after every step;
  (c) ONE run_forced of all steps with two iodef-like schedules: T, S, hmix "last" every 3 steps, and T, S, hmix
      mean / min / max every 9 steps.
Only the steps (and, in (b), the accumulates) are timed; fetching records is not.  One JSON line per shape.
Usage: python tools/window_rate.py [--steps 72] [--settle 60] [--ncol 100000]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)

import common as cm  # noqa: E402
import mckpp_f90_amd as mk  # noqa: E402

FIELDS = ("T", "S", "hmix")


def run(form, ncol, nz, ntotal, settle, steps):
    A = mk.api
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    kc, k3 = cm.make_hip_case(len(idx), nz, index=idx, ntotal=ntotal)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(len(idx), "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(len(idx), settle + 1, steps, kc.dto, "bench", idx))
    nt0 = settle + 1
    if form == "b":
        ctx.window_select([A.OUT[n] for n in FIELDS])
    if form == "c":
        ctx.window_schedule(0, nt0, 3, steps // 3, FIELDS, A.WIN_LAST)
        ctx.window_schedule(1, nt0, 9, steps // 9, FIELDS, A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX)
    ctx.synchronize()
    t0 = time.perf_counter()
    if form == "b":
        for nt in range(nt0, nt0 + steps):
            if (nt - nt0) % 9 == 0:
                ctx.window_reset()
            ctx.run_forced(nt, 1, 1)
            ctx.window_accumulate()
    else:
        ctx.run_forced(nt0, steps, 1)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    if form == "c":
        assert ctx.window_records(0) == (0, steps // 3 - 1) and ctx.window_records(1) == (0, steps // 9 - 1)
    ctx.close()
    del ctx, k3, kc
    gc.collect()
    return dt / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    a = ap.parse_args()
    for nz in (100, 60):
        ms = {f: run(f, a.ncol, nz, 100000, a.settle, a.steps) for f in ("a", "b", "c")}
        print(json.dumps({"shape": f"{a.ncol} x {nz}, model steps {a.settle + 1}-{a.settle + a.steps}",
                          "ms_per_step": {"a_no_output": ms["a"], "b_step_by_step_with_accumulate": ms["b"],
                                          "c_one_launch_two_schedules": ms["c"]},
                          "c_over_a": ms["c"] / ms["a"], "b_over_a": ms["b"] / ms["a"], "build": mk.api.build_id()}),
              flush=True)


if __name__ == "__main__":
    main()
