"""The L_VARY_BOTTOM_TEMP override inside the launch against a launch per step with the host's override
(include/mckpp_hip.h, mckpp_hip_set_bottomtemp).

The same N steps of a forced run with the switch on, each form from the same settled state in a fresh context:
  (a) a launch per step: run_forced(nt, 1) + mckpp_hip_bottomtemp (which compacts on the host, copies, launches
      k_bottomtemp and synchronises the stream), N times - the only correct form before the resident field;
  (b) ONE run_forced of all steps with the resident bottom temperature;
  (c) ONE run_forced of all steps without the switch: what (b)'s override costs inside the launch.
Per form: wall time end to end per step, and for (b) and (c) ms per step from the kernel events ((a): the sum of its
launches' events, without the override's kernel and copies).  One JSON line per shape and repeat, on stdout and - with
--out - appended to that file.
Usage: python tools/bottomtemp_rate.py [--steps 96] [--settle 60] [--repeats 3] [--shapes 100000x60 12500x100]
                                       [--out profiles/bottomtemp/rate.json]"""
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


def run(form, ncol, nz, ntotal, settle, steps):
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    kc, k3 = cm.make_hip_case(len(idx), nz, index=idx, ntotal=ntotal)
    bt = np.asarray(k3.X[:, nz, 0]) - 0.5
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(len(idx), "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(len(idx), settle + 1, steps, kc.dto, "bench", idx))
    nt0 = settle + 1
    if form == "b":
        ctx.set_bottomtemp(bt)
    ctx.synchronize()
    kernel_ms = 0.0
    t0 = time.perf_counter()
    if form == "a":
        for k in range(steps):
            ctx.run_forced(nt0 + k, 1, 1)
            ctx.bottomtemp(bt)
            kernel_ms += ctx.last_kernel_ms()[0]
    else:
        ctx.run_forced(nt0, steps, 1)
        ctx.synchronize()
        kernel_ms = ctx.last_kernel_ms()[0]
    ctx.synchronize()
    wall = time.perf_counter() - t0
    ctx.close()
    del ctx, k3, kc
    gc.collect()
    return {"wall_ms_per_step": 1e3 * wall / steps, "kernel_ms_per_step": kernel_ms / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["100000x60", "12500x100"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for shape in a.shapes:
        ncol, nz = (int(v) for v in shape.split("x"))
        for rep in range(a.repeats):
            r = {f: run(f, ncol, nz, 100000, a.settle, a.steps) for f in ("a", "b", "c")}
            line = json.dumps({"shape": f"{ncol} x {nz}", "steps": a.steps, "repeat": rep,
                               "a_launch_per_step_host_override": r["a"], "b_one_launch_resident_field": r["b"],
                               "c_one_launch_no_switch": r["c"],
                               "a_wall_over_b_wall": r["a"]["wall_ms_per_step"] / r["b"]["wall_ms_per_step"],
                               "b_minus_c_kernel_ms_per_step": r["b"]["kernel_ms_per_step"] - r["c"]["kernel_ms_per_step"],
                               "build": mk.api.build_id()})
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
