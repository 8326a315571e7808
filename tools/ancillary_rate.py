"""Boundary updates inside the one-launch forced run against a launch per step with the update between the launches
(include/mckpp_hip.h, mckpp_hip_set_ancillary_series / mckpp_hip_ancillary_schedule).

The same N forced steps with L_RELAX_OCNT and L_RELAX_SAL on and both climatologies interpolated between two records
every step (L_INTERP_OCNT, L_INTERP_SAL with ndt_interp = 1), each form from the same settled state in a fresh context:
  (a) a launch per step: the two fields formed on the host (numpy, nxt*wn + prv*wp), update_ancillaries, run_forced(nt, 1),
      N times - the only form before the series;
  (b) ONE run_forced of all steps under the two schedules, the records resident;
  (c) ONE run_forced of all steps with no schedule (the climatology of step 1 throughout): what (b)'s selection and second
      load cost inside the launch.
Per form: wall time end to end per step, and ms per step from the kernel events ((a): the sum of its launches' events,
without the transfers between them).  One JSON line per shape and repeat, on stdout and - with --out - appended to that file.
Usage: python tools/ancillary_rate.py [--steps 48] [--settle 12] [--repeats 2] [--shapes 100000x100]
                                      [--out profiles/ancillary/rate.json]"""
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

EVERY = 24   # steps between two records


def run(form, ncol, nz, ntotal, settle, steps):
    A = mk.api
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    kc, k3 = cm.make_hip_case(len(idx), nz, index=idx, ntotal=ntotal)
    kc.L_RELAX_OCNT = kc.L_RELAX_SAL = 1
    n = len(idx)
    k3.relax_ocnT[:] = 1.0 / (30 * 86400.0)
    k3.relax_sal[:] = 1.0 / (15 * 86400.0)
    nrec = (steps - 1) // EVERY + 2
    T0, S0 = np.asarray(k3.X[:, :, 0]).copy(), np.asarray(k3.X[:, :, 1]).copy()
    recs = {"ocnT_clim": np.stack([T0 - 0.3 + 0.1 * r for r in range(nrec)]),     # [nrec, npts, nzp1]
            "sal_clim": np.stack([S0 + 0.05 + 0.01 * r for r in range(nrec)])}
    epochs = [(i // EVERY, i // EVERY + 1, 1.0 - (i % EVERY) / EVERY, (i % EVERY) / EVERY) for i in range(steps)]
    k3.ocnT_clim[...] = recs["ocnT_clim"][0]
    k3.sal_clim[...] = recs["sal_clim"][0]
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(n, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(n, settle + 1, steps, kc.dto, "bench", idx))
    nt0 = settle + 1
    if form == "b":
        for name, kind in (("ocnT_clim", A.ANC_OCNT_CLIM), ("sal_clim", A.ANC_SAL_CLIM)):
            ctx.set_ancillary_series(kind, 0, np.ascontiguousarray(recs[name].transpose(0, 2, 1)))
            ctx.ancillary_schedule(kind, nt0, 1, epochs)
    ctx.synchronize()
    kernel_ms = 0.0
    t0 = time.perf_counter()
    if form == "a":
        for k in range(steps):
            p, q, wp, wn = epochs[k]
            for name in recs:
                getattr(k3, name)[...] = recs[name][q] * wn + recs[name][p] * wp
            ctx.update_ancillaries(k3)
            ctx.run_forced(nt0 + k, 1, 1)
            ctx.synchronize()
            kernel_ms += ctx.last_kernel_ms()[0]
    else:
        ctx.run_forced(nt0, steps, 1)
        ctx.synchronize()
        kernel_ms = ctx.last_kernel_ms()[0]
    wall = time.perf_counter() - t0
    ctx.close()
    del ctx, k3, kc, recs
    gc.collect()
    return {"wall_ms_per_step": 1e3 * wall / steps, "kernel_ms_per_step": kernel_ms / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["100000x100"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for shape in a.shapes:
        ncol, nz = (int(v) for v in shape.split("x"))
        for rep in range(a.repeats):
            r = {f: run(f, ncol, nz, 100000, a.settle, a.steps) for f in ("a", "b", "c")}
            line = json.dumps({"shape": f"{ncol} x {nz}", "steps": a.steps, "repeat": rep,
                               "a_launch_per_step_host_interpolation": r["a"], "b_one_launch_under_schedules": r["b"],
                               "c_one_launch_no_schedule": r["c"],
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
