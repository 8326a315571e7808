"""Output schedules over chosen points and levels against whole-field schedules (include/mckpp_hip_zoom.h).

The same model steps five ways, each from the same settled state in a fresh context, on the shapes of
tools/window_rate.py (1e5 x 100 and 1e5 x 60, model steps 61 onward):
  (a)  mckpp_hip_run_forced of all steps, no output;
  (c)  ONE run_forced with the two iodef-like schedules of profiles/windows/README.md: T, S, hmix "last" every 3 steps,
       and T, S, hmix mean / min / max every 9 steps;
  (z1) the same two schedules zoomed to levels [0, 1);
  (z2) the same two schedules zoomed to a box of 1 % of the points (mckpp_host_zoom_box on a 400 x 250 grid), all levels;
  (s)  a station series: period 1, "last", T, S, u, v at 50 points.
Only the steps are timed; fetching records is not.  --reps repetitions, the forms alternating within each.  One JSON
line per shape: per form every repetition's ms per step, their median, and the ring bytes of its schedules.
Usage: python tools/zoom_rate.py [--steps 72] [--settle 60] [--ncol 100000] [--reps 3]"""
import argparse
import gc
import json
import os
import statistics
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
FORMS = ("a", "c", "z1", "z2", "s")
NX = 400   # the box of (z2): the points as an NX x (npts / NX) grid


def run(form, ncol, nz, ntotal, settle, steps):
    """(ms per step, ring bytes of the form's schedules)"""
    A = mk.api
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    npts = len(idx)
    kc, k3 = cm.make_hip_case(npts, nz, index=idx, ntotal=ntotal)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(npts, settle + 1, steps, kc.dto, "bench", idx))
    nt0 = settle + 1
    red = A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX
    scheds = []
    if form == "c":
        ctx.window_schedule(0, nt0, 3, steps // 3, FIELDS, A.WIN_LAST)
        ctx.window_schedule(1, nt0, 9, steps // 9, FIELDS, red)
        scheds = [0, 1]
    if form in ("z1", "z2"):
        ny = npts // NX
        zoom = dict(levels=(0, 1)) if form == "z1" else dict(points=A.zoom_box(NX, ny, NX // 4, NX // 10, ny // 4, ny // 10))
        ctx.window_schedule_zoom(0, nt0, 3, steps // 3, FIELDS, A.WIN_LAST, **zoom)
        ctx.window_schedule_zoom(1, nt0, 9, steps // 9, FIELDS, red, **zoom)
        scheds = [0, 1]
    if form == "s":
        ctx.window_schedule_zoom(0, nt0, 1, steps, ("T", "S", "u", "v"), A.WIN_LAST,
                                 points=np.linspace(0, npts - 1, 50).astype(np.int32))
        scheds = [0]
    ring_bytes = sum(ctx.window_zoom(s)[3] for s in scheds)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.run_forced(nt0, steps, 1)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    for s in scheds:
        fk, lc = ctx.window_records(s)
        assert fk == 0 and lc >= steps // 9 - 1
    ctx.close()
    del ctx, k3, kc
    gc.collect()
    return dt / steps * 1e3, ring_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nz", type=int, nargs="*", default=[100, 60])
    a = ap.parse_args()
    for nz in a.nz:
        ms = {f: [] for f in FORMS}
        ring = {}
        for _ in range(a.reps):
            for f in FORMS:   # (alternating: a drift of the box falls on every form alike)
                t, ring[f] = run(f, a.ncol, nz, 100000, a.settle, a.steps)
                ms[f].append(t)
        med = {f: statistics.median(v) for f, v in ms.items()}
        print(json.dumps({"shape": f"{a.ncol} x {nz}, model steps {a.settle + 1}-{a.settle + a.steps}",
                          "ms_per_step": ms, "median_ms_per_step": med, "ring_bytes": ring,
                          "over_a": {f: med[f] / med["a"] for f in FORMS}, "build": mk.api.build_id()}), flush=True)


if __name__ == "__main__":
    main()
