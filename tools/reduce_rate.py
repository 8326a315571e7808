"""Records reduced on the device against the fetch of the same plane (include/mckpp_hip_reduce.h).

One context at 1e5 x 60 with two schedules of period 3 over T - unzoomed, and zoomed to level 0 - and one completed
record.  Three reductions, each timed as wall time from the call to the value on the host (records_reduce_host), beside
mckpp_hip_window_record_fetch of the same plane alone - the code every monitor used until now; its host-side reduction
is left out of its time, which favours it:
  (a) domain-mean SST: the area-weighted average of the level-0 zoom's one level          -> 1 double
  (b) area-mean heat content: the axis sum of the unzoomed T with hm, then the average    -> 1 double
  (c) the horizontal-mean T profile: the area-weighted average of every level             -> nzp1 doubles
--reps repetitions, the forms alternating within each, after one untimed call of each (first use allocates the
scratch and pins the fetch's array).  One JSON line: per case every repetition's ms for both paths, their medians, and
the bytes each path moves over the bus.
Usage: python tools/reduce_rate.py [--ncol 100000] [--nz 60] [--reps 7]"""
import argparse
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

PERIOD = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--nz", type=int, default=60)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    A = mk.api
    npts, nzp1 = a.ncol, a.nz + 1
    kc, k3 = cm.make_hip_case(npts, a.nz)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench"))
    ctx.set_forcing(k3.sflux)
    ctx.reduce_weights(np.cos(np.linspace(-1.4, 1.4, npts)), kc.hm, None)
    ctx.window_schedule(0, 1, PERIOD, 1, ("T",), A.WIN_MEAN)
    ctx.window_schedule_zoom(1, 1, PERIOD, 1, ("T",), A.WIN_MEAN, levels=(0, 1))
    ctx.step(1, PERIOD)
    ctx.synchronize()
    both = A.RED_W_LEVELS | A.RED_W_POINTS
    cases = {
        "a_sst_mean": ((1, 0, "T", A.OP_MEAN, np.zeros(1), "none", "average", A.RED_W_POINTS), (1, np.zeros((npts, 1), order="F"))),
        "b_heat_content": ((0, 0, "T", A.OP_MEAN, np.zeros(1), "sum", "average", both), (0, np.zeros((npts, nzp1), order="F"))),
        "c_mean_profile": ((0, 0, "T", A.OP_MEAN, np.zeros(nzp1), "none", "average", A.RED_W_POINTS), (0, np.zeros((npts, nzp1), order="F"))),
    }

    def reduce(name):
        ctx.records_reduce_host([cases[name][0]])

    def fetch(name):
        sched, out = cases[name][1]
        ctx.window_record_fetch(sched, 0, "T", A.OP_MEAN, out)

    ms = {n: {"reduce": [], "fetch": []} for n in cases}
    for rep in range(a.reps + 1):   # (the first round is not timed)
        for n in cases:
            for what, fn in (("reduce", reduce), ("fetch", fetch)):
                t0 = time.perf_counter()
                fn(n)
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    ms[n][what].append(dt)
    out = {"shape": f"{npts} x {a.nz}", "ms": ms, "build": A.build_id()}
    out["median_ms"] = {n: {w: statistics.median(v) for w, v in d.items()} for n, d in ms.items()}
    out["bus_bytes"] = {n: {"reduce": cases[n][0][4].nbytes, "fetch": cases[n][1][1].nbytes} for n in cases}
    out["reduce_below_fetch"] = {n: d["reduce"] < d["fetch"] for n, d in out["median_ms"].items()}
    out["values"] = {n: [float(v) for v in cases[n][0][4][:3]] for n in cases}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
