"""What the caller's vertical axes cost (include/mckpp_hip_vaxis.h), beside the calls on model levels they are built on.

After a spin-up under constant forcing, in one process, on 100,000 columns of 60 levels (61 values) and a caller axis of
75 levels around the column:
  (put)    four planes - u, v, T, S - ADDed in float64: mckpp_hip_vaxis_put_dev from (75, npts) arrays, and mckpp_hip_put_dev
           from (61, npts) arrays, the yardstick;
  (fetch)  the same four fields out: mckpp_hip_vaxis_fetch_dev into (75, npts) arrays, and mckpp_hip_fetch_dev into
           (61, npts) arrays.
Each is timed on an idle device by HIP events on the caller's stream around the call (the puts with dev_fence) - `repeats`
calls behind one that is not timed - and as 200 calls queued back to back between two events.  The two forms of a pair
alternate, `rounds` times, so that a drift of the device shows in both.  One JSON line.
Usage: python tools/vaxis_rate.py [--ncol 100000] [--nz 60] [--levels 75] [--settle 12] [--repeats 7] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = 200
FIELDS = ("u", "v", "T", "S")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--nz", type=int, default=60)
    ap.add_argument("--levels", type=int, default=75)
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()

    import torch   # before the library: one HIP runtime in the process

    import common as cm
    import mckpp_f90_amd as mk

    A = mk.api
    ntotal = 100000
    idx = np.arange(0, ntotal, max(1, ntotal // a.ncol))[:a.ncol]
    kc, k3 = cm.make_hip_case(len(idx), a.nz, dto=1200.0, index=idx, ntotal=ntotal)
    npts, nzp1, n = len(idx), kc.nzp1, a.levels
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, a.settle)
    ctx.synchronize()
    zm = kc.zm
    z = np.linspace(zm[0] + 1.0, zm[-1] - 1.0, n)     # around the column: no clamp, every model level brackets
    ctx.vaxis_define(0, z)
    pt = np.arange(npts)[None, :]
    inc_axis = {f: torch.from_numpy(1e-7 * np.sin(pt + z[:, None] / 10.0 + i)).cuda() for i, f in enumerate(FIELDS)}
    inc_model = {f: torch.from_numpy(1e-7 * np.sin(pt + zm[:, None] / 10.0 + i)).cuda() for i, f in enumerate(FIELDS)}
    out_axis = {f: torch.empty((n, npts), dtype=torch.float64, device="cuda") for f in FIELDS}
    out_model = {f: torch.empty((nzp1, npts), dtype=torch.float64, device="cuda") for f in FIELDS}
    calls = {
        "vaxis_put_dev": lambda fence: ctx.vaxis_put_dev([(f, 0, t) for f, t in inc_axis.items()], op="add", fence=fence),
        "put_dev": lambda fence: ctx.put_dev([(f, t) for f, t in inc_model.items()], op="add", fence=fence),
        "vaxis_fetch_dev": lambda fence: ctx.vaxis_fetch_dev([(f, 0, t) for f, t in out_axis.items()]),
        "fetch_dev": lambda fence: ctx.fetch_dev([(f, t) for f, t in out_model.items()]),
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        call(True)
        ms = []
        for _ in range(a.repeats):
            ctx.synchronize()
            torch.cuda.synchronize()
            ev[0].record()
            call(True)
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        ctx.synchronize()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(BATCH):
            call(False)
        ctx.dev_fence()
        ev[1].record()
        ev[1].synchronize()
        return ms, ev[0].elapsed_time(ev[1]) / BATCH

    ncolumns = int(ctx.ncolumns)
    res = {name: {"event_ms": [], "ms_per_call_of_%d_back_to_back" % BATCH: []} for name in calls}
    for _ in range(a.rounds):
        for name, call in calls.items():
            ms, batch = timed(call)
            res[name]["event_ms"] += ms
            res[name]["ms_per_call_of_%d_back_to_back" % BATCH].append(batch)
    for name, r in res.items():
        r["median_ms"] = float(np.median(r["event_ms"]))
        r["min_ms"], r["max_ms"] = float(min(r["event_ms"])), float(max(r["event_ms"]))
    # bytes a call moves by the algorithm, four planes: the caller's array once, the rows read (an add) and written
    rows = 4 * ncolumns * nzp1 * 8
    res["vaxis_put_dev"]["algorithmic_bytes"] = 4 * ncolumns * n * 8 + 2 * rows
    res["put_dev"]["algorithmic_bytes"] = 4 * ncolumns * nzp1 * 8 + 2 * rows
    res["vaxis_fetch_dev"]["algorithmic_bytes"] = rows + 4 * ncolumns * n * 8
    res["fetch_dev"]["algorithmic_bytes"] = rows + 4 * ncolumns * nzp1 * 8
    out = {"shape": f"{npts} x {a.nz}", "resident_columns": ncolumns, "levels": nzp1, "axis_levels": n, "build": A.build_id(),
           "repeats": a.repeats, "rounds": a.rounds, **res}
    for pair in (("vaxis_put_dev", "put_dev"), ("vaxis_fetch_dev", "fetch_dev")):
        out[f"{pair[0]}_over_{pair[1]}"] = {
            "median": res[pair[0]]["median_ms"] / res[pair[1]]["median_ms"],
            "back_to_back": float(np.median(res[pair[0]]["ms_per_call_of_%d_back_to_back" % BATCH]) /
                                  np.median(res[pair[1]]["ms_per_call_of_%d_back_to_back" % BATCH])),
            "algorithmic_bytes": res[pair[0]]["algorithmic_bytes"] / res[pair[1]]["algorithmic_bytes"]}
    ctx.step(a.settle + 1, 1)   # the state is still one the model steps from
    out["flagged_after_a_step"] = int(ctx.status()[1])
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
