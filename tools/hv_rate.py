"""What fields out and state in on a caller's grid AND a caller's axis cost (include/mckpp_hip_hv.h), beside the calls
that go one of the two ways only, which are the yardsticks.

After a spin-up under constant forcing, in one process, on 100,000 columns of 60 levels (61 values), all resident, a
caller grid of as many points with the bilinear-like table of tools/hgrid_rate.py - 4 entries per row, neighbouring
points, weights that sum to 1 - in both directions, and a caller axis of 75 levels around the column (no clamp: every
model level brackets), as tools/vaxis_rate.py has it:
  (fetch)  T in float64: mckpp_hip_hv_fetch_dev into a (75, n) array, beside mckpp_hip_vaxis_fetch_dev into (75, npts)
           and mckpp_hip_hgrid_fetch_dev into (61, n);
  (put)    T and S incremented over the whole profile (two planes of zeros, so that the state stays what it is):
           mckpp_hip_hv_put_dev from (75, n) arrays, beside mckpp_hip_vaxis_put_dev from (75, npts) arrays and
           mckpp_hip_remap_put_dev from (61, n) arrays.
Each is timed on an idle device by HIP events on the caller's stream around the call (the puts with dev_fence) -
`repeats` calls behind one that is not timed - and as 200 calls queued back to back between two events.  The forms
alternate, `rounds` times, so that a drift of the device shows in all.  One JSON line.
Usage: python tools/hv_rate.py [--ncol 100000] [--nz 60] [--levels 75] [--settle 12] [--repeats 7] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = 200


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
    from hgrid_rate import bilinear_like

    A = mk.api
    ntotal = 100000
    idx = np.arange(0, ntotal, max(1, ntotal // a.ncol))[:a.ncol]
    kc, k3 = cm.make_hip_case(len(idx), a.nz, dto=1200.0, index=idx, ntotal=ntotal)
    npts, nzp1, nax = len(idx), kc.nzp1, a.levels
    n = npts
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, a.settle)
    ctx.hgrid_define(0, n, bilinear_like(npts, n), bilinear_like(n, npts))
    info = ctx.hgrid_info(0)
    zm = kc.zm
    ctx.vaxis_define(0, np.linspace(zm[0] + 1.0, zm[-1] - 1.0, nax))   # around the column: no clamp
    ctx.synchronize()
    flagged_before = int(ctx.status()[1])

    def dev(shape):
        return torch.zeros(shape, dtype=torch.float64, device="cuda")

    out_hv, out_v, out_h = dev((nax, n)), dev((nax, npts)), dev((nzp1, n))
    inc_hv, inc_v, inc_h = ([dev(s) for _ in range(2)] for s in ((nax, n), (nax, npts), (nzp1, n)))
    TS = ("T", "S")
    calls = {
        "hv_fetch_dev": lambda fence: ctx.hv_fetch_dev([("T", 0, 0, out_hv)]),
        "vaxis_fetch_dev": lambda fence: ctx.vaxis_fetch_dev([("T", 0, out_v)]),
        "hgrid_fetch_dev": lambda fence: ctx.hgrid_fetch_dev([("T", 0, out_h)]),
        "hv_put_dev": lambda fence: ctx.hv_put_dev([(f, 0, 0, t) for f, t in zip(TS, inc_hv)], op="add", fence=fence),
        "vaxis_put_dev": lambda fence: ctx.vaxis_put_dev([(f, 0, t) for f, t in zip(TS, inc_v)], op="add", fence=fence),
        "remap_put_dev": lambda fence: ctx.remap_put_dev([(f, 0, t) for f, t in zip(TS, inc_h)], op="add", fence=fence),
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
    key = "ms_per_call_of_%d_back_to_back" % BATCH
    res = {name: {"event_ms": [], key: []} for name in calls}
    for _ in range(a.rounds):
        for name, call in calls.items():
            ms, batch = timed(call)
            res[name]["event_ms"] += ms
            res[name][key].append(batch)
    for name, r in res.items():
        r["median_ms"] = float(np.median(r["event_ms"]))
        r["min_ms"], r["max_ms"] = float(min(r["event_ms"])), float(max(r["event_ms"]))
    # Bytes a call moves by the algorithm.  A fetch on an axis: the rows read, the plane written; on a grid: the same into
    # the staging plane, then the staging read once, the out table (12 B an entry: index and weight) and the caller's
    # plane written.  A put, a plane: the caller's array read once, the in table once where there is one, the rows read
    # and written.
    rows = ncolumns * nzp1 * 8
    res["vaxis_fetch_dev"]["algorithmic_bytes"] = rows + npts * nax * 8
    res["hgrid_fetch_dev"]["algorithmic_bytes"] = rows + 2 * npts * nzp1 * 8 + 12 * info["nnz_out"] + n * nzp1 * 8
    res["hv_fetch_dev"]["algorithmic_bytes"] = rows + 2 * npts * nax * 8 + 12 * info["nnz_out"] + n * nax * 8
    res["vaxis_put_dev"]["algorithmic_bytes"] = 2 * (npts * nax * 8 + 2 * rows)
    res["remap_put_dev"]["algorithmic_bytes"] = 2 * (n * nzp1 * 8 + 12 * info["nnz_in"] + 2 * rows)
    res["hv_put_dev"]["algorithmic_bytes"] = 2 * (n * nax * 8 + 12 * info["nnz_in"] + 2 * rows)
    out = {"shape": f"{npts} x {a.nz}", "resident_columns": ncolumns, "levels": nzp1, "grid_points": n, "axis_levels": nax,
           "hgrid_info": info, "build": A.build_id(), "repeats": a.repeats, "rounds": a.rounds, **res}
    for new, old in (("hv_fetch_dev", "vaxis_fetch_dev"), ("hv_fetch_dev", "hgrid_fetch_dev"), ("hv_put_dev", "vaxis_put_dev"),
                     ("hv_put_dev", "remap_put_dev")):
        out[f"{new}_over_{old}"] = {
            "median": res[new]["median_ms"] / res[old]["median_ms"],
            "back_to_back": float(np.median(res[new][key]) / np.median(res[old][key])),
            "algorithmic_bytes": res[new]["algorithmic_bytes"] / res[old]["algorithmic_bytes"]}
    ctx.step(a.settle + 1, 3)   # the state is still one the model steps from
    out["flagged_before"], out["flagged_after_a_step"] = flagged_before, int(ctx.status()[1])
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
