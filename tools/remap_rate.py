"""What records out and state in on a caller's horizontal grid cost (include/mckpp_hip_remap.h), beside the calls of the
same planes on the model's points, which are the yardstick.

After a spin-up under constant forcing, in one process, on 100,000 columns of 60 levels (61 values), all resident, and a
caller grid of as many points with the bilinear-like table of tools/hgrid_rate.py - 4 entries per row, neighbouring
points, weights that sum to 1 - in both directions; one output schedule keeps the mean of T over `period` steps:
  (records)  the interval mean of T in float64: mckpp_hip_remap_records_dev into a (61, n) array against
             mckpp_hip_records_dev into a (61, npts) array; and the mean SST alone, (1, n) against (1, npts);
  (puts)     T and S incremented over the whole axis (two planes of zeros, so that the state stays what it is):
             mckpp_hip_remap_put_dev from (61, n) arrays against mckpp_hip_put_dev from (61, npts) arrays; and the SST
             set from a (1, n) array - what mckpp_hip_hgrid_fetch_dev delivered - against a (1, npts) array.
Each is timed on an idle device by HIP events on the caller's stream around the call (the puts with dev_fence) -
`repeats` calls behind one that is not timed - and as 200 calls queued back to back between two events.  The forms
alternate, `rounds` times, so that a drift of the device shows in all.  One JSON line.
Usage: python tools/remap_rate.py [--ncol 100000] [--nz 60] [--settle 12] [--period 3] [--repeats 7] [--rounds 3]"""
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
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--period", type=int, default=3)
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
    npts, nzp1 = len(idx), kc.nzp1
    n = npts
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, a.settle)
    ctx.hgrid_define(0, n, bilinear_like(npts, n), bilinear_like(n, npts))
    info = ctx.hgrid_info(0)
    ctx.window_schedule(0, a.settle + 1, a.period, 1, ("T",), A.WIN_MEAN)
    ctx.step(a.settle + 1, a.period)      # record 0 is complete and stays: every delivery below is of it
    ctx.synchronize()
    flagged_before = int(ctx.status()[1])

    def dev(shape):
        return torch.zeros(shape, dtype=torch.float64, device="cuda")

    rec_grid, rec_model, sst_rec_grid, sst_rec_model = dev((nzp1, n)), dev((nzp1, npts)), dev((1, n)), dev((1, npts))
    inc_grid, inc_model = [dev((nzp1, n)) for _ in range(2)], [dev((nzp1, npts)) for _ in range(2)]
    sst_grid, sst_model = dev((1, n)), dev((1, npts))
    ctx.hgrid_fetch_dev([("T", 0, sst_grid, 0, 1)], norm="used")
    ctx.fetch_dev([("T", sst_model, 0, 1)])
    calls = {
        "remap_records_dev": lambda fence: ctx.remap_records_dev([(0, 0, "T", A.OP_MEAN, 0, rec_grid)]),
        "records_dev": lambda fence: ctx.records_dev([(0, 0, "T", A.OP_MEAN, rec_model)]),
        "remap_records_dev_sst": lambda fence: ctx.remap_records_dev([(0, 0, "T", A.OP_MEAN, 0, sst_rec_grid, 0, 1)]),
        "records_dev_sst": lambda fence: ctx.records_dev([(0, 0, "T", A.OP_MEAN, sst_rec_model, 0, 1)]),
        "remap_put_dev": lambda fence: ctx.remap_put_dev([("T", 0, inc_grid[0]), ("S", 0, inc_grid[1])], op="add", fence=fence),
        "put_dev": lambda fence: ctx.put_dev([("T", inc_model[0]), ("S", inc_model[1])], op="add", fence=fence),
        "remap_put_dev_sst": lambda fence: ctx.remap_put_dev([("T", 0, sst_grid)], op="set", fence=fence),
        "put_dev_sst": lambda fence: ctx.put_dev([("T", sst_model)], op="set", fence=fence),
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
    # Bytes a call moves by the algorithm.  records_dev: the record's rows read, the plane written.  remap_records_dev:
    # the same into the staging plane, then the staging read once, the out table (12 B an entry: index and weight) and
    # the caller's plane written.  put_dev, a plane: the array read, the rows read and written (a set: written).
    # remap_put_dev, a plane: the caller's array read once, the in table once, the rows as before.
    for name, nlev in (("", nzp1), ("_sst", 1)):
        first = ncolumns * nlev * 8 + npts * nlev * 8
        res["records_dev" + name]["algorithmic_bytes"] = first
        res["remap_records_dev" + name]["algorithmic_bytes"] = first + npts * nlev * 8 + 12 * info["nnz_out"] + 8 * n * nlev
    res["put_dev"]["algorithmic_bytes"] = 2 * (npts * nzp1 * 8 + ncolumns * nzp1 * 16)
    res["remap_put_dev"]["algorithmic_bytes"] = 2 * (n * nzp1 * 8 + 12 * info["nnz_in"] + ncolumns * nzp1 * 16)
    res["put_dev_sst"]["algorithmic_bytes"] = npts * 8 + ncolumns * 16            # the element and the column's Tref
    res["remap_put_dev_sst"]["algorithmic_bytes"] = n * 8 + 12 * info["nnz_in"] + ncolumns * 16
    out = {"shape": f"{npts} x {a.nz}", "resident_columns": ncolumns, "levels": nzp1, "grid_points": n, "hgrid_info": info,
           "period": a.period, "build": A.build_id(), "repeats": a.repeats, "rounds": a.rounds, **res}
    for new, old in (("remap_records_dev", "records_dev"), ("remap_records_dev_sst", "records_dev_sst"),
                     ("remap_put_dev", "put_dev"), ("remap_put_dev_sst", "put_dev_sst")):
        out[f"{new}_over_{old}"] = {
            "median": res[new]["median_ms"] / res[old]["median_ms"],
            "back_to_back": float(np.median(res[new][key]) / np.median(res[old][key])),
            "algorithmic_bytes": res[new]["algorithmic_bytes"] / res[old]["algorithmic_bytes"]}
    ctx.window_record_release(0, 0)
    ctx.step(a.settle + a.period + 1, a.period)   # the state is still one the model steps from
    out["flagged_before"], out["flagged_after_a_step"] = flagged_before, int(ctx.status()[1])
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
