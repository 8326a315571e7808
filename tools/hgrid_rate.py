"""What the caller's horizontal grids cost (include/mckpp_hip_hgrid.h), beside the calls on the model's points they are
built on.

After a spin-up under constant forcing, in one process, on 100,000 columns of 60 levels (61 values), all resident, and a
caller grid of as many points with a bilinear-like table - 4 entries per row, neighbouring points, weights that sum to
1 - in both directions:
  (fetch)   T on every level in float64: mckpp_hip_hgrid_fetch_dev into a (61, n) array, and mckpp_hip_fetch_dev into a
            (61, npts) array, the yardstick; and the sea surface alone, (1, n) against (1, npts);
  (fluxes)  the eight forcing fields: mckpp_hip_hgrid_fluxes_dev from (8, n), and mckpp_hip_fluxes_dev from (8, npts).
Each is timed on an idle device by HIP events on the caller's stream around the call (the fluxes with dev_fence) -
`repeats` calls behind one that is not timed - and as 200 calls queued back to back between two events.  The forms
alternate, `rounds` times, so that a drift of the device shows in all.  One JSON line.
Usage: python tools/hgrid_rate.py [--ncol 100000] [--nz 60] [--settle 12] [--repeats 7] [--rounds 3]"""
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


def bilinear_like(nrows, nsrc):
    """row r reads the source points around r * nsrc / nrows: 4 entries, spatially local, weights 0.4, 0.3, 0.2, 0.1"""
    base = (np.arange(nrows, dtype=np.int64) * nsrc) // nrows
    idx = np.stack([np.clip(base + d, 0, nsrc - 1) for d in (0, 1, -1, 2)], axis=1).astype(np.int32)
    w = np.tile(np.array([0.4, 0.3, 0.2, 0.1]), (nrows, 1))
    return np.arange(0, 4 * nrows + 1, 4, dtype=np.int64), idx.ravel(), w.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--nz", type=int, default=60)
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
    npts, nzp1 = len(idx), kc.nzp1
    n = npts
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    sflux = cm.synth.forcing(npts, "bench", index=idx)
    cm.set_forcing_3d(k3, sflux)
    ctx.set_forcing(k3.sflux)
    ctx.step(1, a.settle)
    ctx.synchronize()
    ctx.hgrid_define(0, n, bilinear_like(npts, n), bilinear_like(n, npts))
    info = ctx.hgrid_info(0)
    # eight fields that assemble to about the bench forcing: taux, tauy, swf, lwf, 0, 0, rain, 0
    rec = np.zeros((8, npts))
    rec[0], rec[1], rec[2], rec[3], rec[6] = sflux[:, 0], sflux[:, 1], sflux[:, 2], sflux[:, 3], sflux[:, 5]
    f_model = torch.from_numpy(rec).cuda()
    f_grid = torch.from_numpy(np.ascontiguousarray(rec[:, (np.arange(n) * npts) // n])).cuda()
    out_grid = torch.empty((nzp1, n), dtype=torch.float64, device="cuda")
    out_model = torch.empty((nzp1, npts), dtype=torch.float64, device="cuda")
    sst_grid = torch.empty((1, n), dtype=torch.float64, device="cuda")
    sst_model = torch.empty((1, npts), dtype=torch.float64, device="cuda")
    nt = a.settle + 1
    calls = {
        "hgrid_fetch_dev": lambda fence: ctx.hgrid_fetch_dev([("T", 0, out_grid)]),
        "fetch_dev": lambda fence: ctx.fetch_dev([("T", out_model)]),
        "hgrid_fetch_dev_sst": lambda fence: ctx.hgrid_fetch_dev([("T", 0, sst_grid, 0, 1)]),
        "fetch_dev_sst": lambda fence: ctx.fetch_dev([("T", sst_model, 0, 1)]),
        "hgrid_fluxes_dev": lambda fence: ctx.hgrid_fluxes_dev(0, nt, f_grid, fence=fence),
        "fluxes_dev": lambda fence: ctx.fluxes_dev(nt, f_model, fence=fence),
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
    # bytes a call moves by the algorithm.  fetch_dev: the rows read, the plane written.  hgrid_fetch_dev: the same into
    # the staging plane, then stage 2: the staging read once, the table (12 B an entry: index and weight) and the
    # caller's plane written - 12 nnz + 8 n nlev on top of one more pass over the staging.
    nnz = info["nnz_out"]
    for name, nlev in (("", nzp1), ("_sst", 1)):
        first = ncolumns * nlev * 8 + npts * nlev * 8
        res["fetch_dev" + name]["algorithmic_bytes"] = first
        res["hgrid_fetch_dev" + name]["algorithmic_bytes"] = first + npts * nlev * 8 + 12 * nnz + 8 * n * nlev
    # fluxes: eight values per column read, six written (and the 61 values of wXNT1 under the diagnostics, in both forms)
    res["fluxes_dev"]["algorithmic_bytes"] = ncolumns * (8 + 6) * 8
    res["hgrid_fluxes_dev"]["algorithmic_bytes"] = 8 * n * 8 + 12 * info["nnz_in"] + ncolumns * 6 * 8
    out = {"shape": f"{npts} x {a.nz}", "resident_columns": ncolumns, "levels": nzp1, "grid_points": n, "hgrid_info": info,
           "build": A.build_id(), "repeats": a.repeats, "rounds": a.rounds, **res}
    for pair in (("hgrid_fetch_dev", "fetch_dev"), ("hgrid_fetch_dev_sst", "fetch_dev_sst"), ("hgrid_fluxes_dev", "fluxes_dev")):
        out[f"{pair[0]}_over_{pair[1]}"] = {
            "median": res[pair[0]]["median_ms"] / res[pair[1]]["median_ms"],
            "back_to_back": float(np.median(res[pair[0]][key]) / np.median(res[pair[1]][key])),
            "algorithmic_bytes": res[pair[0]]["algorithmic_bytes"] / res[pair[1]]["algorithmic_bytes"]}
    ctx.fluxes_dev(nt, f_model)
    ctx.step(nt, 1)   # the state is still one the model steps from
    out["flagged_after_a_step"] = int(ctx.status()[1])
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
