"""What a completed record on a caller's axis costs (include/mckpp_hip_vrecords.h), beside the calls that deliver the
record on the model's levels or the last step's instant on the caller's, which are the yardsticks.

After a spin-up under constant forcing, in one process, on 100,000 columns of 60 levels (61 values), all resident, with
one complete record of the mean of T over three steps, a caller axis of 75 levels around the column (no clamp: every
caller level brackets), as tools/vaxis_rate.py has it, and a caller grid of as many points with the bilinear-like table
of tools/hgrid_rate.py - 4 entries per row:
  (points)  the mean T in float64: mckpp_hip_vrecords_vaxis_dev into a (75, npts) array, beside mckpp_hip_records_dev
            into (61, npts) and mckpp_hip_vaxis_fetch_dev into (75, npts);
  (grid)    mckpp_hip_vrecords_hv_dev into a (75, n) array, beside mckpp_hip_remap_records_dev into (61, n) and
            mckpp_hip_hv_fetch_dev into (75, n);
  (host)    mckpp_hip_vrecords_vaxis_host into a numpy array (75, npts), beside mckpp_hip_window_record_fetch into
            (npts, 61) followed by tests/vaxis_ref.py's vinterp on the host, by the wall clock.
Each device call is timed on an idle device by HIP events on the caller's stream around the call - `repeats` calls behind
one that is not timed - and as 200 calls queued back to back between two events.  The forms alternate, `rounds` times, so
that a drift of the device shows in all.  One JSON line.
Usage: python tools/vrecords_rate.py [--ncol 100000] [--nz 60] [--levels 75] [--settle 12] [--repeats 7] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = 200
PERIOD = 3


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
    import vaxis_ref as vr
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
    zm = np.array(kc.zm[:nzp1], dtype=np.float64)
    z = np.linspace(zm[0] + 1.0, zm[-1] - 1.0, nax)    # around the column: no clamp
    ctx.vaxis_define(0, z)
    ctx.window_schedule(0, a.settle + 1, PERIOD, 1, ("T",), A.WIN_MEAN)
    ctx.step(a.settle + 1, PERIOD)                     # record 0 is complete and stays
    ctx.synchronize()
    flagged_before = int(ctx.status()[1])

    def dev(shape):
        return torch.zeros(shape, dtype=torch.float64, device="cuda")

    out_v, out_r, out_f = dev((nax, npts)), dev((nzp1, npts)), dev((nax, npts))
    out_hv, out_hr, out_hf = dev((nax, n)), dev((nzp1, n)), dev((nax, n))
    calls = {
        "vaxis_records_dev": lambda: ctx.vaxis_records_dev([(0, 0, "T", A.OP_MEAN, 0, out_v)]),
        "records_dev": lambda: ctx.records_dev([(0, 0, "T", A.OP_MEAN, out_r)]),
        "vaxis_fetch_dev": lambda: ctx.vaxis_fetch_dev([("T", 0, out_f)]),
        "hv_records_dev": lambda: ctx.hv_records_dev([(0, 0, "T", A.OP_MEAN, 0, 0, out_hv)]),
        "remap_records_dev": lambda: ctx.remap_records_dev([(0, 0, "T", A.OP_MEAN, 0, out_hr)]),
        "hv_fetch_dev": lambda: ctx.hv_fetch_dev([("T", 0, 0, out_hf)]),
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        call()
        ms = []
        for _ in range(a.repeats):
            ctx.synchronize()
            torch.cuda.synchronize()
            ev[0].record()
            call()
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        ctx.synchronize()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(BATCH):
            call()
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

    # the host form against the route it replaces, by the wall clock
    host_v = np.zeros((nax, npts))
    host_r = np.zeros((npts, nzp1), order="F")
    host = {"vaxis_records_host": [], "vaxis_records_host_keep": [], "window_record_fetch": [], "numpy_vinterp": []}
    for _ in range(1 + a.rounds):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.vaxis_records_host([(0, 0, "T", A.OP_MEAN, 0, host_v)], fill_land=False)   # the array goes up first
        host["vaxis_records_host_keep"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ctx.vaxis_records_host([(0, 0, "T", A.OP_MEAN, 0, host_v)])
        t1 = time.perf_counter()
        ctx.window_record_fetch(0, 0, "T", A.OP_MEAN, host_r)
        t2 = time.perf_counter()
        want = vr.vinterp(zm, np.ascontiguousarray(host_r.T), z)
        t3 = time.perf_counter()
        host["vaxis_records_host"].append(1e3 * (t1 - t0))
        host["window_record_fetch"].append(1e3 * (t2 - t1))
        host["numpy_vinterp"].append(1e3 * (t3 - t2))
    same = bool(np.array_equal(host_v.view(np.uint64), want.view(np.uint64)))
    same = same and bool(np.array_equal(out_v.cpu().numpy().view(np.uint64), want.view(np.uint64)))
    host = {k: {"wall_ms": v, "first_ms": v[0], "median_of_the_rest_ms": float(np.median(v[1:]))} for k, v in host.items()}

    # Bytes a call moves by the algorithm.  A record on the model's levels: the rows' 61 values read, the plane written;
    # on an axis: the same rows read, a plane of 75 levels written; on a grid: that into the staging plane, then the
    # staging read once, the out table (12 B an entry: index and weight) and the caller's plane written.
    rows = ncolumns * nzp1 * 8
    res["records_dev"]["algorithmic_bytes"] = rows + npts * nzp1 * 8
    res["vaxis_records_dev"]["algorithmic_bytes"] = rows + npts * nax * 8
    res["vaxis_fetch_dev"]["algorithmic_bytes"] = rows + npts * nax * 8
    res["remap_records_dev"]["algorithmic_bytes"] = rows + 2 * npts * nzp1 * 8 + 12 * info["nnz_out"] + n * nzp1 * 8
    res["hv_records_dev"]["algorithmic_bytes"] = rows + 2 * npts * nax * 8 + 12 * info["nnz_out"] + n * nax * 8
    res["hv_fetch_dev"]["algorithmic_bytes"] = rows + 2 * npts * nax * 8 + 12 * info["nnz_out"] + n * nax * 8
    out = {"shape": f"{npts} x {a.nz}", "resident_columns": ncolumns, "levels": nzp1, "grid_points": n, "axis_levels": nax,
           "period": PERIOD, "hgrid_info": info, "build": A.build_id(), "repeats": a.repeats, "rounds": a.rounds,
           "host_and_device_bits_equal_the_restatement": same, **res, "host": host}
    for new, old in (("vaxis_records_dev", "records_dev"), ("vaxis_records_dev", "vaxis_fetch_dev"),
                     ("vaxis_fetch_dev", "records_dev"), ("hv_records_dev", "remap_records_dev"), ("hv_records_dev", "hv_fetch_dev")):
        out[f"{new}_over_{old}"] = {
            "median": res[new]["median_ms"] / res[old]["median_ms"],
            "back_to_back": float(np.median(res[new][key]) / np.median(res[old][key])),
            "algorithmic_bytes": res[new]["algorithmic_bytes"] / res[old]["algorithmic_bytes"]}
    ctx.window_record_release(0, 0)
    ctx.step(a.settle + PERIOD + 1, 3)   # the state is still one the model steps from
    out["flagged_before"], out["flagged_after_a_step"] = flagged_before, int(ctx.status()[1])
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
