"""What it costs to write the prognostic state of a resident run: through mckpp_hip_put_dev (include/mckpp_hip_put.h), or
through the route it replaces - a download of the prognostic group, an add on the host and mckpp_hip_upload.

After a spin-up under constant forcing, in one process per shape (both routes in the same session):
  (put)   one call that puts T and S over the whole axis from two device tensors (nzp1, npts): ADD in float64, ADD in
          float32, and SET with both time levels in float64.  Timed on an idle device by HIP events on the caller's
          stream around put_dev + dev_fence - they include the two event waits that order the call -, by the host's
          clock around the call alone (what the caller's thread pays: nothing waits for the device), and as 50 calls
          queued back to back between two events (ms per call of a steady sequence);
  (host)  download(F_RESTART) of the prognostic group, X(:,:,1:2) += dX in numpy, upload: the host's clock around each,
          the first round (which pins the host arrays) reported apart from the later ones.
One JSON line per shape.  Every shape runs under a time limit of its own and the first failure ends the run.
Usage: python tools/put_rate.py [--ncol 100000] [--settle 12] [--repeats 5] [--shapes 60 shipped]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


BATCH = 50


def run(shape, ncol, settle, repeats):
    import torch   # before the library: one HIP runtime in the process

    import common as cm
    import mckpp_f90_amd as mk

    A = mk.api
    ntotal = 100000
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    if shape == "shipped":   # 69 stretched levels, 35 % land, dto 1200 s
        kc, k3 = cm.make_hip_case(len(idx), 69, grid="stretched", dto=1200.0, index=idx, ntotal=ntotal)
        land = (np.arange(len(idx)) * 7) % 20 < 7
        k3.run_physics[land] = 0
        k3.l_ocean[land] = 0
    else:
        kc, k3 = cm.make_hip_case(len(idx), int(shape), dto=1200.0, index=idx, ntotal=ntotal)
    npts, nzp1 = len(idx), kc.nzp1
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.synchronize()
    ncolumns = int(ctx.ncolumns)
    pt, lev = np.arange(npts)[None, :], np.arange(nzp1)[:, None]
    inc = {"T": 1e-6 * np.sin(pt + lev / 10.0), "S": 1e-7 * np.cos(pt + lev / 10.0)}
    out = {"shape": f"{npts} x {shape}", "resident_columns": ncolumns, "levels": nzp1, "build": A.build_id()}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(planes, **kw):
        """(event ms, host ms of the call) of `repeats` puts on an idle device, behind one that is not timed; then ms per
        call of BATCH calls back to back"""
        ctx.put_dev(planes, fence=True, **kw)
        ms, host = [], []
        for _ in range(repeats):
            ctx.synchronize()
            torch.cuda.synchronize()
            ev[0].record()
            t0 = time.perf_counter()
            ctx.put_dev(planes, fence=True, **kw)
            host.append(1e3 * (time.perf_counter() - t0))
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        ctx.synchronize()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(BATCH):
            ctx.put_dev(planes, fence=False, **kw)
        ctx.dev_fence()
        ev[1].record()
        ev[1].synchronize()
        return ms, host, ev[0].elapsed_time(ev[1]) / BATCH

    def entry(ms, host, batch, bytes_per_element):
        b = 2 * ncolumns * nzp1 * bytes_per_element   # two planes; the cs sector of level 0 apart
        b += 2 * ncolumns * 64
        return {"event_ms": ms, "host_call_ms": host, "ms_per_call_of_%d_back_to_back" % BATCH: batch, "algorithmic_bytes": b,
                "GB_per_s_at_best": b / (min(ms) * 1e-3) / 1e9, "GB_per_s_back_to_back": b / (batch * 1e-3) / 1e9}

    d64 = {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in inc.items()}
    d32 = {n: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))).cuda() for n, v in inc.items()}
    out["add_f64"] = entry(*timed([(n, t) for n, t in d64.items()], op="add"), 8 + 8 + 8)
    out["add_f32"] = entry(*timed([(n, t) for n, t in d32.items()], op="add"), 4 + 8 + 8)
    now = {n: torch.empty((nzp1, npts), dtype=torch.float64, device="cuda") for n in inc}
    ctx.fetch_dev([(n, t) for n, t in now.items()], land_value=0.0)
    out["set_time_levels_f64"] = entry(*timed([(n, t) for n, t in now.items()], op="set", time_levels=True), 8 + 3 * 8)

    # the route a put replaces, in the same session
    host_inc = {n: np.asfortranarray(v.T) for n, v in inc.items()}
    rounds = []
    for _ in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.download(k3, A.F_RESTART)
        t1 = time.perf_counter()
        k3.X[:, :, 0] += host_inc["T"]
        k3.X[:, :, 1] += host_inc["S"]
        t2 = time.perf_counter()
        ctx.upload(k3)
        ctx.synchronize()
        t3 = time.perf_counter()
        rounds.append({"download_ms": 1e3 * (t1 - t0), "host_add_ms": 1e3 * (t2 - t1), "upload_ms": 1e3 * (t3 - t2),
                       "total_ms": 1e3 * (t3 - t0)})
    out["download_add_upload"] = {"first_round_pins_the_arrays": rounds[0], "later_rounds": rounds[1:],
                                  "prognostic_group_bytes_each_way": int(12 * npts * nzp1 * 8)}
    ctx.step(settle + 1, 1)   # the state is still one the model steps from
    st, nflag, _ = ctx.status()
    out["flagged_after_a_step"] = int(nflag)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["60", "shipped"])
    ap.add_argument("--limit", type=int, default=150, help="seconds a shape may take")
    ap.add_argument("--one", metavar="SHAPE", help="(internal) one shape in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one, a.ncol, a.settle, a.repeats)), flush=True)
        return
    for shape in a.shapes:   # a fresh process per shape, under its own time limit; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, "--ncol", str(a.ncol), "--settle",
                                str(a.settle), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"shape {shape}: no result within {a.limit} s")
        if r.returncode != 0:
            sys.exit(f"shape {shape}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
