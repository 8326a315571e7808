"""What it costs to bring a forced run's flux records to the device: set_flux_series before every chunk of steps against
the flux ring filled while the chunk before runs (include/mckpp_hip.h, mckpp_hip_flux_ring).

N steps with ndtocn 3 after a spin-up under constant forcing, fed in chunks of 4 records (12 steps), from the same
settled state, in a fresh process per way:
  (a) per chunk: set_flux_series of the chunk's records, then run_forced over its steps - the only way a library
      without the ring has;
  (b) a ring of 8 slots: the first chunk's records put, then per chunk run_forced and, right after it is queued, the
      next chunk's records put;
  (c) every record resident (one set_flux_series, outside the timed part), ONE run_forced: the floor;
  (s) nothing run: on an idle device, set_flux_series of one chunk's records (waited for: the call blocks) and the
      flux_ring_put calls of one chunk's records (the calls alone, then the wait for their copies), each chunk timed
      apart - what the feeding itself costs, without any wait for launches.
  (o) does a put's copy run under a launch?  A ring of 16 slots, 8 records put and waited for, ONE run_forced over their
      24 steps queued, then 4 more records put into slots the launch does not read, each call timed: the staging has
      two turns, so the third call returns when the first call's copy has completed, the fourth when the second's has.
      Beside them the launch's own time.
Per way: wall time from the first call to the end of a final synchronize, per step; seconds inside the set_flux_series
/ flux_ring_put calls (in (a) that includes the wait for the chunk before: replacing the series frees its block, which
waits for the device).  One JSON line per way, shape and repeat; the ways alternate within a repeat.
Usage: python tools/flux_ring_rate.py [--steps 72] [--settle 60] [--ncol 100000] [--repeats 3] [--shapes 60 shipped]
                                      [--ways a b c s o]"""
import argparse
import gc
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

NDTOCN, CHUNK_REC, NSLOTS = 3, 4, 8


def run(way, shape, ncol, settle, steps):
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)

    import common as cm
    import mckpp_f90_amd as mk

    ntotal = 100000
    idx = np.arange(0, ntotal, max(1, ntotal // ncol))[:ncol]
    if shape == "shipped":   # 69 stretched levels, 35 % land, dto 1200 s
        kc, k3 = cm.make_hip_case(len(idx), 69, grid="stretched", dto=1200.0, index=idx, ntotal=ntotal)
        land = (np.arange(len(idx)) * 7) % 20 < 7
        k3.run_physics[land] = 0
        k3.l_ocean[land] = 0
    else:
        kc, k3 = cm.make_hip_case(len(idx), int(shape), dto=1200.0, index=idx, ntotal=ntotal)
    npts = len(idx)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    nt0 = settle + 1
    assert settle % NDTOCN == 0 and steps % (NDTOCN * CHUNK_REC) == 0
    rec0, nrec = settle // NDTOCN, steps // NDTOCN
    # record r of the run is what the reader holds at step r * ndtocn + 1
    rec = np.ascontiguousarray(cm.synth.flux_series(npts, nt0, steps, kc.dto, "bench", idx)[::NDTOCN])
    assert rec.shape == (nrec, 8, npts)
    nchunks, per = nrec // CHUNK_REC, CHUNK_REC * NDTOCN
    if way == "s":
        set_ms, put_ms, put_done_ms = [], [], []
        for k in range(nchunks):
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.set_flux_series(rec0 + k * CHUNK_REC, rec[k * CHUNK_REC:(k + 1) * CHUNK_REC])
            set_ms.append(1e3 * (time.perf_counter() - t1))
        ctx.flux_ring(NSLOTS)
        for k in range(nchunks):
            t1 = time.perf_counter()
            for r in range(k * CHUNK_REC, (k + 1) * CHUNK_REC):
                ctx.flux_ring_put(rec0 + r, rec[r])
            put_ms.append(1e3 * (time.perf_counter() - t1))
            ctx.flux_ring(NSLOTS)   # (cancelling waits for the transfer stream; a new ring takes any first record)
            put_done_ms.append(1e3 * (time.perf_counter() - t1))
        ctx.close()
        return {"way": way, "shape": f"{npts} x {shape}", "chunk_records": CHUNK_REC, "record_bytes_host": 8 * 8 * npts,
                "set_flux_series_ms_per_chunk": set_ms, "flux_ring_put_calls_ms_per_chunk": put_ms,
                "flux_ring_put_until_arrived_ms_per_chunk": put_done_ms, "build": mk.api.build_id()}
    if way == "o":
        ctx.flux_ring(16)
        for r in range(8):
            ctx.flux_ring_put(rec0 + r, rec[r])
        ctx.synchronize()
        time.sleep(0.05)   # (the 8 copies: nothing waits for them but a launch)
        t0 = time.perf_counter()
        ctx.run_forced(nt0, 8 * NDTOCN, NDTOCN)
        queued_ms = 1e3 * (time.perf_counter() - t0)
        put_ms = []
        for r in range(8, 12):
            t1 = time.perf_counter()
            ctx.flux_ring_put(rec0 + r, rec[r])
            put_ms.append(1e3 * (time.perf_counter() - t1))
        puts_done_ms = 1e3 * (time.perf_counter() - t0)
        ctx.synchronize()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        kernel_ms = ctx.last_kernel_ms()[0]
        ctx.close()
        return {"way": way, "shape": f"{npts} x {shape}", "run_forced_call_ms": queued_ms, "put_call_ms": put_ms,
                "puts_returned_after_ms": puts_done_ms, "launch_done_after_ms": wall_ms, "launch_kernel_ms": kernel_ms,
                "build": mk.api.build_id()}
    if way == "b":
        ctx.flux_ring(NSLOTS)
    if way == "c":
        ctx.set_flux_series(rec0, rec)
    ctx.synchronize()
    feed_s = 0.0
    t0 = time.perf_counter()
    if way == "a":
        for k in range(nchunks):
            t1 = time.perf_counter()
            ctx.set_flux_series(rec0 + k * CHUNK_REC, rec[k * CHUNK_REC:(k + 1) * CHUNK_REC])
            feed_s += time.perf_counter() - t1
            ctx.run_forced(nt0 + k * per, per, NDTOCN)
    elif way == "b":
        for k in range(nchunks + 1):
            if k > 0:
                ctx.run_forced(nt0 + (k - 1) * per, per, NDTOCN)
            if k < nchunks:   # the next chunk's records, under the chunk just queued
                t1 = time.perf_counter()
                for r in range(k * CHUNK_REC, (k + 1) * CHUNK_REC):
                    ctx.flux_ring_put(rec0 + r, rec[r])
                feed_s += time.perf_counter() - t1
    else:
        ctx.run_forced(nt0, steps, NDTOCN)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    st, nflag, _ = ctx.status()
    build = mk.api.build_id()
    ncolumns = int(ctx.ncolumns)
    ctx.download(k3, mk.api.F_SCALARS)
    hmix = float(np.asarray(k3.hmix)[np.asarray(k3.run_physics) != 0].mean())
    ctx.close()
    del ctx, k3
    gc.collect()
    return {"way": way, "shape": f"{npts} x {shape}", "resident_columns": ncolumns, "steps": steps, "chunks": nchunks,
            "wall_s": wall, "wall_ms_per_step": 1e3 * wall / steps, "feed_s": feed_s, "feed_ms_per_chunk": 1e3 * feed_s / nchunks,
            "record_bytes_host": 8 * 8 * npts, "flagged": int(nflag), "mean_hmix": hmix, "build": build}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["60", "shipped"])
    ap.add_argument("--ways", nargs="+", default=["a", "b", "c"])
    ap.add_argument("--one", nargs=2, metavar=("WAY", "SHAPE"), help="(internal) one way of one shape in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one[0], a.one[1], a.ncol, a.settle, a.steps)), flush=True)
        return
    for shape in a.shapes:
        for rep in range(a.repeats):
            for way in a.ways:   # a fresh process per way: its own device memory
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", way, shape, "--steps", str(a.steps),
                                    "--settle", str(a.settle), "--ncol", str(a.ncol)], capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    sys.exit(f"way {way}, shape {shape}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                line["repeat"] = rep
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
