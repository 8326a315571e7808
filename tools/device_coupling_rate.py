"""What a coupling interval costs through host arrays and through device arrays (include/mckpp_hip_device.h).

A coupled run cuts into intervals of ndtocn = 3 steps: forcing in, three steps, surface fields out.  After a spin-up
under constant forcing, from the same settled state, in a fresh process per way:
  (a)  the host path: fluxes + step(nt, 3) + window_fetch of T, u, v and hmix - what a library without the device-array
       interface offers (window_fetch has no level range: the three profiles cross the bus whole);
  (b)  the device path: fluxes_dev + step(nt, 3) + ONE fetch_dev of T[0:1], u[0:1], v[0:1] and hmix, the forcing
       records resident as torch tensors, a torch consumer of the sea-surface temperature behind every delivery; no host
       wait inside the loop.  Beside it the times of k_fluxes_dev and k_fetch_planes on an idle device, from HIP events
       on the caller's stream around the call (they include the two event waits that order the call);
  (rh) a ring of 8 slots fed by flux_ring_put, as way (b) of tools/flux_ring_rate.py: per chunk of 4 records run_forced
       and, right after it is queued, the next chunk's records put;
  (rd) the same ring fed by flux_ring_put_dev from resident tensors;
  (o)  what does a device put do under a running launch?  8 records resident, ONE run_forced over their 24 steps queued,
       then 4 records put from device arrays into slots the launch does not read: the calls' times, when the four
       gathers have run (a fence on a side stream, then a host wait for that stream) and when the launch has.
One JSON line per way, shape and repeat; the ways alternate within a repeat.  Every way runs under a time limit of its
own and the first failure ends the run.
Usage: python tools/device_coupling_rate.py [--intervals 24] [--settle 60] [--ncol 100000] [--repeats 3]
                                            [--shapes 60 shipped] [--ways a b rh rd o]"""
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

NDTOCN, CHUNK_REC, NSLOTS = 3, 4, 8
FLSN, EL = 334000.0, 2.5e6


def run(way, shape, ncol, settle, intervals):
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
    nt0, steps = settle + 1, intervals * NDTOCN
    assert settle % NDTOCN == 0 and intervals % CHUNK_REC == 0
    rec0 = settle // NDTOCN
    rec = np.ascontiguousarray(cm.synth.flux_series(npts, nt0, steps, kc.dto, "bench", idx)[::NDTOCN])
    assert rec.shape == (intervals, 8, npts)
    base = {"way": way, "shape": f"{npts} x {shape}", "intervals": intervals, "build": A.build_id()}

    def finish(out):
        st, nflag, _ = ctx.status()
        out.update(resident_columns=int(ctx.ncolumns), flagged=int(nflag))
        ctx.download(k3, A.F_SCALARS)
        out["mean_hmix"] = float(np.asarray(k3.hmix)[np.asarray(k3.run_physics) != 0].mean())
        ctx.close()
        return out

    if way == "a":
        prof = [np.zeros((npts, nzp1), order="F") for _ in range(3)]
        hmix = np.zeros(npts)
        ctx.synchronize()
        t0 = time.perf_counter()
        for k in range(intervals):
            nt = nt0 + k * NDTOCN
            ctx.fluxes(nt, *rec[k], flsn=FLSN, el=EL)
            ctx.step(nt, NDTOCN)
            for f, o in zip(("T", "u", "v"), prof):
                ctx.window_fetch(A.OUT[f], A.OP_INSTANT, o)
            ctx.window_fetch(A.OUT["hmix"], A.OP_INSTANT, hmix)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        return finish(dict(base, wall_s=wall, wall_ms_per_interval=1e3 * wall / intervals,
                           bytes_over_the_bus_per_interval=8 * npts * (8 + 3 * nzp1 + 1), sst_sum=float(prof[0][:, 0].sum())))
    recd = torch.from_numpy(rec).cuda()
    if way == "b":
        out4 = [torch.zeros((1, npts), dtype=torch.float64, device="cuda") for _ in range(4)]
        planes = [("T", out4[0], 0, 1), ("u", out4[1], 0, 1), ("v", out4[2], 0, 1), ("hmix", out4[3], 0, 1)]
        acc = torch.zeros(npts, dtype=torch.float64, device="cuda")
        # the two kernels alone, on an idle device
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        k_ms = {"fluxes_dev": [], "fetch_dev": []}
        ctx.fetch_dev(planes, land_value=0.0)   # (first use builds the list of land points)
        for _ in range(5):
            for name, call in (("fluxes_dev", lambda: ctx.fluxes_dev(nt0, recd[0], flsn=FLSN, el=EL, fence=True)),
                               ("fetch_dev", lambda: ctx.fetch_dev(planes, land_value=0.0))):
                ctx.synchronize()
                torch.cuda.synchronize()
                ev[0].record()
                call()
                ev[1].record()
                ev[1].synchronize()
                k_ms[name].append(ev[0].elapsed_time(ev[1]))
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(intervals):
            nt = nt0 + k * NDTOCN
            ctx.fluxes_dev(nt, recd[k], flsn=FLSN, el=EL, fence=False)
            ctx.step(nt, NDTOCN)
            ctx.fetch_dev(planes, land_value=0.0)
            acc.add_(out4[0][0])   # the consumer: behind the delivery, on torch's stream
        queued = time.perf_counter() - t0
        torch.cuda.synchronize()
        ctx.synchronize()
        wall = time.perf_counter() - t0
        return finish(dict(base, wall_s=wall, wall_ms_per_interval=1e3 * wall / intervals, host_queued_all_after_s=queued,
                           bytes_over_the_bus_per_interval=0, k_fluxes_dev_call_ms=k_ms["fluxes_dev"],
                           k_fetch_planes_call_ms=k_ms["fetch_dev"], sst_sum=float(out4[0].sum().item())))
    if way == "o":
        ctx.flux_ring(16)
        for r in range(8):
            ctx.flux_ring_put_dev(rec0 + r, recd[r])
        side = torch.cuda.Stream()
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.run_forced(nt0, 8 * NDTOCN, NDTOCN, flsn=FLSN, el=EL)
        queued_ms = 1e3 * (time.perf_counter() - t0)
        put_ms = []
        for r in range(8, 12):
            t1 = time.perf_counter()
            ctx.flux_ring_put_dev(rec0 + r, recd[r])
            put_ms.append(1e3 * (time.perf_counter() - t1))
        puts_returned_ms = 1e3 * (time.perf_counter() - t0)
        ctx.dev_fence(side)
        side.synchronize()
        gathers_done_ms = 1e3 * (time.perf_counter() - t0)
        ctx.synchronize()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        kernel_ms = ctx.last_kernel_ms()[0]
        ctx.close()
        return dict(base, run_forced_call_ms=queued_ms, put_dev_call_ms=put_ms, puts_returned_after_ms=puts_returned_ms,
                    gathers_done_after_ms=gathers_done_ms, launch_done_after_ms=wall_ms, launch_kernel_ms=kernel_ms)
    # rh / rd: the ring, the next chunk put right after the current chunk's run_forced is queued
    put = (lambda r: ctx.flux_ring_put(rec0 + r, rec[r])) if way == "rh" else (lambda r: ctx.flux_ring_put_dev(rec0 + r, recd[r]))
    nchunks, per = intervals // CHUNK_REC, CHUNK_REC * NDTOCN
    ctx.flux_ring(NSLOTS)
    ctx.synchronize()
    torch.cuda.synchronize()
    feed_s = 0.0
    t0 = time.perf_counter()
    for k in range(nchunks + 1):
        if k > 0:
            ctx.run_forced(nt0 + (k - 1) * per, per, NDTOCN, flsn=FLSN, el=EL)
        if k < nchunks:
            t1 = time.perf_counter()
            for r in range(k * CHUNK_REC, (k + 1) * CHUNK_REC):
                put(r)
            feed_s += time.perf_counter() - t1
    ctx.synchronize()
    wall = time.perf_counter() - t0
    return finish(dict(base, steps=steps, chunks=nchunks, wall_s=wall, wall_ms_per_step=1e3 * wall / steps, feed_s=feed_s,
                       feed_ms_per_chunk=1e3 * feed_s / nchunks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=24)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["60", "shipped"])
    ap.add_argument("--ways", nargs="+", default=["a", "b", "rh", "rd", "o"])
    ap.add_argument("--limit", type=int, default=120, help="seconds a way may take")
    ap.add_argument("--one", nargs=2, metavar=("WAY", "SHAPE"), help="(internal) one way of one shape in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one[0], a.one[1], a.ncol, a.settle, a.intervals)), flush=True)
        return
    for shape in a.shapes:
        for rep in range(a.repeats):
            for way in a.ways:   # a fresh process per way, under its own time limit; the first failure ends the run
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", way, shape, "--intervals",
                                        str(a.intervals), "--settle", str(a.settle), "--ncol", str(a.ncol)],
                                       capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    sys.exit(f"way {way}, shape {shape}: no result within {a.limit} s")
                if r.returncode != 0:
                    sys.exit(f"way {way}, shape {shape}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                line["repeat"] = rep
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
