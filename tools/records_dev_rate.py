"""What a coupling interval costs when the interval MEANS go to a partner on the GPU: through the export and back over the
bus, or through mckpp_hip_records_dev (include/mckpp_hip_device_records.h).

A coupled run cuts into intervals of K = 3 steps.  A level-0 zoomed schedule keeps the interval mean of T, u, v and hmix
(period K).  The forcing records are resident as torch tensors and go in through fluxes_dev in both ways; after a
spin-up under constant forcing, from the same settled state, in a fresh process per way:
  (h)  the host route, what the library offered before: a ring of two records with an f8 export; per interval
       fluxes_dev + step(nt, K) + window_export_fetch_record of the four planes into pinned host memory (it ends with a
       host wait) + one host-to-device copy into the partner's tensor + release;
  (d)  the device route: a ring of ONE record; per interval fluxes_dev + step(nt, K) + ONE records_dev of the four
       planes + release at once; no host wait inside the loop.  Beside it the time of the delivery on an idle device,
       from HIP events on the caller's stream around the call (they include the two event waits that order the call).
In both a torch consumer reads the mean SST behind every delivery.  One JSON line per way, shape and repeat; the ways
alternate within a repeat.  Every way runs under a time limit of its own and the first failure ends the run.
Usage: python tools/records_dev_rate.py [--intervals 24] [--settle 60] [--ncol 100000] [--repeats 3]
                                        [--shapes 60 shipped] [--ways h d]"""
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

K = 3
FLSN, EL = 334000.0, 2.5e6
NAMES = ("T", "u", "v", "hmix")


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
    npts = len(idx)
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(npts, "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    assert settle % K == 0
    ctx.step(1, settle)
    nt0 = settle + 1
    rec = np.ascontiguousarray(cm.synth.flux_series(npts, nt0, intervals * K, kc.dto, "bench", idx)[::K])
    recd = torch.from_numpy(rec).cuda()
    acc = torch.zeros(npts, dtype=torch.float64, device="cuda")
    base = {"way": way, "shape": f"{npts} x {shape}", "intervals": intervals, "steps_per_interval": K, "build": A.build_id()}
    ctx.window_schedule_zoom(0, nt0, K, 2 if way == "h" else 1, NAMES, A.WIN_MEAN, levels=(0, 1))

    def finish(out):
        st, nflag, _ = ctx.status()
        out.update(resident_columns=int(ctx.ncolumns), flagged=int(nflag), sst_mean_sum=float(acc.sum().item()))
        ctx.close()
        return out

    if way == "h":
        ctx.window_export(0, "f8", 0.0)
        layout, nbytes = ctx.window_export_layout(0)
        assert nbytes >= 4 * 8 * npts and [p[2] for p in layout] == [1] * 4
        host = [torch.zeros(nbytes // 8, dtype=torch.float64).pin_memory() for _ in range(2)]   # used in turn
        dev = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
        sst = dev[layout[0][3] // 8:][:npts]
        for k in range(intervals):   # (the first interval is not timed, in either way)
            if k == 1:
                ctx.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            nt = nt0 + k * K
            ctx.fluxes_dev(nt, recd[k], flsn=FLSN, el=EL, fence=False)
            ctx.step(nt, K)
            ctx.window_export_fetch_record(0, k, host[k % 2].numpy())
            ctx.window_record_release(0, k)
            dev.copy_(host[k % 2], non_blocking=True)
            acc.add_(sst)   # the consumer: behind the copy, on torch's stream
        torch.cuda.synchronize()
        ctx.synchronize()
        wall = time.perf_counter() - t0
        return finish(dict(base, timed_intervals=intervals - 1, wall_s=wall, wall_ms_per_interval=1e3 * wall / (intervals - 1),
                           bytes_over_the_bus_per_interval=2 * nbytes))
    out4 = [torch.zeros((1, npts), dtype=torch.float64, device="cuda") for _ in NAMES]

    def planes(k):
        return [(0, k, n, A.OP_MEAN, o, 0, 1) for n, o in zip(NAMES, out4)]

    # the delivery alone, on an idle device: the first interval's record, delivered five times before it is released
    ctx.fluxes_dev(nt0, recd[0], flsn=FLSN, el=EL, fence=False)
    ctx.step(nt0, K)
    ctx.records_dev(planes(0), land_value=0.0)   # (first use builds the list of land points)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    call_ms = []
    for _ in range(5):
        ctx.synchronize()
        torch.cuda.synchronize()
        ev[0].record()
        ctx.records_dev(planes(0), land_value=0.0)
        ev[1].record()
        ev[1].synchronize()
        call_ms.append(ev[0].elapsed_time(ev[1]))
    ctx.window_record_release(0, 0)
    acc.add_(out4[0][0])
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(1, intervals):
        nt = nt0 + k * K
        ctx.fluxes_dev(nt, recd[k], flsn=FLSN, el=EL, fence=False)
        ctx.step(nt, K)
        ctx.records_dev(planes(k), land_value=0.0)
        ctx.window_record_release(0, k)
        acc.add_(out4[0][0])   # the consumer: behind the delivery, on torch's stream
    queued = time.perf_counter() - t0
    torch.cuda.synchronize()
    ctx.synchronize()
    wall = time.perf_counter() - t0
    return finish(dict(base, timed_intervals=intervals - 1, wall_s=wall, wall_ms_per_interval=1e3 * wall / (intervals - 1),
                       host_queued_all_after_s=queued, bytes_over_the_bus_per_interval=0, k_record_planes_call_ms=call_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=24)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["60", "shipped"])
    ap.add_argument("--ways", nargs="+", default=["h", "d"])
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
