"""What it costs to bring a run's output records to the host: window_record_fetch after every chunk of steps against
the packed export fetched while the next chunk runs (include/mckpp_hip.h, mckpp_hip_window_export).

The shipped run/iodef.xml as schedules (dto 1200 s: an hour is 3 steps): schedule 0 the hourly instants of T, S and
hmix; schedule 1 the three-hourly mean, minimum and maximum of T, S and hmix (three files, one schedule: same period,
same fields); schedule 2 the three-hourly instants of every field a context without the optional physics offers (all
but scorr, tinc_fcorr, fcorr_z and sinc_fcorr: 31 of 35).  37 table entries of 64.  The same N steps in chunks of 9
from the same settled state, in a fresh process per form:
  (a) ONE run_forced of all steps, no output;
  (b) chunks of 9 steps, then window_record_fetch of every plane of the chunk's records, then release - the only form
      a library without the export has (--lib names such a library);
  (c) export "f8": queue chunk k+1, fetch chunk k's records with window_export_fetch_record, release;
  (d) the same with "f4";
  (c_kernel) ONE run_forced of all steps under the schedules and the export (rings of N / period records, nothing
      fetched): the pack launches' own cost, for the comparison with (a).
Per form: wall time end to end, ms per step from the kernel events where a form can read them without waiting ((a),
(b), (c_kernel); the events stop before the pack launches, so (c_kernel) also reports wall time), seconds inside the
fetch calls, bytes fetched.  One JSON line per form, shape and repeat; the forms alternate within a repeat.
Usage: python tools/export_rate.py [--steps 72] [--settle 60] [--ncol 100000] [--repeats 3] [--shapes 60 shipped]
                                   [--forms a b c d c_kernel] [--lib PARENT_LIBRARY_FOR_b]"""
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

CHUNK = 9
NO_ROWS = ("scorr", "tinc_fcorr", "fcorr_z", "sinc_fcorr")


def schedules(A):
    every = [n for n in A.OUT_FIELDS if n not in NO_ROWS]
    return [(3, ("T", "S", "hmix"), A.WIN_LAST), (9, ("T", "S", "hmix"), A.WIN_MEAN | A.WIN_MIN | A.WIN_MAX),
            (9, every, A.WIN_LAST)]


def run(form, shape, ncol, settle, steps):
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)

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
    ctx = mk.MckppHip(kc)
    ctx.upload(k3)
    ctx.init_ocean(0)
    cm.set_forcing_3d(k3, cm.synth.forcing(len(idx), "bench", index=idx))
    ctx.set_forcing(k3.sflux)
    ctx.step(1, settle)
    ctx.set_flux_series(settle, cm.synth.flux_series(len(idx), settle + 1, steps, kc.dto, "bench", idx))
    nt0, nchunks = settle + 1, steps // CHUNK
    sch = schedules(A)
    npts = len(idx)
    if form != "a":
        for s, (period, names, mask) in enumerate(sch):
            per_chunk = CHUNK // period
            ctx.window_schedule(s, nt0, period, steps // period if form == "c_kernel" else 2 * per_chunk, names, mask)
            if form in ("c", "d", "c_kernel"):
                ctx.window_export(s, "f4" if form == "d" else "f8")
    bufs, planes = {}, []
    if form == "b":
        for s, (period, names, mask) in enumerate(sch):
            for n in names:
                two_d = n == "hmix" or A.OUT[n] >= A.OUT["fcorr"]
                shp = (npts,) if two_d else (npts, kc.nzp1)
                for op in range(4):
                    if (mask >> op) & 1:
                        planes.append((s, period, n, op, np.zeros(shp, order="F")))
    if form in ("c", "d"):
        dt = np.float32 if form == "d" else np.float64
        for s, (period, names, mask) in enumerate(sch):
            rb = ctx.window_export_layout(s)[1]
            bufs[s] = [np.zeros(rb // np.dtype(dt).itemsize, dtype=dt) for _ in range(CHUNK // period)]
    ctx.synchronize()
    kernel_ms, fetch_s, nbytes = 0.0, 0.0, 0
    t0 = time.perf_counter()
    if form in ("a", "c_kernel"):
        ctx.run_forced(nt0, steps, 1)
        kernel_ms = ctx.last_kernel_ms()[0]
    elif form == "b":
        for k in range(nchunks):
            ctx.run_forced(nt0 + k * CHUNK, CHUNK, 1)
            kernel_ms += ctx.last_kernel_ms()[0]
            t1 = time.perf_counter()
            for s, period, n, op, out in planes:
                for r in range(k * (CHUNK // period), (k + 1) * (CHUNK // period)):
                    ctx.window_record_fetch(s, r, n, op, out)
                    nbytes += out.nbytes
            fetch_s += time.perf_counter() - t1
            for s, (period, _, _) in enumerate(sch):
                ctx.window_record_release(s, (k + 1) * (CHUNK // period) - 1)
    else:
        ctx.run_forced(nt0, CHUNK, 1)
        for k in range(1, nchunks + 1):
            if k < nchunks:
                ctx.run_forced(nt0 + k * CHUNK, CHUNK, 1)   # queued behind the chunk whose records are fetched now
            t1 = time.perf_counter()
            for s, (period, _, _) in enumerate(sch):
                for j, r in enumerate(range((k - 1) * (CHUNK // period), k * (CHUNK // period))):
                    ctx.window_export_fetch_record(s, r, bufs[s][j])
                    nbytes += bufs[s][j].nbytes
            fetch_s += time.perf_counter() - t1
            for s, (period, _, _) in enumerate(sch):
                ctx.window_record_release(s, k * (CHUNK // period) - 1)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    build = A.build_id()
    ncolumns = int(ctx.ncolumns)
    ctx.close()
    del ctx, k3
    gc.collect()
    return {"form": form, "shape": f"{npts} x {shape}", "resident_columns": ncolumns, "steps": steps, "wall_s": wall,
            "wall_ms_per_step": 1e3 * wall / steps, "kernel_ms_per_step": kernel_ms / steps if kernel_ms else None,
            "fetch_s": fetch_s, "bytes_fetched": nbytes, "build": build}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=72)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["60", "shipped"])
    ap.add_argument("--forms", nargs="+", default=["a", "b", "c", "d", "c_kernel"])
    ap.add_argument("--lib", default=None, help="library for form b (one built without the export)")
    ap.add_argument("--one", nargs=2, metavar=("FORM", "SHAPE"), help="(internal) one form of one shape in this process")
    a = ap.parse_args()
    assert a.steps % CHUNK == 0
    if a.one:
        print(json.dumps(run(a.one[0], a.one[1], a.ncol, a.settle, a.steps)), flush=True)
        return
    for shape in a.shapes:
        for rep in range(a.repeats):
            for form in a.forms:   # a fresh process per form: its own library, its own device memory
                env = dict(os.environ)
                if form == "b" and a.lib:
                    env["MCKPP_HIP_LIBRARY"] = os.path.abspath(a.lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", form, shape, "--steps", str(a.steps),
                                    "--settle", str(a.settle), "--ncol", str(a.ncol)], env=env, capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    sys.exit(f"form {form}, shape {shape}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                line["repeat"] = rep
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
