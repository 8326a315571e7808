#!/usr/bin/env python3
"""Which branches of the oracle's physics do the suite's inputs take?

The column kernel is asserted equal to the oracle (oracle/mckpp_oracle.c) bit for bit, so an oracle branch that no
test input takes is a kernel branch that no test checks.  This script builds the oracle with `gcc --coverage` into a
temporary directory, drives it with the oracle half of the suite's inputs, and prints the branches of the physics
functions (ddmix ... check_profile) that were never taken, with their source text:

  before   the generators' inputs: the bench mix at 40/60/69/100 levels, the 72- and 48-step diurnal runs, the seeded
           sweep of shapes and forcings, the two-ended-solver depths, and the cases of tests/ref_step_cases.py that
           are not regime cases (without the 2000-column one)
  after    the same plus the regime cases (rc.REGIME_CASES)
  pinned   the same plus the advection, precedence and trap_v cases (rc.ADVECTION_CASES, rc.PRECEDENCE_CASES, trap_v_*):
           every input of this phase is also run through the reference's own compiled step

    python tools/oracle_coverage.py > profiles/coverage/oracle_branches.md

Needs gcc and gcov.  Not run by any test."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ("before", "after", "pinned")
FIRST = "static void ddmix("      # the physics: from ddmix to the end of check_profile


def drive(phase):
    """the oracle half of the suite's inputs, in this process (the instrumented library is already selected)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np

    import common as cm
    import ref_step_cases as rc
    from oracle import orc

    def run(ncol, nz, nsteps, grid="uniform", dto=3600.0, diurnal=False, **sw):
        oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid, dto=dto, **sw)
        orc.init_ocean(oc, ob, 0)
        for nt in range(1, nsteps + 1):
            ob["sflux"] = cm.synth.forcing(ncol, "bench", t_seconds=(nt - 1) * dto if diurnal else None)
            orc.physics_driver(oc, ob, nt)

    if phase == "before":
        for nz, grid in ((40, "uniform"), (60, "uniform"), (69, "stretched"), (100, "uniform")):
            run(300, nz, 3, grid=grid)
            run(130, nz, 2, grid=grid, solver_mode=1)
        run(300, 60, 72, diurnal=True)
        run(300, 69, 48, grid="stretched", dto=1200.0, diurnal=True)
        rng = np.random.default_rng(20261003)      # tests/test_parity_gpu.py: test_seeded_sweep_of_shapes_and_forcings
        depths = [2, 3, 4, 5, 7, 12, 23, 31, 32, 33, 47, 59, 60, 61, 62, 63, 64, 65, 77, 96, 124, 125, 126, 127, 128,
                  160, 188, 189, 190, 255, 300, 509]
        for i, nz in enumerate(depths):
            grid = "stretched" if (i % 3 == 1 and nz >= 10) else "uniform"
            dto = [3600.0, 1200.0, 900.0][i % 3]
            ncol = int(rng.integers(3, 40))
            oc, ob = cm.make_oracle(ncol, nz, init=False, exp_mode=1, grid=grid, dto=dto)
            rng.integers(0, 6)
            ob["jerlov"] = rng.integers(1, 6, ncol).astype(np.int32)
            orc.init_ocean(oc, ob, 0)
            r2 = np.random.default_rng(1000 + i)
            for nt in (1, 2, 3):
                sf = cm.synth.forcing(ncol, "bench", t_seconds=(nt - 1) * dto + 6 * 3600.0)
                sf[:, 0] *= r2.uniform(0.0, 3.0, ncol)
                sf[:, 1] = r2.uniform(-0.2, 0.2, ncol)
                sf[:, 3] *= r2.uniform(0.0, 2.0, ncol)
                sf[:, 5] += r2.uniform(-1e-4, 1e-4, ncol)
                ob["sflux"] = sf
                orc.physics_driver(oc, ob, nt)
    def phase_of(t):
        if t in rc.REGIME_CASES:
            return "after"
        return "pinned" if t in rc.ADVECTION_CASES + rc.PRECEDENCE_CASES or t.startswith("trap_v_") else "before"
    tags = [t for t in rc.CASES if phase_of(t) == phase and rc.CASES[t].ncol < 2000]
    for tag in tags:
        case = rc.CASES[tag]
        oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
        for _ in rc.run_oracle(case, oc, ob):
            pass


def untaken(tmp):
    """[(line number, source text, [branch numbers never taken])] of the physics functions, from gcov -b -c"""
    subprocess.check_call(["gcov", "-b", "-c", "mckpp_oracle.c"], cwd=tmp,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out, inside, cur = [], False, None
    for line in open(os.path.join(tmp, "mckpp_oracle.c.gcov"), errors="replace"):
        m = re.match(r"\s*([^:]+):\s*(\d+):(.*)", line)
        if m:
            text = m.group(3)
            if text.startswith(FIRST):
                inside = True
            elif inside and text.startswith(("void ", "double ", "int ", "orc_batch")):
                inside = False            # the first function after check_profile
            cur = [int(m.group(2)), text.strip(), []] if inside else None
            if cur:
                out.append(cur)
            continue
        m = re.match(r"branch\s+(\d+) (never executed|taken 0)", line)
        if m and cur is not None:
            cur[2].append(int(m.group(1)))
    return [c for c in out if c[2]]


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--drive":
        return drive(sys.argv[2])
    with tempfile.TemporaryDirectory() as tmp:
        for f in ("mckpp_oracle.c", "mckpp_oracle.h"):
            with open(os.path.join(ROOT, "oracle", f)) as src, open(os.path.join(tmp, f), "w") as dst:
                dst.write(src.read())
        lib = os.path.join(tmp, "liboracle.so")
        subprocess.check_call(["gcc", "--coverage", "-O0", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math",
                               "-c", "mckpp_oracle.c"], cwd=tmp)
        subprocess.check_call(["gcc", "--coverage", "-shared", "-o", lib, "mckpp_oracle.o", "-lm"], cwd=tmp)
        env = dict(os.environ, MCKPP_ORACLE_LIBRARY=lib)
        seen = {}
        for phase in PHASES:       # the counts of a phase add to those of the phases before it
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--drive", phase], env=env,
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            seen[phase] = untaken(tmp)
    def total(phase):
        return f"{sum(len(b) for _, _, b in seen[phase])} branches on {len(seen[phase])} lines"

    print("# Branches of the oracle's physics that the suite's inputs never take\n")
    print("Made by `tools/oracle_coverage.py` (gcc --coverage, gcov -b -c; line numbers of oracle/mckpp_oracle.c, from")
    print("ddmix to check_profile; a line with several conditions has several branches).  *Before*: the generators'")
    print("inputs and the cases of tests/ref_step_cases.py other than the regime cases.  *After*: with the regime cases.")
    print("*Pinned*: with the advection, precedence and trap_v cases, all of them recorded from the reference's own step.\n")
    print(f"Untaken before: {total('before')}; after: {total('after')}; pinned: {total('pinned')}.\n")
    print("| line | source | untaken before | after | pinned |\n|---|---|---|---|---|")
    for ln, text, br in seen["before"]:
        left = {ph: [b for l2, _, b2 in seen[ph] if l2 == ln for b in b2] for ph in PHASES[1:]}
        cells = " | ".join("taken" if not left[ph] else str(left[ph]) for ph in PHASES[1:])
        print(f"| {ln} | `{text.replace('|', chr(92) + '|')}` | {br} | {cells} |")
    print(NOTES)


NOTES = """
## What is left of rhsmod and of the precedence conditions, and why

- `FACT(n)` (1030, 1035, 1039, 1045, 1047, 1077): two branches each are `jsclr == 1` true and `jsclr == 2` false.  The
  reference's ocnint calls rhsmod for salinity alone (`jsclr = 2`, src/mckpp_physics_ocnint_mod.F90:182), and so does
  the oracle's: no input reaches them.
- 1042, the guard `n1 < nzi + 1` of mode 4's search: false only on a grid with no level below 100 m, where the
  reference reads past `zm` (src/mckpp_physics_solvers.F90:258-259).  The only input that reaches the branch is out
  of bounds in the reference, so it is not recorded; the device and the oracle are compared on it
  (tests/test_options_gpu.py, test_mode_4_on_a_grid_shallower_than_100_m_is_a_no_op).
- 1057 and 1068, the loops of modes 6 and 7 ending at nzi: mode 7 does (a 90 m grid); mode 6 cannot with km <= NZ,
  it meets dmax by n = km - 1 (tests/ref_step_cases.py, "prescribed advection").
- 1063, `mode == 7` false, which is a mode above 7: the reference aborts (solvers.F90:320-323), so none is recorded;
  the upload refuses such a mode (test_an_advection_mode_above_7_is_refused).
- 1237, `kmixn == NZP1`: bldepth leaves kbl in 2 .. NZ (bldepth_mod.F90:101-183 with km = NZ), so no input makes it
  true, in the reference or here.
- 1025 `mode <= 0`, 1120, 1129, 1132, 1151, 1158 and the V half of 1260 are taken by the pinned cases.
- The totals of *before* and *after* are three above those of the record made before the pinned cases (96 and 89):
  the guard gave line 1042 two more branches, the bit for the V half gave 1262 one more.
"""


if __name__ == "__main__":
    main()
