#!/usr/bin/env python3
"""Record the COMPILED REFERENCE's own physics step on the cases of tests/ref_step_cases.py.

Run where the reference's sources are mounted (`make -C oracle ref` builds oracle/_ref/libmckpp_ref_step.so and
oracle/_ref/libmckpp_ref_step_pexp.so from them):
    python tests/golden/make_ref_step_golden.py

Produces tests/golden/ref_step.npz (the inputs' digests and recorded outputs only, no reference source).  For every
case and each build - `libm` (EXP = libm exp, as amdflang builds the reference) and `pexp` (EXP = the project's
portable exp, what the oracle's exp_mode=1 and the HIP kernel use):
  <case>/<build>/input_sha   SHA-256 of the starting state (the oracle's state after init_ocean, which the HIP init
                             matches bit for bit, plus the forcing): generator drift fails loudly
  <case>/<build>/sha         [step, field, 32] SHA-256 of each field of `fields` after each step, over the columns
                             the reference steps (all but land columns)
  <case>/pexp/val/<field>    T, hmix, kmix after the last step in full (small cases), for the diagnosis of a mismatch
  fields                     the field names, in tests/ref_step_cases.py's STEP_FIELDS order
Digests and values are taken after -0.0 -> +0.0 and NaN -> one NaN (tests/ref_step_cases.py: canonical).

Every case is recorded anew, and every array the file already held has to come out byte for byte as it was: new cases
are added to a record, they never move it.  A case whose inputs or expected outputs are meant to change is removed
from the file first, by hand and for a stated reason.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_step_cases as rc  # noqa: E402
from oracle import orc  # noqa: E402

BUILDS = {"libm": 0, "pexp": 1}


def main():
    if not orc.have_ref_step():
        raise SystemExit("the reference's step is not built (make -C oracle ref, with the reference's sources mounted)")
    out = {"fields": np.array(rc.STEP_FIELDS)}
    for tag, case in rc.CASES.items():
        for b, em in BUILDS.items():
            oc, ob, _, _ = rc.oracle_start(case, exp_mode=em)
            digests, values = rc.record(case, rc.run_reference(case, oc, ob, em))
            out[f"{tag}/{b}/input_sha"] = rc.input_digest(ob)
            out[f"{tag}/{b}/sha"] = digests
            if b == "pexp":
                out.update({f"{tag}/{b}/val/{k}": v for k, v in values.items()})
        print(tag, "recorded", flush=True)
    path = os.path.join(HERE, "ref_step.npz")
    if os.path.exists(path):
        with np.load(path) as old:
            moved = [k for k in old.files if k not in out or out[k].dtype != old[k].dtype
                     or out[k].shape != old[k].shape or out[k].tobytes() != old[k].tobytes()]
            kept = len(old.files)
        if moved:
            raise SystemExit(f"{len(moved)} recorded arrays would change, the file is left as it was: {moved[:8]} ...")
        print(f"all {kept} arrays of the existing record are byte-identical; {len(out) - kept} added")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
