#!/usr/bin/env python3
"""Record the COMPILED REFERENCE's own init, flux assembly and time loop on the cases of tests/ref_loop_cases.py.

Run where the reference's sources are mounted (`make -C oracle ref` builds oracle/_ref/libmckpp_ref_step.so and
oracle/_ref/libmckpp_ref_step_pexp.so from them):
    python tests/golden/make_ref_loop_golden.py

Produces tests/golden/ref_loop.npz (digests of the inputs and recorded outputs only, no reference source).  For every
case and each build - `libm` (EXP = libm exp, as amdflang builds the reference) and `pexp` (EXP = the project's
portable exp, what the oracle's exp_mode=1 and the HIP kernels use):
  <case>/<build>/input_sha   SHA-256 of what the run is given (raw profiles, flux records, masks, switches): generator
                             drift fails loudly
  <case>/<build>/init_sha    [field, 32] SHA-256 of each field of `init_fields` after the reference's
                             mckpp_initialize_time / _fluxes / _ocean_model, over the columns the reference works on
                             (all but land); tri0, tri1 are tri(0:nz,0,1), tri(0:nz,1,1) as its init computed them
  <case>/<build>/sha         [step, field, 32] the same for each field of `loop_fields` after each step of its loop
  <case>/pexp/val/<field>    T, hmix, kmix, wXNT1 and the six sflux rows after the last step in full (small cases)
  init_fields, loop_fields   the field names, in tests/ref_loop_cases.py's INIT_FIELDS / LOOP_FIELDS order
Digests and values are taken after -0.0 -> +0.0 and NaN -> one NaN (tests/ref_step_cases.py: canonical).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loop_cases as lc  # noqa: E402
from oracle import orc  # noqa: E402


def main():
    if not orc.have_ref_step():
        raise SystemExit("the reference's step is not built (make -C oracle ref, with the reference's sources mounted)")
    out = {"init_fields": np.array(lc.INIT_FIELDS), "loop_fields": np.array(lc.LOOP_FIELDS)}
    for tag, case in lc.CASES.items():
        for b, em in lc.BUILDS.items():
            _, ob, _ = lc.oracle_raw(case, em)
            init, steps = lc.run_reference(case, em)
            out[f"{tag}/{b}/input_sha"] = lc.input_digest(case, ob, lc.flux_records(case))
            for k, v in lc.record(case, init, steps).items():
                if b == "pexp" or not k.startswith("val/"):
                    out[f"{tag}/{b}/{k}"] = v
        print(tag, "recorded", file=sys.stderr, flush=True)
    path = os.path.join(HERE, "ref_loop.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
