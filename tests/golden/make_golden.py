#!/usr/bin/env python3
"""Generate the committed golden vectors from the COMPILED REFERENCE.

Run in the build container (needs /root/reference and `make -C oracle ref`):
    python tests/golden/make_golden.py

Produces (inputs + expected outputs only, no reference source):
  eos_ref.npz   - mckpp_abk80 / mckpp_cpsw of the reference
                  (src/mckpp_physics_state_equations.F90) on 4096 (S,T,P) points
  z121_ref.npz  - mckpp_physics_verticalmixing_z121 of the reference
                  (src/mckpp_physics_verticalmixing_z121_mod.F90) on 64 vectors
  eos_ref_checks.json - what tests/test_oracle_cpu.py compares with the compiled reference where it is built:
                  SHA-256 digests of mckpp_abk80 / mckpp_cpsw on its 1e6 seeded points, and mckpp_abk80 on
                  every entry path (`python tests/golden/make_golden.py checks` writes this file alone)
The reference's whole physics step is recorded by the sibling script make_ref_step_golden.py
(tests/golden/ref_step.npz; DESIGN.md section 4, "What pins it").
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import orc  # noqa: E402

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes: equal digests <=> bit-identical arrays."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


EOS_NAMES = ("alpha", "beta", "sig0", "sig", "cp")


def eos_points_1e6():
    """The 1e6 (S, T, P) points of test_eos_vs_compiled_reference_1e6."""
    rng = np.random.default_rng(7)
    n = 1_000_000
    return rng.uniform(0, 42, n), rng.uniform(-4, 35, n), rng.uniform(0.05, 6000, n)


def eos_batch(L, prefix, s, t, p):
    """alpha, beta, sig0, sig, cp of <prefix>_abk80_batch / <prefix>_cpsw_batch (L: the oracle or the reference)."""
    n = len(s)
    o = [np.zeros(n) for _ in range(5)]
    getattr(L, prefix + "_abk80_batch")(n, dp(s), dp(t), dp(p), *[dp(x) for x in o[:4]])
    getattr(L, prefix + "_cpsw_batch")(n, dp(s), dp(t), dp(p), dp(o[4]))
    return dict(zip(EOS_NAMES, o))


# P = 0 short-cuts and the kappa-only / alpha-only entry paths of mckpp_abk80
ABK80_POINTS = ((35.0, 10.0, 0.0), (0.0, 4.0, 0.0), (35.0, 10.0, 500.0), (20.0, -5.0, 50.0))
ABK80_FLAGS = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 0, 0))


def abk80_paths(fn):
    """(alpha, beta, kappa, sig0, sig) of `fn` (orc_abk80 or ref_abk80) at every ABK80_POINTS x ABK80_FLAGS entry."""
    res = []
    for S, T, P in ABK80_POINTS:
        for a0, b0, k0 in ABK80_FLAGS:
            a, b, k, s0, s = (C.c_double(v) for v in (a0, b0, k0, 9.0, 9.0))
            fn(S, T, P, C.byref(a), C.byref(b), C.byref(k), C.byref(s0), C.byref(s))
            res.append((a.value, b.value, k.value, s0.value, s.value))
    return res


def write_checks(R):
    pts = eos_points_1e6()
    out = eos_batch(R, "ref", *pts)
    checks = {
        "eos_1e6": {"inputs_sha256": digest(np.stack(pts)), "sha256": {k: digest(v) for k, v in out.items()}},
        "abk80_paths": [[float.hex(v) for v in r] for r in abk80_paths(R.ref_abk80)],
    }
    with open(os.path.join(HERE, "eos_ref_checks.json"), "w") as f:
        json.dump(checks, f, indent=1)
        f.write("\n")


def main():
    assert orc.have_ref(), "oracle/_ref/libmckpp_ref.so missing (make -C oracle ref)"
    R = orc.ref()
    rng = np.random.default_rng(20261003)
    n = 4096
    s = rng.uniform(0.0, 42.0, n)
    t = rng.uniform(-4.0, 35.0, n)       # includes T < -2 (clamped in the reference)
    p = rng.uniform(0.05, 6000.0, n)
    # include the model's own operating points: fresh water / brine at the surface
    s[:8] = [0.0, 4.0, 35.0, 35.0, 40.0, 0.0, 4.0, 34.5]
    t[:8] = [10.0, 10.0, 15.0, -3.0, 0.0, 28.0, 28.0, 2.0]
    p[:8] = [2.5, 2.5, 1.6667, 100.0, 1000.0, 1.0, 1.0, 200.0]
    alpha, beta, sig0, sig, cp = (np.zeros(n) for _ in range(5))
    R.ref_abk80_batch(n, dp(s), dp(t), dp(p), dp(alpha), dp(beta), dp(sig0), dp(sig))
    R.ref_cpsw_batch(n, dp(s), dp(t), dp(p), dp(cp))
    np.savez_compressed(os.path.join(HERE, "eos_ref.npz"), s=s, t=t, p=p, alpha=alpha, beta=beta,
                        sig0=sig0, sig=sig, cp=cp)
    vin, vout, wout, kms = [], [], [], []
    for i in range(64):
        km = int(rng.integers(3, 110))
        v = rng.uniform(-0.6, 1.6, km + 2)
        if i % 4 == 0:
            v[rng.integers(1, km + 1, 3)] = [0.0, 0.8, -1e-30]   # edge values of the weight test
        w = rng.uniform(0, 1, km + 2)
        vi = np.zeros(112); vi[:km + 2] = v
        R.ref_z121(km + 1, 0.0, 0.8, dp(v), dp(w))
        vo = np.zeros(112); vo[:km + 2] = v
        wo = np.zeros(112); wo[:km + 2] = w
        vin.append(vi); vout.append(vo); wout.append(wo); kms.append(km)
    np.savez_compressed(os.path.join(HERE, "z121_ref.npz"), km=np.array(kms), vin=np.array(vin),
                        vout=np.array(vout), wout=np.array(wout))
    write_checks(R)
    print("wrote eos_ref.npz, z121_ref.npz, eos_ref_checks.json")


if __name__ == "__main__":
    if sys.argv[1:] == ["checks"]:
        assert orc.have_ref(), "oracle/_ref/libmckpp_ref.so missing (make -C oracle ref)"
        write_checks(orc.ref())
    else:
        main()
