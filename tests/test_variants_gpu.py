"""The matrix of tests/variant_cases.py on the device: every instantiation of k_column_ps<XV, SM, LF> through the
launch forms it has to meet - the optional physics and double diffusion, both solvers, the kernels with the level count
as a literal and the general ones, on a mix of columns with stragglers, trapped and clamped columns and something for
every switch to act on (tests/test_variants_cpu.py asserts that on the oracle).

Bar: the project's own.  Every field of rc.STEP_FIELDS bit for bit over the active columns, the status words and the
pass counts, against the oracle stepped one model step at a time on the CPU - after every step for the forms that make
a call per step, after the last for those that take all steps in one call, and there the time levels' parity too (a
lost or repeated step shows in `old` and `new_`).  Never against another run of the kernel.

The tests cannot see which instantiation ran: the ids name what variant_cases.instantiation says, and of that the
library confirms what it can - kernel_name - and, for the forced geometries, the threads and the LDS of a workgroup."""
import numpy as np
import pytest

import common as cm
import variant_cases as vc
from harness import assert_equal_to_oracle, cleared, differing, mk  # noqa: F401

pytestmark = pytest.mark.gpu

_clean_env = cleared(vc.ENV)       # MCKPP_SOLVER_MODE among them: the suite is also run whole under MCKPP_SOLVER_MODE=1


@pytest.mark.parametrize("case", vc.MATRIX, ids=[c.id for c in vc.MATRIX])
def test_instantiation_through_the_launch_form(mk, monkeypatch, case):
    form = vc.FORMS[case.form]
    env, nz = case.env, case.nz
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run = vc.run_of(case)
    xv = case.instantiation[0]
    for again in range(form.runs):       # (F13 twice, for the races' sake)
        what = f"{case.id} {env}" + (f" run {again + 1}" if form.runs > 1 else "")
        oc, ob, land, kc, k3 = vc.start(case.set_name, case.solver, nz, case.grid, case.dto, case.ncol, hip=True)
        ctx = mk.MckppHip(kc)
        ctx.set_solver_mode(case.solver)
        ctx.upload(k3)
        ctx.init_ocean(0)
        ctx.download(k3)
        active = np.nonzero(k3.run_physics)[0]
        assert np.array_equal(active, run.active)
        bad = differing(k3, run.init, nz, active)
        assert not bad, f"{what} init: {bad}"
        assert ctx.kernel_name == ("k_column_ps<EXT>" if xv > 0 else "k_column_ps"), (what, ctx.kernel_name)
        cm.set_forcing_3d(k3, cm.synth.forcing(case.ncol, "bench"))
        ctx.set_forcing(k3.sflux)
        if form.one_call:
            ctx.step(1, form.nsteps)
        else:
            for nt in range(1, form.nsteps + 1):
                ctx.step(nt, 1)
                assert_equal_to_oracle(ctx, k3, run.steps[nt - 1], nz, active, f"{what} step {nt}")
        last = run.steps[-1]
        assert_equal_to_oracle(ctx, k3, last, nz, active, what)
        if form.one_call:
            assert np.array_equal(np.asarray(k3.old)[active], last["old"][active]), f"{what}: old"
            assert np.array_equal(np.asarray(k3.new_)[active], last["newi"][active]), f"{what}: new"
        if "MCKPP_PS" in env:
            slots, waves, per_cu = (int(x) for x in env["MCKPP_PS"].split("x"))
            asked, fit, threads, lds = ctx.kernel_residency()
            assert threads == 64 * waves, (what, threads)
            assert lds == vc.lds_bytes(nz + 3, slots, xv), (what, lds)
        ctx.close()
    if "MCKPP_L3_CAP" in env:
        assert np.any(last["kmix"][active] > int(env["MCKPP_L3_CAP"])), "no column deeper than the cap: nothing tested"
