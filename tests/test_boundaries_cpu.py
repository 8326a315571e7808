"""The edge cases of tests/ref_step_cases.py stay on their boundaries, and the record of the oracle's comparisons
(profiles/coverage/oracle_boundaries.md, made by tools/oracle_boundaries.py) is the one of the current source.

For every comparison the record classes *pinned*, that one mutant - the comparison swapped for its neighbour - is built
into a temporary directory with the tool's own site lookup and build line, and the case the record names for it has to
come out with another digest than from the unmutated build: generator drift that slides a case off its equality fails
here.  That the unmutated oracle reproduces the recorded reference on the edge cases is
tests/test_ref_step_cpu.py::test_oracle_matches_the_reference_step, which takes every case of rc.CASES."""
import os
import sys
import tempfile

import numpy as np
import pytest

import ref_step_cases as rc
from oracle import orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import oracle_boundaries as bnd  # noqa: E402
import oracle_boundaries_classes as cls  # noqa: E402

ROWS = bnd.parse_record()
PINNED = [r for r in ROWS if r[6].startswith("pinned: ")]
CLASSES = ("pinned", cls.SAME, cls.UNREAD, cls.UNREACHABLE, "not run by a step")


def test_record_lists_exactly_the_sites_of_the_source():
    """the lookup only, no mutant is built: function, source text and position of every row, in source order"""
    assert [r[:4] for r in ROWS] == [bnd.key(s) for s in bnd.sites()], \
        "profiles/coverage/oracle_boundaries.md is not the record of oracle/mckpp_oracle.c (run tools/oracle_boundaries.py)"
    for r in ROWS:
        if r[4] == "survived":
            assert r[6].split(":")[0] in CLASSES, f"{r[0]}: `{r[1]}` survives without a class"
            assert (r[5] == "killed") == r[6].startswith("pinned: "), r
            assert r[6].split(": ")[-1] in rc.EDGE_CASES or not r[6].startswith("pinned"), r
        else:
            assert r[5] == "killed" and r[6] == "-", r


def test_must_pin_sites_are_pinned_or_were_killed_before():
    """the comparisons whose equality is plainly constructible: none of them survives"""
    def row(function, fragment, occ=0):
        got = [r for r in ROWS if r[0] == function and fragment in r[1] and r[3] == occ]
        assert len(got) == 1, (function, fragment)
        return got[0]

    for function, fragment, occ in (("ddmix", "(aDT < 0.0) && (bDS < 0.0)", 1), ("ocnint", "relax_sst > 1.e-10", 0),
                                    ("ocnstep", "reset_flag > comp_iter_max", 0), ("ocnstep", "iter > (c->itermax + 1)", 0)):
        r = row(function, fragment, occ)
        assert r[5] == "killed", r
    # `betaDS > 0.` of the salt-finger arm adds exactly zero at betaDS == 0: no output can pin it (see the record)
    assert row("ddmix", "(aDT > bDS) && (bDS > 0.)", 1)[6] == cls.SAME


@pytest.fixture(scope="module")
def unmutated(built):
    """{edge case: digest} of the oracle built with the tool's own line"""
    with tempfile.TemporaryDirectory() as tmp:
        got = bnd.digests(bnd.build(tmp), "edges")
    assert got and sorted(got) == sorted(rc.EDGE_CASES)
    return got


@pytest.mark.parametrize("row", PINNED, ids=[f"{r[0]}-{r[2]}.{r[3]}-{i}" for i, r in enumerate(PINNED)])
def test_pinned_comparison_is_seen_by_its_case(unmutated, row):
    tag = row[6][len("pinned: "):]
    site = bnd.find(*row[:4])
    with tempfile.TemporaryDirectory() as tmp:
        got = bnd.digests(bnd.build(tmp, site), tag, limit=120.0)
    assert got is None or got[tag] != unmutated[tag], \
        f"{tag} no longer tells `{site['op']}` from `{bnd.SWAP[site['op']]}` in {row[0]}: `{row[1]}`"


def _through(tag):
    """[{field: array} after each step] of the oracle on a case, STEP_FIELDS plus status and npasses"""
    case = rc.CASES[tag]
    oc, ob, _, _ = rc.oracle_start(case, exp_mode=1)
    out = []
    for _ in rc.run_oracle(case, oc, ob):
        got = {n: rc.canonical(rc.field_of(ob, n, case.nz)) for n in rc.STEP_FIELDS}
        got["status"], got["npasses"] = ob["status"].astype(np.float64), ob["npasses"].astype(np.float64)
        out.append(got)
    return out


@pytest.mark.parametrize("tag", [t for t in rc.EDGE_CASES if rc.EDGE_TRIPLES[t]])
def test_neighbours_differ(built, tag):
    """In every triple the column at equality and at least one of its neighbours end with different outputs: else the
    case pins nothing."""
    steps = _through(tag)
    for lo, eq, hi in rc.EDGE_TRIPLES[tag]:
        differ = any(not np.array_equal(s[n][eq].view(np.int64), s[n][c].view(np.int64))
                     for s in steps for n in s for c in (lo, hi))
        assert differ, f"{tag}: the columns {lo}, {eq}, {hi} are alike in every output"


def test_the_cases_are_the_size_the_suite_can_afford(built):
    assert sorted(rc.EDGE_TRIPLES) == sorted(rc.EDGE_CASES)
    for tag in rc.EDGE_CASES:
        case = rc.CASES[tag]
        assert case.ncol <= 64 and 12 <= case.nz <= 69 and case.nsteps <= 6, tag
    assert {rc.CASES[t].nz for t in rc.EDGE_CASES} >= {12, 40, 60, 69}


def test_the_counter_cases_end_on_and_past_their_bounds(built):
    """ocnstep's integer counters: with itermax = 3 a column leaves the iteration after itermax + 1 passes of a try
    (no long-iteration flag) or after more (flagged); one column is accepted on its 10th try, reset_flag ==
    comp_iter_max and no failure, another fails on its 11th."""
    first = _through("edge_itermax3_nz40")[0]
    long_iter = (first["status"].astype(int) & orc.ST_LONG_ITER) != 0
    assert (~long_iter & (first["npasses"] == 4)).any() and (long_iter & (first["npasses"] > 4)).any()
    first = _through("edge_retry_count_thin")[0]
    st, n = first["status"].astype(int), first["npasses"]
    on, past = rc.RETRY_ON_THE_BOUND, rc.RETRY_PAST_THE_BOUND
    assert st[on] & orc.ST_RETRIED and not st[on] & orc.ST_FAILED and n[on] == 10 * 6
    assert st[past] & orc.ST_FAILED and n[past] == 11 * 6
