#!/usr/bin/env python3
"""Which comparisons of the oracle's physics do the suite's inputs ever evaluate with both sides equal?

Branch coverage (tools/oracle_coverage.py) cannot tell `<` from `<=`.  The column kernel states every comparison of
the step a second time and is asserted equal to the oracle (oracle/mckpp_oracle.c) bit for bit, so an oracle comparison
whose swap for its neighbour no input can see is a kernel comparison no test checks at equality.  This script swaps one
`<`/`<=`/`>`/`>=` at a time (`<` <-> `<=`, `>` <-> `>=`) in the functions a model step, init_ocean, vmix_only or the
kppmix + tridiagonal pass can execute (orc_cpsw ... check_profile, without the orc_conv_* probes, the *_batch probe
wrappers, the lookup-table builder and col_new / col_free), builds each mutant into a temporary directory with

    gcc -O1 -fPIC -std=gnu11 -ffp-contract=off -fno-fast-math

(no sanitizer, at most 16 builds and runs in flight), selects it through MCKPP_ORACLE_LIBRARY and drives it in a child
process with

  before   the three phases of tools/oracle_coverage.py (the generators' inputs and every case of
           tests/ref_step_cases.py under 2000 columns that is no edge case), the same cases under solver mode 1, and
           the vmix_only / vmix_batch entry points on one bathymetry case
  after    the same plus the edge cases (rc.EDGE_CASES), each under solver modes 0 and 1 and through vmix_only

One digest per run: every STEP_FIELDS array (canonicalised as rc.canonical does), `status` and `npasses` over all
columns after init_ocean and after every step.  A mutant whose digests all equal the unmutated build's survives; one
that crashes, aborts or runs longer than max(120 s, 10 x the unmutated run) is killed.

    python tools/oracle_boundaries.py > profiles/coverage/oracle_boundaries.md

A site is (function, text of its source line, which such line of the function, which operator of the line): the record
survives edits elsewhere; the line numbers in the table are for the reader.  Needs gcc.  The mutation run is not a
test; tests/test_boundaries_cpu.py checks the record's site list and re-kills every pinned site with its case."""
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "oracle", "mckpp_oracle.c")
RECORD = os.path.join(ROOT, "profiles", "coverage", "oracle_boundaries.md")
BUILD = ["gcc", "-O1", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math"]
JOBS = min(16, os.cpu_count() or 1)
FIRST, LAST = "orc_cpsw", "check_profile"
SKIP = re.compile(r"^(orc_conv_\w+|\w+_batch|orc_lookup_mode|orc_lookup|col_new|col_free)$")
SWAP = {"<": "<=", "<=": "<", ">": ">=", ">=": ">"}
OPERATOR = re.compile(r"(?<![<>=!-])(<=|>=|<|>)(?![<>=])")
VMIX_CASE = "seafloor_nz40"          # the bathymetry case the vmix_only / vmix_batch entry points are driven on


# ----------------------------------------------------------------------------------------------------------------
# sites
# ----------------------------------------------------------------------------------------------------------------
def _without_comments(src):
    """the source with every comment, string and character literal blanked out, offsets kept"""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r"/\*.*?\*/|//[^\n]*|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", blank, src, flags=re.S)


def functions(src):
    """[(name, first line, last line)] of the function definitions of a C source, 1-based and inclusive"""
    code = _without_comments(src)
    out, depth, head, line, start, name = [], 0, 0, 1, 0, None
    for i, ch in enumerate(code):
        if ch == "\n":
            line += 1
        elif ch == "{":
            if depth == 0:
                header = "\n".join(l for l in code[head:i].split("\n") if not l.lstrip().startswith("#"))
                m = re.search(r"(\w+)\s*\(", header)
                name = m.group(1) if m and "=" not in header[:m.start()] and "typedef" not in header else None
                start = line - header[m.start():].count("\n") if name else line
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth == 0:
                if name:
                    out.append((name, start, line))
                head = i + 1
        elif ch == ";" and depth == 0:
            head = i + 1
    return out


def sites(src=None):
    """[{function, text, nth, occ, line, col, op}] in source order.  `text`: the stripped source line; `nth`: which
    line with that text inside the function (0-based); `occ`: which comparison operator of the line (0-based)"""
    if src is None:
        with open(SOURCE) as f:
            src = f.read()
    raw, code = src.split("\n"), _without_comments(src).split("\n")
    funcs = functions(src)
    names = [f[0] for f in funcs]
    lo, hi = names.index(FIRST), names.index(LAST)
    out = []
    for name, a, b in funcs[lo:hi + 1]:
        if SKIP.match(name):
            continue
        seen = {}
        for ln in range(a, b + 1):
            if code[ln - 1].lstrip().startswith("#"):
                continue
            ops = list(OPERATOR.finditer(code[ln - 1]))
            if not ops:
                continue
            text = raw[ln - 1].strip()
            nth = seen.get(text, 0)
            seen[text] = nth + 1
            for occ, m in enumerate(ops):
                out.append(dict(function=name, text=text, nth=nth, occ=occ, line=ln, col=m.start(), op=m.group(1)))
    return out


def key(site):
    return (site["function"], site["text"], site["nth"], site["occ"])


def find(function, text, nth=0, occ=0, src=None):
    """the site of the current source with this identity (KeyError when the source no longer has it)"""
    for s in sites(src):
        if key(s) == (function, text, nth, occ):
            return s
    raise KeyError((function, text, nth, occ))


def mutate(src, site):
    lines = src.split("\n")
    l, c, op = lines[site["line"] - 1], site["col"], site["op"]
    assert l[c:c + len(op)] == op
    lines[site["line"] - 1] = l[:c] + SWAP[op] + l[c + len(op):]
    return "\n".join(lines)


def build(tmp, site=None):
    """liboracle.so of the oracle (site None) or of one mutant in the directory `tmp`; returns its path"""
    with open(SOURCE) as f:
        src = f.read()
    with open(os.path.join(ROOT, "oracle", "mckpp_oracle.h")) as f, open(os.path.join(tmp, "mckpp_oracle.h"), "w") as g:
        g.write(f.read())
    with open(os.path.join(tmp, "mckpp_oracle.c"), "w") as g:
        g.write(mutate(src, site) if site else src)
    lib = os.path.join(tmp, "liboracle.so")
    subprocess.check_call(BUILD + ["-shared", "-o", lib, "mckpp_oracle.c", "-lm"], cwd=tmp)
    return lib


# ----------------------------------------------------------------------------------------------------------------
# the drive (child process; MCKPP_ORACLE_LIBRARY is already set)
# ----------------------------------------------------------------------------------------------------------------
def drive(what):
    """prints {run: digest}: `what` is "all" (the run "before" and one run per edge case) or one case's tag"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import numpy as np

    import oracle_coverage
    import ref_step_cases as rc
    from oracle import orc

    state = {"h": None}

    def take(ob):
        h = state["h"]
        for name in rc.STEP_FIELDS:
            h.update(rc.canonical(rc.field_of(ob, name, ob.nz)).tobytes())
        h.update(np.ascontiguousarray(ob["status"]).tobytes())
        h.update(np.ascontiguousarray(ob["npasses"]).tobytes())

    def wrap(fn):
        def run(const, batch, *a, **k):
            fn(const, batch, *a, **k)
            take(batch)
        return run
    for fn in ("init_ocean", "physics_driver", "vmix_only", "vmix_batch"):
        setattr(orc, fn, wrap(getattr(orc, fn)))

    def case_runs(tag, modes, vmix):
        case = rc.CASES[tag]
        for mode in modes:
            oc, ob, _, _ = rc.oracle_start(case, exp_mode=1, solver_mode=mode)
            for _ in rc.run_oracle(case, oc, ob):
                pass
            if vmix and mode == 0:
                orc.vmix_only(oc, ob.copy(), case.nsteps + 1)
                orc.vmix_batch(oc, ob.copy(), case.nsteps + 1)

    edges = list(getattr(rc, "EDGE_CASES", []))
    out = {}
    if what == "all":
        state["h"] = hashlib.sha256()
        held = dict(rc.CASES)
        for t in edges:                       # the phases of oracle_coverage.py, as the parent commit has them
            del rc.CASES[t]
        for phase in oracle_coverage.PHASES:
            oracle_coverage.drive(phase)
        for tag in [t for t in rc.CASES if rc.CASES[t].ncol < 2000]:
            case_runs(tag, (1,), tag == VMIX_CASE)
        rc.CASES.update(held)
        out["before"] = state["h"].hexdigest()
    for tag in (edges if what in ("all", "edges") else [what]):
        state["h"] = hashlib.sha256()
        case_runs(tag, (0, 1), True)
        out[tag] = state["h"].hexdigest()
    print(json.dumps(out))


def digests(lib, what="all", limit=None):
    """{run: digest} of a build, or None when the child crashed, aborted or ran past `limit` seconds"""
    env = dict(os.environ, MCKPP_ORACLE_LIBRARY=lib, OMP_NUM_THREADS="1")
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--drive", what], env=env, timeout=limit,
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        return None
    if p.returncode != 0:
        return None
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


def _one(args):
    site, limit = args
    with tempfile.TemporaryDirectory() as tmp:
        return digests(build(tmp, site), limit=limit)


# ----------------------------------------------------------------------------------------------------------------
# the record
# ----------------------------------------------------------------------------------------------------------------
def parse_record(path=RECORD):
    """[(function, text, nth, occ, survived before, survived after, class)] of the committed table"""
    rows = []
    for line in open(path):
        m = re.match(r"\| (\w+) \| (\d+)\.(\d+) @\d+ \| `(.*)` \| (\S+) \| (\S+) \| (.*) \|$", line.rstrip("\n"))
        if m:
            rows.append((m.group(1), m.group(4).replace("\\|", "|"), int(m.group(2)), int(m.group(3)), m.group(5),
                         m.group(6), m.group(7)))
    return rows


def classify(cls, site):
    """(class, reason) of a surviving site from tools/oracle_boundaries_classes.py"""
    if key(site) in cls.CLASSES:
        return cls.CLASSES[key(site)]
    if (site["function"], site["text"]) in cls.LAST_TRIP:
        return cls.UNREAD, cls.LAST_TRIP[(site["function"], site["text"])]
    return "UNCLASSIFIED", ""


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--drive":
        return drive(sys.argv[2])
    sys.path[:0] = [os.path.join(ROOT, "tools")]
    import oracle_boundaries_classes as cls

    all_sites = sites()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        base = digests(build(tmp))
        took = time.time() - t0
    assert base, "the unmutated oracle does not run"
    limit = max(120.0, 10.0 * took)
    with concurrent.futures.ThreadPoolExecutor(JOBS) as pool:
        got = list(pool.map(_one, [(s, limit) for s in all_sites]))
    edges = [t for t in base if t != "before"]
    rows, left, n_before, n_after, by_class = [], [], 0, 0, {}
    for s, d in zip(all_sites, got):
        before = d is not None and d["before"] == base["before"]
        killers = [] if d is None else [t for t in edges if d[t] != base[t]]
        after = before and not killers
        n_before += before
        n_after += after
        if not before:
            c = "-"
        elif killers:
            c = f"pinned: {killers[0]}"
        else:
            c = classify(cls, s)[0]
            left.append(s)
        if before:
            by_class[c.split(":")[0]] = by_class.get(c.split(":")[0], 0) + 1
        text = s["text"].replace("|", "\\|")
        rows.append(f"| {s['function']} | {s['nth']}.{s['occ']} @{s['line']} | `{text}` | "
                    f"{'survived' if before else 'killed'} | {'survived' if after else 'killed'} | {c} |")
    print("# Comparisons of the oracle's physics that no input evaluates with both sides equal\n")
    print("Made by `tools/oracle_boundaries.py`: every `<`, `<=`, `>`, `>=` of oracle/mckpp_oracle.c from orc_cpsw to")
    print("check_profile (without the orc_conv_* probes, the *_batch wrappers, the lookup-table builder, col_new and")
    print("col_free) swapped for its neighbour, one at a time; built with `" + " ".join(BUILD) + "`.  A mutant")
    print("*survives* when every STEP_FIELDS array, `status` and `npasses` come out bit-identical (after rc.canonical)")
    print("after init_ocean and after every step of every input; it is *killed* when anything differs, when it crashes")
    print("or aborts, or when it runs past max(120 s, 10 x the unmutated run).  *Before*: the inputs of")
    print("tools/oracle_coverage.py's three phases, the cases of tests/ref_step_cases.py under 2000 columns that are no")
    print(f"edge cases again under solver mode 1, and vmix_only / vmix_batch on {VMIX_CASE}.  *After*: with the edge")
    print("cases (rc.EDGE_CASES) under solver modes 0 and 1 and through vmix_only / vmix_batch.  A site is the function,")
    print("`n.m` (the n-th line of the function with this text, the m-th comparison on it) and, for the reader, the")
    print("line number.\n")
    classes = ", ".join(f"{v} {k}" for k, v in sorted(by_class.items()) if k != "pinned")
    print(f"Sites: {len(all_sites)}.  Survived before: {n_before}; after: {n_after}.  Of the {n_before}, "
          f"{by_class.get('pinned', 0)} are pinned by an edge case; the {n_after} still surviving: {classes}.\n")
    print("| function | site | source | before | after | class |\n|---|---|---|---|---|---|")
    print("\n".join(rows))
    print(cls.NOTES.rstrip("\n"))
    for s in left:
        c, why = classify(cls, s)
        print(f"- `{s['function']}` {s['nth']}.{s['occ']} @{s['line']}, `{s['op']}` in `{s['text'].split('/*')[0].strip()}`: "
              f"**{c}**.  {why}")


if __name__ == "__main__":
    main()
