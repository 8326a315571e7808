"""The suite's support code is stated once (tests/harness.py, tests/common.py and the *_cases modules): a helper that
two test files define identically is a copy that a correction then has to reach twice."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_helper_is_defined_twice():
    """Every top-level function of tests/*.py that is no test, compared by the ast.dump of its definition (decorators
    included, positions and comments not): none occurs in two files."""
    seen = {}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and not node.name.startswith("test_"):
                seen.setdefault(ast.dump(node), []).append((node.name, os.path.basename(path)))
    twice = sorted((where[0][0], sorted({f for _, f in where})) for where in seen.values()
                   if len({f for _, f in where}) > 1)
    assert not twice, "defined identically in more than one file (state it once, in tests/harness.py):\n" + "\n".join(
        f"  {name}: {', '.join(files)}" for name, files in twice)
