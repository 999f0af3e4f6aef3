"""CPU test (no GPU): test modules are leaves.  Helpers that more than one test module needs live in the support modules tests/_*.py
(tests/README.md); no module under tests/ imports a test module, and a support module neither marks itself `gpu` nor needs torch to be
imported, so that the CPU tests can use it."""
import ast
import os

TESTS = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = {"_alias_multi_gpu", "_world2_gram", "_world2_tsqr"}   # run as subprocesses by the multi-GPU tests, not imported


def _trees():
    out = {}
    for f in sorted(os.listdir(TESTS)):
        if f.endswith(".py"):
            with open(os.path.join(TESTS, f)) as src:
                out[f[:-3]] = ast.parse(src.read(), f)
    return out


def _imported(node):
    if isinstance(node, ast.Import):
        return [a.name.split(".")[0] for a in node.names]
    if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
        return [node.module.split(".")[0]]
    return []


def test_no_module_imports_a_test_module():
    trees = _trees()
    assert len(trees) > 70
    for name, tree in trees.items():
        for node in ast.walk(tree):   # function-level imports too
            bad = [m for m in _imported(node) if m.startswith("test_")]
            assert not bad, "%s.py line %d imports %s: move what it needs into a support module" % (name, node.lineno, bad)


def test_support_modules_are_plain_modules_that_load_without_torch():
    support = {name: tree for name, tree in _trees().items() if name.startswith("_") and name not in SCRIPTS}
    assert {"_chains", "_arrays", "_cabi", "_fuzz"} <= set(support)
    for name, tree in support.items():
        for node in tree.body:   # module level only: helpers take torch as an argument or import it inside the function
            assert "torch" not in _imported(node), "%s.py imports torch at module level (line %d)" % (name, node.lineno)
            targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AnnAssign, ast.AugAssign)) else []
            assert not any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in targets), "%s.py sets pytestmark" % name
