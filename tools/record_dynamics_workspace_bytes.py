#!/usr/bin/env python3
"""Records what the five workspace queries of the forward-dynamics family return (no GPU needed) into
tests/golden/dynamics_workspace_bytes.json, the values tests/test_dynamics_workspace_sizes.py pins.  The chains, chunk sizes, sample
counts and integrators are that test's.  Run it on the commit whose sizes are the contract -- the file in the tree was written by the
library as it stood BEFORE the C-ABI layer was split -- and never to make a failing test pass: a size that moved is a finding."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cabi as t                                                        # noqa: E402

if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    with open(dst, "w") as f:
        json.dump({name: t.measure(name) for name in t.CHUNKED}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)
