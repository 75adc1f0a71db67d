#!/usr/bin/env python3
"""What the operand checks of the `ops` wrappers cost on the host, per call: `eval_collect`, `ms_pool_append` and
`link_boxes` (the three with the most operands) of this tree against the same wrappers of a parent commit, both loaded
into ONE interpreter and timed in turns.  CPU only: the library is stubbed as in tests/golden/make_ops_calls.py (pinned
stream, `_lib.call` / `call_size` / `call_int` answer without a launch) and the operands are that file's tiny CPU tensors —
the checks read metadata only, so the sizes do not matter.

    python scripts/ops_check_cost.py [--parent HEAD~1] [--calls 20000] [--repeats 9] [--out profiles/ops_operand_checks.json]

A figure is the best of `repeats` runs of `calls` calls, in microseconds per call (the best run is the one the machine
disturbed least; the calls themselves do not vary).  The new figure is held against the parent's, never against itself:
allowed is the parent's cost plus one launch boundary (about 5 us per dependent launch) — every one of
these wrappers is followed by at least one launch, so a check that costs less than the launch hides behind the queue.
Exit status 1 when a wrapper is beyond that."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WRAPPERS = ("eval_collect", "ms_pool_append", "link_boxes")
LAUNCH_BOUNDARY_US = 5.0


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def best_us(fn, kw, calls, repeats):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(**kw)
        best = min(best, time.perf_counter() - t0)
    return best / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD~1", help="the commit whose ops.py is the baseline")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ops_operand_checks.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, ops
    sets = load("make_ops_calls", os.path.join(ROOT, "tests", "golden", "make_ops_calls.py")).operand_sets()
    rev = subprocess.check_output(["git", "rev-parse", args.parent], cwd=ROOT, text=True).strip()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ops_parent.py")
        with open(path, "w") as f:
            f.write(subprocess.check_output(["git", "show", rev + ":tensorflow_ocr_amd/ops.py"], cwd=ROOT, text=True))
        parent = load("tensorflow_ocr_amd.ops_parent", path)
    _lib.call = _lib.call_int = lambda name, *a: 0
    _lib.call_size = lambda name, *a: 256
    _lib.set_stream(ctypes.c_void_p(0))
    res = {"what": "host microseconds per call with the library stubbed, best of %d runs of %d calls, this tree against %s"
                   % (args.repeats, args.calls, rev[:12]),
           "parent": rev, "python": sys.version.split()[0], "launch_boundary_us": LAUNCH_BOUNDARY_US, "wrappers": {}}
    ok = True
    for name in WRAPPERS:
        kw = sets[name]
        for mod in (parent, ops):
            getattr(mod, name)(**kw)                                     # both take the set
        p, n = [], []
        for _ in range(3):                                               # in turns: a drifting clock touches both alike
            p.append(best_us(getattr(parent, name), kw, args.calls, args.repeats // 3 or 1))
            n.append(best_us(getattr(ops, name), kw, args.calls, args.repeats // 3 or 1))
        row = {"parent_us": round(min(p), 3), "new_us": round(min(n), 3), "allowed_us": round(min(p) + LAUNCH_BOUNDARY_US, 3)}
        row["within"] = row["new_us"] <= row["allowed_us"]
        ok = ok and row["within"]
        res["wrappers"][name] = row
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
