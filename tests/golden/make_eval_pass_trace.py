"""Records tests/golden/eval_pass_trace.json: what `evaluate.Evaluator` / `evaluate.LinkEvaluator` passes launch under the
recorder of tests/test_eval_pass_host.py (every case x protocol x sweep, the result dictionaries, and the error text of
every overflow case).  The test requires the same calls: run this on the commit whose evaluator is to be kept (with this
file and the test file copied onto it), BEFORE changing evaluate.py — never on the rewritten one.  It uses only the
constructors, `run()` and stubs on modules the rewrite leaves alone, so the same file runs on both sides.  No GPU needed.

    python tests/golden/make_eval_pass_trace.py [--parent HASH]

HASH is the commit the evaluator is taken from (default: `git rev-parse HEAD`)."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_eval_pass_host as T                      # noqa: E402


def write(parent, gold):
    with open(T.GOLDEN, "w") as f:
        f.write('{"parent": %s,\n "passes": {\n' % json.dumps(parent))
        rows = []
        for name, run in gold["passes"].items():
            tail = '"result": %s' % json.dumps(run["result"]) if "result" in run else '"raised": %s' % json.dumps(run["raised"])
            rows.append('  %s: {"trace": [\n%s],\n   %s}' % (json.dumps(name), ",\n".join("    " + json.dumps(e) for e in run["trace"]), tail))
        f.write(",\n".join(rows) + "\n },\n \"overflow\": {\n")
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in gold["overflow"].items()) + "\n }}\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    parent = argv[1] if argv[:1] == ["--parent"] else subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    with tempfile.TemporaryDirectory() as d:
        T.write_dir(d)
        gold = T.record_all(d)
    write(parent, gold)
    print("%d passes, %d overflow cases -> %s (%d bytes)" % (len(gold["passes"]), len(gold["overflow"]), T.GOLDEN, os.path.getsize(T.GOLDEN)))
