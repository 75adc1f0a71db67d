"""Records tests/golden/train_tail_plans.json: the recorded step plan (C entries with their tags, no pointers) of the eight
cases of tests/test_gpu_train_step.py::test_every_tail_mode_records_the_parents_plan_and_replays_the_eager_step.  Needs the
GPU.  Run it on the commit whose plans are to be kept, with the test file copied onto it — never on the rewritten code.
Equal plans are stored once.

    python tests/golden/make_train_tail_plans.py [--parent HASH] [--out FILE]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_train_step as T                      # noqa: E402


def record(device="cuda:0"):
    plans, cases = [], {}
    for which, mode in T.TAIL_CASES:
        names = json.loads(json.dumps(T.run_tail_case(device, which, mode)[0]))
        if names not in plans:
            plans.append(names)
        cases["%s %s" % (which, mode)] = plans.index(names)
    return plans, cases


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    parent = opt("--parent", None) or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = opt("--out", T.TAIL_PLANS)
    plans, cases = record()
    again, cases2 = record()                            # a plan that differs between two runs cannot be pinned whole
    with open(out, "w") as f:
        f.write('{"parent": %s,\n "stable": %s,\n "cases": %s,\n "plans": [\n' % (
            json.dumps(parent), json.dumps(plans == again and cases == cases2), json.dumps(cases)))
        f.write(",\n".join("  [" + ",\n   ".join(json.dumps(e) for e in p) + "]" for p in plans) + "\n ]}\n")
    print("%d cases, %d distinct plans, stable %s -> %s (%d bytes)" % (len(cases), len(plans), plans == again, out,
                                                                      os.path.getsize(out)))
