"""Records tests/golden/train_tail_trace.json: under "tail" what the loss seeds, the optimiser steps, `summary_factor` and
the optimiser state round trip do under the recorder of tests/test_train_tail_host.py, under "cli" what the four drivers'
`parse` return and say (tests/test_cli_host.py).  The tests require the same: run this on the commit whose training tail and
drivers are to be kept (with this file and the two test files copied onto it), BEFORE changing them — never on the rewritten
ones.  It uses only names both sides have.  No GPU needed.

    python tests/golden/make_train_tail_trace.py [--parent HASH]

HASH is the commit the code is taken from (default: `git rev-parse HEAD`)."""
import io
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_cli_host as C                            # noqa: E402
import test_train_tail_host as T                     # noqa: E402


class _Capture:
    """pytest's capsys, as far as test_cli_host.error_text uses it"""

    def readouterr(self):
        err, sys.stderr = sys.stderr.getvalue(), io.StringIO()
        return types.SimpleNamespace(err=err)


def section(d, indent):
    pad = " " * indent
    return "{\n" + ",\n".join("%s%s: %s" % (pad, json.dumps(k), json.dumps(v)) for k, v in d.items()) + "}"


if __name__ == "__main__":
    argv = sys.argv[1:]
    parent = argv[1] if argv[:1] == ["--parent"] else subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    tail = T.record_all()
    real, sys.stderr = sys.stderr, io.StringIO()
    try:
        cli = C.record_all(_Capture())
    finally:
        sys.stderr = real
    with open(T.GOLDEN, "w") as f:
        f.write('{"parent": %s,\n "tail": {\n' % json.dumps(parent))
        f.write(",\n".join('  %s: %s' % (json.dumps(k), section(v, 3)) for k, v in tail.items()))
        f.write("\n },\n \"cli\": {\n")
        f.write(",\n".join('  %s: %s' % (json.dumps(k), section(v, 3)) for k, v in cli.items()))
        f.write("\n }}\n")
    print("%d tail cases, %d drivers -> %s (%d bytes)" % (sum(len(v) for v in tail.values()), len(cli), T.GOLDEN,
                                                         os.path.getsize(T.GOLDEN)))
