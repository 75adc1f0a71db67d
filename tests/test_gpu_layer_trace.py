"""GPU: what the Python layer modules launch, build by build, against tests/golden/layer_trace.json.

tensorflow_ocr_amd/layers.py, resnet_layers.py and head_layers.py decide which C-ABI entries a step calls, in which order
and on which tensors.  tests/golden/make_layer_trace.py recorded that for a table of small builds — the three training
nets, their forward-only builds, the f32 precision, the two big nets with each of seven switches off, and four builds
for the head paths those do not reach — as the address-free list of one eager step's calls under `_lib.Recorder`, plus
the loss bits of two training steps and a CRC-32 of the parameters after them.  Every build is recorded again here, in a fresh interpreter (the switches are read at import), and must give
the SAME list (the golden keeps its SHA-256, and a CRC-32 per entry to name the first one that moved) and the SAME
bits: no tolerance.  A replayed step issues the recorded list, so an equal list is an equal step.  When a change is
MEANT to alter the launches: record the lists as text on both commits (`make_layer_trace.py --text DIR`), read their
`diff`, and commit the new golden."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("make_layer_trace", os.path.join(ROOT, "tests", "golden", "make_layer_trace.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

with open(T.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_golden_covers_every_build():
    assert sorted(GOLDEN["builds"]) == sorted(T.BUILDS)


@pytest.mark.parametrize("name", list(T.BUILDS))
def test_build_launches_what_the_golden_recorded(device, name):
    want = GOLDEN["builds"][name]
    got = T.run_build(name, GOLDEN["batch"], GOLDEN["size"], storage=GOLDEN["storage"])
    now, was = "".join(T.digest(got["trace"])["entries"]), "".join(want["entries"])
    for i, t in enumerate(got["trace"]):
        assert now[8 * i:8 * i + 8] == was[8 * i:8 * i + 8], "%s: entry %d is not the recorded one (%s); now: %s" % (
            name, i, was[8 * i:8 * i + 8] or "the recorded list ends before it", t)
    assert len(now) == len(was), "%s: %d entries, %d recorded" % (name, len(now) // 8, len(was) // 8)
    assert T.digest(got["trace"])["sha256"] == want["sha256"], name
    if want.get("numbers") is not None:
        print("%s: loss bits %s, parameters' CRC-32 %s, record step %.1f ms" % (name, got["loss"], got["flat_crc32"], got["record_ms"]))
        assert {"loss": got["loss"], "flat_crc32": got["flat_crc32"]} == want["numbers"], name
