"""CPU: host side of the ICDAR-2015 evaluation protocol (csrc/eval_ic15.hip, include/ocr_eval_ic15.h, evaluate.py's
protocol='icdar15') — the C ABI's declarations and bindings, the --eval_protocol flag of the four scripts, and the exact
reference tests/ic15_ref.py pinned against answers worked out by hand (they stand as comments beside the cases there and
here), plus the condition under which tests/test_gpu_eval_ic15.py may ask the float64 kernels for the exact decisions.

The test_reference_* tests check tests/ic15_ref.py itself, so they pass with or without the feature; every other test
here needs it."""
import ctypes
import importlib
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import ic15_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocr_eval_ic15_workspace", "ocr_eval_ic15_match_batch"]
CASES = R.directed_cases()


# ------------------------------------------------------------------------------------------------ ABI, bindings
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_the_new_entries_and_keeps_the_abi_version():
    """the two entries stand in include/ocr_eval_ic15.h, which ocr_hip.h includes: one ABI, one version"""
    hip = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    assert re.search(r'^#include "ocr_eval_ic15\.h"$', hip, flags=re.M)
    assert _declared("ocr_eval_ic15.h") == set(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", hip)
    txt = open(os.path.join(ROOT, "include", "ocr_eval_ic15.h")).read()
    assert "BUILD-DEFINED" in txt and "reflex against reflex is outside the" in txt
    mk = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "Makefile")).read()
    assert "eval_ic15" in re.search(r"^NOFMA := (.*)$", mk, flags=re.M).group(1).split()
    assert "ocr_eval_ic15.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1)


def test_ops_and_tools_have_the_bindings():
    import torch
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import bboxes
    assert callable(getattr(ops, "eval_ic15_match_batch", None)) and callable(getattr(bboxes, "ic15_matching_batch", None))
    assert evaluate.PROTOCOLS == ("raster", "icdar15")
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    U8, I64 = torch.uint8, torch.int64
    with pytest.raises(ValueError, match="do not match"):
        ops.eval_ic15_match_batch(z(3, 16, 4, 2), z(3), z(3, 8, 4, 2), z(3), z(3, 8, dt=U8), 0.5, 0.5, z(3, 16), z(3, 9), z(4, dt=I64), None)
    with pytest.raises(ValueError, match="do not match"):
        ops.eval_ic15_match_batch(z(3, 16, 4, 2), z(3), z(3, 8, 4, 2), z(3), z(3, 8, dt=U8), 0.5, 0.5, z(3, 16), z(3, 8), z(4, dt=I64), None,
                                  inter=z(3, 16, 8, dt=torch.float64))
    with pytest.raises(ValueError, match="int32"):
        ops.eval_ic15_match_batch(z(3, 16, 4, 2), z(3), z(3, 8, 4, 2), z(3), z(3, 8), 0.5, 0.5, z(3, 16), z(3, 8), z(4, dt=I64), None)
    with pytest.raises(ValueError, match="contiguous"):
        ops.eval_ic15_match_batch(z(3, 16, 4, 2), z(3), z(3, 8, 4, 2), z(3), z(3, 8, dt=U8), 0.5, 0.5, z(16, 3).t(), z(3, 8), z(4, dt=I64), None)


def test_both_product_libraries_export_the_entries_and_check_their_arguments():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = ctypes.create_string_buffer(256)
    D, SZ = ctypes.c_double, ctypes.c_size_t
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        assert lib.ocr_abi_version() == 7
        ws = lib.ocr_eval_ic15_workspace
        ws.restype = ctypes.c_size_t
        # pair areas, polygon areas (f64), normalised polygons and kinds (9 int32 per polygon)
        assert ws(3, 16, 8) == 3 * (16 * 8 + 16 + 8) * 8 + 3 * (16 + 8) * 36
        assert ws(0, 16, 8) == 0 and ws(3, 0, 8) == 0 and ws(3, 16, -1) == 0
        assert ws(65535, 1024, 254) == 65535 * (1024 * 254 + 1024 + 254) * 8 + 65535 * (1024 + 254) * 36      # no 32-bit overflow
        # (no GPU is touched: every argument is checked before anything is launched)
        fn = lib.ocr_eval_ic15_match_batch
        a = lambda dets=buf, nd=buf, gts=buf, ng=buf, dc=buf, n=3, d=16, g=8, dm=buf, gm=buf, rec=buf, wsp=buf, wsb=1 << 20: (
            dets, nd, gts, ng, dc, n, d, g, D(0.5), D(0.5), dm, gm, None, rec, wsp, SZ(wsb), None)
        for kw in (dict(dets=None), dict(nd=None), dict(gts=None), dict(ng=None), dict(dc=None), dict(dm=None), dict(gm=None),
                   dict(rec=None), dict(wsp=None), dict(n=0), dict(d=0), dict(g=-1)):
            assert fn(*a(**kw)) == -1, kw
        assert fn(*a(d=1025)) == -2 and fn(*a(g=255)) == -2 and fn(*a(n=65536, wsb=1 << 40)) == -2
        assert fn(*a(wsb=ws(3, 16, 8) - 1)) == -4 and fn(*a(wsb=0)) == -4


# ------------------------------------------------------------------------------------------------ flags, evaluator
def test_eval_protocol_parses_in_the_four_scripts(capsys):
    sys.path.insert(0, ROOT)
    east, fast = importlib.import_module("test"), importlib.import_module("eval_pixellink_fast")
    mg, tp = importlib.import_module("multigpu_train"), importlib.import_module("train_pixellink")
    assert all(m.__file__.startswith(ROOT) for m in (east, fast, mg, tp))
    assert [m.parse([]).eval_protocol for m in (east, fast, mg, tp)] == ["raster"] * 4
    assert east.parse(["--geometry", "RBOX", "--gt_path", "/data/gt", "--eval_protocol", "icdar15"]).eval_protocol == "icdar15"
    assert fast.parse(["--eval_protocol", "icdar15"]).eval_protocol == "icdar15"
    rb = ["--net", "east", "--geometry", "RBOX", "--eval_data_path", "/data/val", "--eval_steps", "5"]
    assert mg.parse(rb + ["--eval_protocol", "icdar15"]).eval_protocol == "icdar15"
    assert tp.parse(["--eval_protocol", "icdar15"]).eval_protocol == "icdar15"
    for mod, bad, message in ((east, ["--eval_protocol", "icdar15"], "--eval_protocol needs --gt_path"),
                              (east, ["--geometry", "RBOX", "--gt_path", "/d", "--eval_protocol", "official"], "invalid choice"),
                              (mg, ["--net", "east", "--geometry", "RBOX", "--eval_protocol", "icdar15"],
                               "--eval_protocol needs --eval_data_path and --eval_steps"),
                              (mg, rb[:-2] + ["--eval_protocol", "icdar15"], "--eval_protocol needs --eval_data_path and --eval_steps"),
                              (fast, ["--eval_protocol", "polygon"], "invalid choice"),
                              (tp, ["--eval_protocol", "polygon"], "invalid choice")):
        with pytest.raises(SystemExit):
            mod.parse(bad)
        err = capsys.readouterr().err
        assert message in err, (bad, err)


def test_evaluator_rejects_other_protocols_and_drops_bow_ties(tmp_path):
    from tensorflow_ocr_amd import evaluate
    d = str(tmp_path)
    for bad in ("official", "ICDAR15", None, ""):
        with pytest.raises(ValueError, match="protocol must be"):
            evaluate.Evaluator(object(), None, d, protocol=bad)
        with pytest.raises(ValueError, match="protocol must be"):
            evaluate.LinkEvaluator(object(), None, d, protocol=bad)
    assert evaluate.quad_is_bow_tie(R.BOW_TIE) and evaluate.quad_is_bow_tie(R.BOW_TIE[::-1])
    assert not [q for q in R.CHEVRONS + [R.A, R.rect(5, 5, 15, 5)] if evaluate.quad_is_bow_tie(q)]
    line = dict(precision=0.5, recall=0.25, hmean=1 / 3, num_gt=8, num_det=4)
    assert evaluate.format_line(dict(line, protocol="icdar15")) == "precision 0.5000 recall 0.2500 hmean 0.3333 (gt 8 det 4) [icdar15]"
    assert evaluate.format_line(line) == "precision 0.5000 recall 0.2500 hmean 0.3333 (gt 8 det 4)"


# ------------------------------------------------------------------------------------------------ the reference, by hand
def test_reference_geometry_by_hand():
    # classification: either orientation, every rotation; the reflex vertex (10, 4) comes first
    for q in R.CHEVRONS:
        p, kind, area = R.normalise(q)
        assert kind == R.REFLEX and p[0] == (10, 4) and area == 80
        assert R._cross(p[0], p[1], p[2]) > 0 and R._cross(p[0], p[2], p[3]) > 0          # both triangles counter-clockwise
    assert R.normalise(R.A)[1:] == (R.CONVEX, Fr(400)) and R.normalise(R.A[::-1])[1:] == (R.CONVEX, Fr(400))
    assert R.normalise(R.BOW_TIE)[1] == R.BOWTIE and R.normalise(R.rect(5, 5, 15, 5))[1:] == (R.ZERO, Fr(0))
    assert R.normalise([[0, 0], [20, 0], [10, 12], [10, 12]])[1:] == (R.CONVEX, Fr(120))  # a doubled vertex is no turn
    # the chevron = triangle (0,0) (20,0) (10,12) [area 120] minus the notch (0,0) (20,0) (10,4) [area 40], against
    #   the left half's box: half of it by symmetry = 40
    #   the strip y <= 4: the big triangle's trapezoid (20 + 40/3) / 2 * 4 = 200/3, minus the whole notch = 80/3
    #   its bounding box: all of it = 80;  a box beside it: 0;  a box touching its tip (10, 12) from below: 0
    for q in R.CHEVRONS:
        assert R.intersection(R.rect(0, 0, 10, 12), q) == 40 and R.intersection(R.rect(0, 0, 20, 4), q) == Fr(80, 3)
        assert R.intersection(R.rect(0, 0, 20, 12), q) == 80 and R.intersection(R.rect(30, 0, 40, 12), q) == 0
        assert R.intersection(R.rect(0, 12, 20, 20), q) == 0
        assert R.intersection(q, R.rect(0, 0, 20, 4)) == Fr(80, 3)                         # a reflex detection, from its side
        assert R.intersection(q, q) == 0                                                   # reflex x reflex: outside the contract
    # two unit-slope diamonds |x| + |y| <= 2 and |x - 2| + |y| <= 2 meet in the square of diagonal 2: area 2
    assert R.intersection([[-2, 0], [0, -2], [2, 0], [0, 2]], [[0, 0], [2, -2], [4, 0], [2, 2]]) == 2
    assert R.intersection(R.BOW_TIE, R.rect(0, 0, 10, 10)) == 0 and R.intersection(R.rect(0, 0, 10, 10), R.BOW_TIE) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_gives_the_hand_worked_matches(name):
    images, expected = CASES[name]
    assert len(images) == R.N
    for i, (dets, gts, dontcare) in enumerate(images):
        assert len(dets) <= R.MAX_D and len(gts) <= R.MAX_G and len(dontcare) == len(gts)
        r = R.match_image(dets, gts, dontcare)
        assert (r["det_match"], r["gt_match"]) == (list(expected[i][0]), list(expected[i][1])), (name, i)


def test_reference_records_and_totals_by_hand():
    rec = lambda name, i: R.match_image(*CASES[name][0][i])["record"]
    # {care gt, matched, care det - matched, detections}
    assert rec("identical_and_order", 1) == [1, 1, 1, 2] and rec("identical_and_order", 2) == [2, 1, 0, 1]
    assert rec("half_iou_is_no_match", 0) == [1, 0, 1, 1]                   # IoU exactly 1/2: a miss and a false positive
    assert rec("dontcare_half_precision", 0) == [0, 0, 1, 1]                # precision exactly 1/2: still a care detection
    assert rec("dontcare_half_precision", 1) == [0, 0, 0, 1]                # one pixel column more: filtered out
    assert rec("bow_tie_and_zero_area", 0) == [0, 0, 1, 1]                  # the bow-tie is no care gt
    assert rec("bow_tie_and_zero_area", 1) == [2, 1, 1, 2]                  # a zero-area gt is a care gt nobody can match
    assert rec("empty_and_negative", 0) == [0, 0, 2, 2] and rec("empty_and_negative", 1) == [1, 0, 0, 0]
    assert rec("empty_and_negative", 2) == [2, 2, 0, 2]
    # the tie values themselves
    r = R.match_image(*CASES["half_iou_is_no_match"][0][0])
    assert r["iou"][0][0] == R.HALF and r["inter"][0][0] == 100
    r = R.match_image(*CASES["dontcare_half_precision"][0][0])
    assert r["prec"][0][0] == R.HALF
    assert R.match_image(*CASES["dontcare_half_precision"][0][1])["prec"][0][0] == Fr(11, 20)


def _values(r):
    return [v for row in r["iou"] for v in row] + [v for row in r["prec"] for v in row]


def test_every_fixture_decision_is_far_from_the_thresholds():
    """The condition of the GPU test: over every pair of every fixture the exact IoU and the exact area precision are
    further than 1e-6 from 1/2 (the float64 clipper is within 1e-12 of the exact area), except the containment ties of
    ic15_ref.TIE_IMAGES, where the value IS 1/2 or further than 1e-6 from it and float64 is exact: axis-aligned lattice
    rectangles only.  The seeds are ic15_ref.JITTER_SEEDS = (1, 2, 3), the first three tried."""
    eps, ties = Fr(1, 10 ** 6), 0
    for name, (images, _) in CASES.items():
        for i, image in enumerate(images):
            for v in _values(R.match_image(*image)):
                if (name, i) in R.TIE_IMAGES:
                    assert v == R.HALF or abs(v - R.HALF) > eps
                    ties += v == R.HALF
                else:
                    assert abs(v - R.HALF) > eps, (name, i, float(v))
            if (name, i) in R.TIE_IMAGES:
                for q in list(image[0]) + list(image[1]):
                    assert len(set(q[:, 0].tolist())) == 2 and len(set(q[:, 1].tolist())) == 2      # an axis-aligned rectangle
    assert ties >= 4
    assert R.JITTER_SEEDS == (1, 2, 3)
    for seed in R.JITTER_SEEDS:
        for i, image in enumerate(R.jittered_cases(seed)):
            assert min(abs(v - R.HALF) for v in _values(R.match_image(*image))) > eps, (seed, i)


def test_jittered_fixtures_spread_over_the_decisions():
    """detections are convex (the kernel's contract), every image holds a reflex ground truth, and the three seeds
    together hold matches, misses, false positives, don't-care detections and IoUs on both sides of 1/2"""
    seen = np.zeros(4, int)
    for seed in R.JITTER_SEEDS:
        images = R.jittered_cases(seed)
        assert [(len(d), len(g)) for d, g, _ in images] == [(R.MAX_D, R.MAX_G), (9, 5), (12, 3)]
        for dets, gts, dontcare in images:
            assert all(R.normalise(d)[1] == R.CONVEX for d in dets)
            assert R.normalise(gts[0])[1] == R.REFLEX and all(R.normalise(g)[1] == R.CONVEX for g in gts[1:])
            r = R.match_image(dets, gts, dontcare)
            ious = [float(v) for row in r["iou"] for v in row]
            seen += [r["record"][1], r["record"][2], sum(m == -2 for m in r["det_match"]), sum(0.2 < v < 0.5 for v in ious)]
            assert max(ious) > 0.6
    assert (seen > 0).all(), seen
