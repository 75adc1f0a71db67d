"""CPU: host side of the device evaluation (csrc/eval_match.hip, tensorflow_ocr_amd/evaluate.py) — the C ABI's declarations
and bindings, the flags of test.py and multigpu_train.py, the float64 / NumPy restatement of ocr_eval_collect's rule that
tests/test_gpu_eval_chain.py holds the kernel to (checked here against answers worked out by hand), and the directed
matching cases of tests/test_gpu_eval_match.py, pinned here against oracle/evalboxes.py: every case is reachable by the
reference rule alone, and the answers the GPU test expects are worked out by hand below.

The test_collect_restatement_* and test_directed_cases_* tests check this file's helpers and the oracle, so they pass with
or without the feature; every other test here needs it."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

from oracle import evalboxes as OE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32 = np.float32, np.float64, np.int32

NEW_SYMBOLS = ["ocr_eval_collect", "ocr_eval_match_workspace", "ocr_eval_match_batch", "ocr_eval_record_init"]
BINDINGS = ["eval_collect", "eval_match_batch", "eval_record_init"]
MAX_D, MAX_G = 16, 8          # the shapes of the GPU matching test
COORD_LIMIT = 2.0 ** 22


# ------------------------------------------------------------------------------------------------ collect restatement
def collect_ref(merged, keep, n_keep, passed, ratio, max_d):
    """ocr_eval_collect's rule for ONE image in float64 / NumPy: merged [max_k,9] f32, keep [max_k] int, n_keep, passed
    [max_k] bool or None, ratio (ratio_w, ratio_h) f32 -> (dets int32 [m,4,2], score f32 [m], nd_total), m =
    min(nd_total, max_d).  A vertex is trunc(f32(x / ratio)): the float64 quotient of two f32 numbers rounded to f32 IS
    the IEEE f32 quotient (53 >= 2 * 24 + 2 bits); non-finite -> 0, |.| >= 2^22 clamped.  Order: descending score, ties
    in keep order, NaN last = np.argsort(-score, kind="stable")."""
    merged = np.asarray(merged, f32)
    max_k = merged.shape[0]
    rows = [int(keep[j]) for j in range(min(max(int(n_keep), 0), max_k))
            if (passed is None or passed[j]) and 0 <= int(keep[j]) < max_k]
    score = merged[rows, 8] if rows else np.zeros((0,), f32)
    order = np.argsort(-score.astype(f64), kind="stable")[:max_d]
    div = np.array([ratio[0], ratio[1]] * 4, f32).astype(f64)
    dets = np.zeros((len(order), 8), i32)
    with np.errstate(all="ignore"):
        for o, k in enumerate(order):
            q = (merged[rows[k], :8].astype(f64) / div).astype(f32).astype(f64)
            q = np.where(np.isfinite(q), np.clip(np.trunc(q), -COORD_LIMIT, COORD_LIMIT), 0.0)
            dets[o] = q.astype(i32)
    return dets.reshape(-1, 4, 2), score[order].astype(f32), len(rows)


def test_collect_restatement_divides_truncates_and_clamps():
    merged = np.zeros((4, 9), f32)
    merged[0] = [3, 3, -3, -3, 7.5, 7.49, 1e9, -1e9, 0.5]
    merged[1] = [np.nan, np.inf, -np.inf, 1, 2, 3, 4, 5, 0.25]
    dets, score, total = collect_ref(merged, [0, 1], 2, None, (f32(0.75), f32(1.5)), MAX_D)
    assert total == 2 and score.tolist() == [0.5, 0.25]
    # 3 / 0.75 = 4; 3 / 1.5 = 2; -3 / 0.75 = -4; -3 / 1.5 = -2; 7.5 / 0.75 = 10; 7.49 / 1.5 = 4.99.. -> 4 (towards zero)
    assert dets[0].reshape(-1).tolist() == [4, 2, -4, -2, 10, 4, 2 ** 22, -2 ** 22]
    # non-finite -> 0; 1 / 1.5 -> 0; 2 / 0.75 = 2.67 -> 2; 3 / 1.5 = 2; 4 / 0.75 = 5.33 -> 5; 5 / 1.5 = 3.33 -> 3
    assert dets[1].reshape(-1).tolist() == [0, 0, 0, 0, 2, 2, 5, 3]
    # the f32 quotient, not the f64 one: 0.3f / 0.1f is exactly 3 in f32 (truncates to 3), 2.9999999.. in float64
    m = np.zeros((1, 9), f32)
    m[0, 0] = f32(0.3)
    assert f64(f32(0.3)) / f64(f32(0.1)) != 3.0 and f32(0.3) / f32(0.1) == f32(3.0)
    assert collect_ref(m, [0], 1, None, (f32(0.1), f32(1)), 4)[0][0, 0, 0] == 3


def test_collect_restatement_order_is_stable_descending_with_mask_and_overflow():
    merged = np.zeros((8, 9), f32)
    merged[:, 8] = [1.0, 2.0, 2.0, np.nan, 3.0, 2.0, 0.5, 9.0]
    merged[:, 0] = np.arange(8) * 10                       # x1 names the row
    keep = [6, 2, 1, 3, 4, 5, 0, 7]                        # 7 lies beyond n_keep = 7
    passed = np.array([1, 1, 1, 1, 1, 0, 1, 1], bool)      # keep position 5 (row 5) is filtered out
    dets, score, total = collect_ref(merged, keep, 7, passed, (f32(1), f32(1)), MAX_D)
    assert total == 6
    # 3.0 (row 4); the 2.0 rows in KEEP order (2 then 1); 1.0 (row 0); 0.5 (row 6); NaN last (row 3)
    assert dets[:, 0, 0].tolist() == [40, 20, 10, 0, 60, 30]
    assert np.isnan(score[-1]) and score[:-1].tolist() == [3.0, 2.0, 2.0, 1.0, 0.5]
    dets, score, total = collect_ref(merged, keep, 7, passed, (f32(1), f32(1)), 3)
    assert total == 6 and dets[:, 0, 0].tolist() == [40, 20, 10]           # overflow: the first max_d of the order
    assert collect_ref(merged, keep, 0, None, (f32(1), f32(1)), 3)[2] == 0
    assert collect_ref(merged, [9, -1, 2], 3, None, (f32(1), f32(1)), 3)[2] == 1       # indices outside the list are dropped


# ------------------------------------------------------------------------------------------------ directed matching cases
def rect(x0, y0, x1, y1):
    """axis-aligned quad; its fillPoly raster is (x1 - x0 + 1) (y1 - y0 + 1) pixels"""
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def random_quads(rng, k, lo=10, hi=54):
    """perturbed rotated rectangles inside 64 x 64, int32 [k,4,2]"""
    out = np.zeros((k, 4, 2), i32)
    for j in range(k):
        cx, cy = rng.uniform(lo, hi, 2)
        hw, hh, a = rng.uniform(3, 12), rng.uniform(2, 8), rng.uniform(-0.7, 0.7)
        c, s = np.cos(a), np.sin(a)
        local = np.array([[-hw, -hh], [hw, -hh], [hw, hh], [-hw, hh]])
        pts = np.stack([cx + local[:, 0] * c - local[:, 1] * s, cy + local[:, 0] * s + local[:, 1] * c], axis=1)
        out[j] = np.clip(np.rint(pts + rng.uniform(-1.5, 1.5, (4, 2))), 0, 63).astype(i32)
    return out


def _image(dets, gts, ignored):
    return (np.asarray(dets, i32).reshape(-1, 4, 2), np.asarray(gts, i32).reshape(-1, 4, 2), np.asarray(ignored, bool).reshape(-1))


A, B, FAR = rect(10, 10, 29, 29), rect(40, 40, 59, 59), rect(2, 50, 8, 60)
NEG_DET, NEG_GT = rect(-30, -30, -10, -10), rect(-50, -50, -35, -35)


def directed_cases():
    """name -> (threshold, [3 images of (dets [k,4,2], gts [g,4,2], ignored [g])], expected [(tp list, fp list)] or None).
    `expected` is worked out by hand from tool/bboxes.py:171-240; None = random, the oracle alone says."""
    cases = {}
    cases["duplicate_ignored_identical"] = (0.5, [
        _image([A, A], [A, B], [0, 0]),                    # the second copy finds A matched: a false positive
        _image([A, B], [A, B], [1, 0]),                    # the best match of det 0 is ignored: neither; det 1 matches B
        _image([A, A], [A, A], [0, 0]),                    # two identical ground truths: argmax is index 0 both times
    ], [([1, 0], [0, 1]), ([0, 1], [0, 0]), ([1, 0], [0, 1])])
    cases["first_index_wins"] = (0.5, [
        _image([A], [A, A], [1, 0]),                       # index 0 wins the tie and is ignored: neither
        _image([A], [A, A], [0, 1]),                       # index 0 wins and counts
        _image([FAR], [A, B], [0, 0]),                     # IoU 0 with both: argmax 0, no match: fp
    ], [([0], [0]), ([1], [0]), ([0], [1])])
    # IoU exactly at the threshold is no match (strict >): 100 / 400, 100 / 200, 150 / 200 pixels; one pixel row more is
    for name, thr, det_at, det_over, gt in (("at_threshold_025", 0.25, rect(0, 0, 9, 9), rect(0, 0, 9, 10), rect(0, 0, 19, 19)),
                                            ("at_threshold_05", 0.5, rect(0, 0, 9, 9), rect(0, 0, 9, 10), rect(0, 0, 9, 19)),
                                            ("at_threshold_075", 0.75, rect(0, 0, 9, 14), rect(0, 0, 9, 15), rect(0, 0, 9, 19))):
        cases[name] = (thr, [_image([det_at], [gt], [0]), _image([det_over], [gt], [0]), _image([det_at, det_over], [gt], [0])],
                       [([0], [1]), ([1], [0]), ([0, 1], [1, 0])])
    # the detection and the second ground truth lie wholly at negative coordinates: both rasters are empty, 0 / 0 = NaN,
    # and np.argmax takes the NaN: index 1, no match
    cases["nan_pair"] = (0.5, [
        _image([NEG_DET], [A, NEG_GT], [0, 0]),            # fp through the NaN ground truth
        _image([NEG_DET], [A, NEG_GT], [0, 1]),            # the NaN ground truth is ignored: neither
        _image([NEG_DET, A], [A, NEG_GT, NEG_GT], [0, 0, 0]),   # the FIRST NaN wins (index 1); A still matches afterwards
    ], [([0], [1]), ([0], [0]), ([0, 1], [1, 0])])
    rng = np.random.default_rng(2024)
    g0, g1, g2 = random_quads(rng, MAX_G), random_quads(rng, 5), random_quads(rng, 3)

    def near(gts, k):          # detections scattered around the ground truths, plus strays
        idx = rng.integers(0, len(gts), k)
        d = gts[idx] + rng.integers(-2, 3, (k, 4, 2))
        d[k // 2:] = random_quads(rng, k - k // 2)
        return np.clip(d, 0, 63).astype(i32)
    cases["random"] = (0.5, [_image(near(g0, 12), g0, rng.integers(0, 2, MAX_G)), _image(near(g1, 7), g1, [0, 0, 1, 0, 0]),
                             _image(near(g2, 9), g2, [0, 0, 0])], None)
    cases["random_025"] = (0.25, cases["random"][1], None)
    cases["random_075"] = (0.75, cases["random"][1], None)
    # nd = max_d, nd = 0, ng = 0 (build-defined: every detection is a false positive)
    cases["full_empty_no_gt"] = (0.5, [_image(near(g0, MAX_D), g0, [0] * MAX_G), _image(np.zeros((0, 4, 2)), g1, [0, 1, 0, 0, 0]),
                                       _image(near(g2, 4), np.zeros((0, 4, 2)), [])], None)
    return cases


def oracle_image(dets, gts, ignored, thr):
    """(ground truths not ignored, tp bool [k], fp bool [k]) of one image by oracle/evalboxes.py; no ground truth at all:
    the build-defined rule (all false positives); no detection: nothing to match."""
    k = len(dets)
    n_g = int(np.count_nonzero(~ignored))
    if k == 0:
        return n_g, np.zeros(0, bool), np.zeros(0, bool)
    if len(gts) == 0:
        return 0, np.zeros(k, bool), np.ones(k, bool)
    return OE.bboxes_matching(dets.reshape(k, 8), gts[:, :, 0], gts[:, :, 1], ignored, thr)


@pytest.mark.parametrize("name", sorted(directed_cases()))
def test_directed_cases_are_what_the_reference_rule_gives(name):
    thr, images, expected = directed_cases()[name]
    assert len(images) == 3 and f64(f32(thr)) == thr                        # the f32 and f64 comparisons agree
    for i, (dets, gts, ignored) in enumerate(images):
        assert len(dets) <= MAX_D and len(gts) <= MAX_G and len(ignored) == len(gts)
        assert max([int(dets.max()) if dets.size else 0, int(gts.max()) if gts.size else 0]) < 64
        n_g, tp, fp = oracle_image(dets, gts, ignored, thr)
        assert n_g == int((~ignored).sum()) and not (tp & fp).any()
        if expected is not None:
            assert (tp.astype(int).tolist(), fp.astype(int).tolist()) == expected[i], (name, i)


def test_directed_cases_reach_the_edges_they_are_named_for():
    c = directed_cases()
    # the exact-threshold pairs: the oracle's f32 Jaccard IS the threshold
    for name in ("at_threshold_025", "at_threshold_05", "at_threshold_075"):
        thr, images, _ = c[name]
        dets, gts, _ = images[0]
        jac = OE.np_bboxes_jaccard(dets[0].reshape(8), gts[:, :, 0], gts[:, :, 1])
        assert jac.dtype == f32 and jac[0] == f32(thr)
        dets, gts, _ = images[1]
        assert OE.np_bboxes_jaccard(dets[0].reshape(8), gts[:, :, 0], gts[:, :, 1])[0] > f32(thr)
    # the NaN pair: 0 for the positive ground truth, NaN for the negative one, and argmax takes the NaN
    dets, gts, _ = c["nan_pair"][1][2]
    jac = OE.np_bboxes_jaccard(dets[0].reshape(8), gts[:, :, 0], gts[:, :, 1])
    assert jac[0] == 0 and np.isnan(jac[1]) and np.isnan(jac[2]) and int(np.argmax(jac)) == 1
    # the random images hold true positives, false positives and ignored matches, and the shapes named
    kinds = np.zeros(3, int)
    for name in ("random", "full_empty_no_gt"):
        thr, images, _ = c[name]
        for dets, gts, ignored in images:
            _, tp, fp = oracle_image(dets, gts, ignored, thr)
            kinds += [int(tp.sum()), int(fp.sum()), int((~tp & ~fp).sum())]
    assert (kinds > 0).all(), kinds
    shapes = [(len(d), len(g)) for d, g, _ in c["full_empty_no_gt"][1]]
    assert shapes[0][0] == MAX_D and shapes[1][0] == 0 and shapes[2][1] == 0 and shapes[2][0] > 0


# ------------------------------------------------------------------------------------------------ ABI, bindings
def test_header_declares_the_new_entries_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert sorted(s for s in declared if s.startswith("ocr_eval_")) == sorted(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert "BUILD-DEFINED: ng[i] = 0" in txt                                # the rule for an image without ground truths is stated


def test_ops_and_tools_have_the_bindings():
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import bboxes, metrics, rbox
    assert not [b for b in BINDINGS if not callable(getattr(ops, b, None))]
    assert (ops.EVAL_MAX_D, ops.EVAL_MAX_G) == (1024, 254)
    assert callable(bboxes.bboxes_matching_batch) and callable(rbox.detect_device) and callable(metrics.DeviceTpFp)
    assert callable(evaluate.Evaluator) and callable(evaluate.TrainEval)


def test_both_product_libraries_export_the_entries_and_check_their_arguments():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = ctypes.create_string_buffer(256)
    F, SZ = ctypes.c_float, ctypes.c_size_t
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        ws = lib.ocr_eval_match_workspace
        ws.restype = ctypes.c_size_t
        assert ws(3, 16, 8) == 3 * 16 * 8 * 2 * 4 and ws(0, 16, 8) == 0 and ws(3, 0, 8) == 0 and ws(3, 16, -1) == 0
        assert ws(65535, 1024, 254) == 65535 * 1024 * 254 * 8                    # no 32-bit overflow in the query
        # (no GPU is touched: every argument is checked before anything is launched)
        col, mat = lib.ocr_eval_collect, lib.ocr_eval_match_batch
        assert col(None, buf, buf, None, buf, 3, 40, 16, buf, buf, buf, buf, None) == -1
        assert col(buf, buf, buf, None, None, 3, 40, 16, buf, buf, buf, buf, None) == -1
        assert col(buf, buf, buf, None, buf, 0, 40, 16, buf, buf, buf, buf, None) == -1
        assert col(buf, buf, buf, None, buf, 3, 40, 0, buf, buf, buf, buf, None) == -1
        assert col(buf, buf, buf, None, buf, 3, 40, 1025, buf, buf, buf, buf, None) == -2
        assert col(buf, buf, buf, None, buf, 65536, 40, 16, buf, buf, buf, buf, None) == -2
        args = lambda n=3, d=16, g=8, mh=74, mw=74, wsb=1 << 20, rec=buf: (
            buf, buf, buf, buf, buf, n, d, g, F(0.5), mh, mw, buf, buf, rec, buf, SZ(wsb), None)
        assert mat(*args(rec=None)) == -1 and mat(*args(n=0)) == -1 and mat(*args(mh=0)) == -1 and mat(*args(g=0)) == -1
        assert mat(*args(d=1025)) == -2 and mat(*args(g=255)) == -2 and mat(*args(n=65536, wsb=1 << 40)) == -2
        assert mat(*args(mw=32769)) == -2
        assert mat(*args(wsb=3 * 16 * 8 * 8 - 1)) == -4
        assert lib.ocr_eval_record_init(None, None) == -1


# ------------------------------------------------------------------------------------------------ flags
def test_test_py_parses_gt_path_only_with_rbox(capsys):
    sys.path.insert(0, ROOT)
    east = importlib.import_module("test")
    assert east.__file__.startswith(ROOT)
    assert east.parse([]).gt_path is None
    r = east.parse(["--geometry", "RBOX", "--gt_path", "/data/gt"])
    assert (r.geometry, r.gt_path) == ("RBOX", "/data/gt")
    with pytest.raises(SystemExit):
        east.parse(["--gt_path", "/data/gt"])                               # the default geometry is link
    assert "--gt_path needs --geometry RBOX" in capsys.readouterr().err


def test_multigpu_train_parses_the_eval_flags(capsys):
    sys.path.insert(0, ROOT)
    T = importlib.import_module("multigpu_train")
    d = T.parse([])
    assert (d.eval_data_path, d.eval_steps, d.eval_max_images, d.eval_weights) == (None, 0, None, "ema")
    rb = ["--net", "east", "--geometry", "RBOX"]
    f = T.parse(rb + ["--eval_data_path", "/data/val", "--eval_steps", "500", "--eval_max_images", "100", "--eval_weights", "raw"])
    assert (f.eval_data_path, f.eval_steps, f.eval_max_images, f.eval_weights) == ("/data/val", 500, 100, "raw")
    assert T.make_train_eval(d, None, None) is None                         # off by default: nothing is built
    for bad in (rb + ["--eval_steps", "5"],                                 # no directory
                ["--eval_data_path", "/data/val", "--eval_steps", "5"],     # not RBOX
                ["--net", "east", "--eval_data_path", "/data/val", "--eval_steps", "5"],
                rb + ["--eval_data_path", "/data/val", "--eval_steps", "-1"],
                rb + ["--eval_data_path", "/data/val", "--eval_steps", "5", "--eval_weights", "best"],
                rb + ["--eval_data_path", "/data/val", "--eval_steps", "5", "--eval_max_images", "0"]):
        with pytest.raises(SystemExit):
            T.parse(bad)
    assert "--eval_steps needs --eval_data_path" in capsys.readouterr().err


def test_resize_rule_is_test_pys_rule():
    from tensorflow_ocr_amd.evaluate import resize_rule
    assert resize_rule(64, 64) == (64, 64) and resize_rule(64, 96) == (64, 96)
    assert resize_rule(720, 1280) == (672, 1280)                            # 720 // 32 - 1 = 21 rows of 32
    assert resize_rule(100, 70) == (64, 32)
    assert resize_rule(6000, 3000) == (2944, 1440)                          # ratio 0.5: 3000 -> 92 * 32, 1500 -> 45 * 32
    with pytest.raises(ValueError):
        resize_rule(40, 40)


def test_ground_truth_files_parse_with_ignore_tags(tmp_path):
    from tensorflow_ocr_amd import evaluate
    d = str(tmp_path)
    np.save(os.path.join(d, "img_1.npy"), np.zeros((64, 64, 3), np.uint8))
    np.save(os.path.join(d, "img_2.npy"), np.zeros((64, 64, 3), np.uint8))                  # no gt file: skipped
    with open(os.path.join(d, "gt_img_1.txt"), "w") as f:
        f.write("10.9,10,29,10,29,29,10,29,word\r\n40,40,59,40,59,59,40,59,###\r\n")
    assert [os.path.basename(p) for p in evaluate.list_images(d)] == ["img_1.npy", "img_2.npy"]
    polys, ign = evaluate.load_ground_truth(os.path.join(d, "img_1.npy"))
    assert polys.dtype == i32 and polys.tolist() == [rect(10, 10, 29, 29), rect(40, 40, 59, 59)] and ign.tolist() == [False, True]
    assert evaluate.load_ground_truth(os.path.join(d, "img_2.npy")) is None
    assert evaluate.format_line(dict(precision=0.5, recall=0.25, hmean=1 / 3, num_gt=8, num_det=4)) == \
        "precision 0.5000 recall 0.2500 hmean 0.3333 (gt 8 det 4)"
