"""CPU: host side of the score-threshold sweep and AP (csrc/eval_curve.hip, include/ocr_eval_curve.h, evaluate.py's
`sweep`).  The prefix property the kernels rest on — counting over the states of ONE full matching gives, for every
threshold, what the matcher gives on the filtered list — is checked here against real re-runs of both matchers'
references (tests/sweep_ref.py) on seeded random images; then a hand-worked AP, the C ABI's declarations and bindings, the
--eval_sweep flag of the four scripts, and the formatting.

test_prefix_property_* and test_average_precision_by_hand check references against each other, so they pass with or
without the feature; every other test here needs it."""
import ctypes
import importlib
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import ic15_ref as R
import sweep_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocr_eval_curve_init", "ocr_eval_curve_batch", "ocr_eval_ic15_curve_batch", "ocr_eval_ap_workspace", "ocr_eval_ap"]
f32 = np.float32
SWEEP = [0.0, 0.25, 0.625, 0.75, 1.0, 1.5, 9.0, float("nan")]      # 0.25, 0.75, 1.0, 1.5 ARE scores of the random images


# ------------------------------------------------------------------------------------------------ the prefix property
@pytest.mark.parametrize("rule,seed,images", [("raster", 11, 150), ("icdar15", 12, 150)])
def test_prefix_property_counts_from_one_matching_equal_the_reruns(rule, seed, images):
    rng = np.random.default_rng(seed)
    seen = dict(no_gt=0, no_det=0, absent=0, contested=0, nan=0, rows_that_differ=0)
    for _ in range(images):
        dets, scores, gts, flags = image = S.random_image(rng, rule)
        assert S.is_collect_order(scores)
        state, care_gt = S.match_states(rule, dets, gts, flags)
        counted = S.counts_from_one_matching(state, scores, care_gt, SWEEP)
        rerun = S.rerun_rows(rule, image, SWEEP)
        assert counted == rerun, (rule, dets.tolist(), scores.tolist(), gts.tolist(), flags.tolist())
        seen["no_gt"] += len(gts) == 0 and len(dets) > 0
        seen["no_det"] += len(dets) == 0
        seen["absent"] += int((state == S.ABSENT).sum()) > 0
        seen["nan"] += bool(np.isnan(scores).any())
        seen["contested"] += int((state == S.CARE).sum()) > 0 and int((state == S.MATCHED).sum()) > 0
        seen["rows_that_differ"] += len({tuple(r) for r in counted}) >= 3
    print("sweep host %s: %s" % (rule, seen))
    assert all(v >= 3 for v in seen.values()), seen


def test_prefix_property_fails_without_the_order():
    """the property is one of score PREFIXES: with the scores of a matched detection and of the false positive behind
    it swapped (the list no longer in collect's order), counting and re-running part — which is why `unsorted` exists"""
    A = R.rect(10, 10, 30, 30)
    dets, gts, flags = np.array([A, A], np.int32), np.array([A], np.int32), np.zeros(1, bool)
    for rule in ("raster", "icdar15"):
        state, care_gt = S.match_states(rule, dets, gts, flags)
        assert state.tolist() == [S.MATCHED, S.CARE]
        good, bad = np.array([2.0, 1.0], f32), np.array([1.0, 2.0], f32)
        assert S.is_collect_order(good) and not S.is_collect_order(bad)
        assert S.counts_from_one_matching(state, good, care_gt, [1.5]) == S.rerun_rows(rule, (dets, good, gts, flags), [1.5]) == [[1, 1, 0, 1]]
        assert S.counts_from_one_matching(state, bad, care_gt, [1.5]) == [[1, 0, 1, 1]]
        assert S.rerun_rows(rule, (dets, bad, gts, flags), [1.5]) == [[1, 1, 0, 1]]
    assert S.is_collect_order(np.array([2, 2, 1, np.nan, np.nan], f32)) and not S.is_collect_order(np.array([2, np.nan, 1], f32))
    assert S.is_collect_order(np.zeros(0, f32))


# ------------------------------------------------------------------------------------------------ AP by hand
def test_average_precision_by_hand():
    M, C, A = S.MATCHED, S.CARE, S.ABSENT
    # image 0: scores 3 (matched), 2 (care), 2 (matched), 1 (absent);  image 1: scores 2 (matched), 2 (care), NaN (matched: outside AP)
    # order: (0,0) 3 M | (0,1) 2 C | (0,2) 2 M | (1,0) 2 M | (1,1) 2 C | the absent and the NaN slot are no slots
    # matched slots:  (0,0): 1/1   (0,2): 2/3   (1,0): 3/4   ->  AP = (1 + 2/3 + 3/4) / G, G = 4
    pool = [(np.array([M, C, M, A]), np.array([3, 2, 2, 1], f32)), (np.array([M, C, M]), np.array([2, 2, np.nan], f32))]
    ap, k = S.average_precision(pool, 4)
    assert (ap, k) == (Fr(29, 48), 3)
    # the images the other way round: (0,0) 2 M | (0,1) 2 C are now BEFORE the 2s of the other image, the 3 stays first
    # (1,0) 3 M: 1/1   (0,0) 2 M: 2/2   (1,2) 2 M: 3/5   ->  (1 + 1 + 3/5) / 4
    assert S.average_precision(pool[::-1], 4) == (Fr(13, 20), 3)
    assert S.average_precision(pool, 0) == (Fr(0), 3) and S.average_precision([], 5) == (Fr(0), 0)
    # the prefix counts of the pool rows
    assert S.pool_cum(pool[0][0], pool[0][1], 6).tolist() == [[1, 1], [2, 1], [3, 2], [3, 2], [3, 2], [3, 2]]
    assert S.pool_cum(pool[1][0], pool[1][1], 3).tolist() == [[1, 1], [2, 1], [2, 1]]


def test_gpu_fixture_holds_the_cases_and_is_far_from_the_matchers_thresholds():
    """what tests/test_gpu_eval_sweep.py relies on: every pair of its images is further than 1e-6 from the IC15 thresholds
    (the condition under which the float64 kernels decide as the exact rule), the scores are in collect's order, and the
    named edge cases are there"""
    images = S.gpu_images()
    eps = Fr(1, 10 ** 6)
    crowd = images["crowd"]
    assert [len(images[k][0]) for k in ("crowd", "no_gt", "no_det")] == [66, 12, 0]
    assert [len(images[k][2]) for k in ("crowd", "no_gt", "no_det")] == [5, 0, 3]
    assert len(S.THRESHOLDS) == S.T and max(len(im[0]) for im in images.values()) <= S.MAX_D > 64
    r = R.match_image(crowd[0][:16], crowd[2], crowd[3])                     # the 16 distinct detections hold every pair value
    assert min(abs(v - R.HALF) for row in r["iou"] + r["prec"] for v in row) > eps
    for dets, scores, gts, flags in images.values():
        assert S.is_collect_order(scores) and len(scores) == len(dets)
        assert dets.size == 0 or (dets.min() >= 0 and dets.max() < 400)
        assert gts.size == 0 or (gts.min() >= 0 and gts.max() < 400)
    finite = np.concatenate([im[1] for im in images.values()])
    finite = finite[~np.isnan(finite)]
    lo, nan, eq, hi, a, b = S.THRESHOLDS
    assert lo < finite.min() and hi > finite.max() and np.isnan(nan) and (finite == f32(eq)).any()
    assert finite.min() < b < a < finite.max() and not (finite == f32(a)).any() and not (finite == f32(b)).any()
    assert np.isnan(crowd[1][-1]) and not np.isnan(crowd[1][:-1]).any()
    assert (images["crowd"][1] == f32(1.5)).any() and (images["no_gt"][1] == f32(1.5)).any()          # a tie across two images
    for rule in ("raster", "icdar15"):
        state, care_gt = S.match_states(rule, crowd[0], crowd[2], crowd[3])
        assert care_gt >= 2 and (state == S.MATCHED).sum() >= 2 and (state == S.CARE).sum() >= 10
        assert (state == S.ABSENT).sum() >= 1                               # a don't-care detection
        assert (state[64:] != S.ABSENT).any()                               # something to count beyond the first wave
        tied = [set(state[crowd[1] == v].tolist()) for v in np.unique(crowd[1][:-1])]
        assert any({S.MATCHED, S.CARE} <= t for t in tied)                  # equal scores, one matched and one not, in one image
        at = crowd[1] == f32(2.75)                                          # ... and across two images: no_gt's 2.75s are unmatched
        assert (state[at] == S.MATCHED).any() and (images["no_gt"][1] == f32(2.75)).sum() == 2


# ------------------------------------------------------------------------------------------------ ABI, bindings
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_the_new_entries_and_keeps_the_abi_version():
    hip = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    assert re.search(r'^#include "ocr_eval_curve\.h"$', hip, flags=re.M) and re.search(r'^#include "ocr_eval_ic15\.h"$', hip, flags=re.M)
    assert _declared("ocr_eval_curve.h") == set(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", hip)
    txt = open(os.path.join(ROOT, "include", "ocr_eval_curve.h")).read()
    assert "BUILD-DEFINED" in txt and "a NaN-scored" in txt and "pinned by no test" in txt
    mk = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "Makefile")).read()
    assert "eval_curve" in re.search(r"^NOFMA := (.*)$", mk, flags=re.M).group(1).split()
    assert "ocr_eval_curve.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1)


def test_ops_and_tools_have_the_bindings():
    import torch
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import metrics
    for name in ("eval_curve_init", "eval_curve_batch", "eval_ic15_curve_batch", "eval_ap"):
        assert callable(getattr(ops, name, None)), name
    assert ops.EVAL_MAX_T == 64 and callable(metrics.DeviceCurve) and callable(evaluate.format_sweep)
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    U8, I64, F32 = torch.uint8, torch.int64, torch.float32
    ok = dict(det_score=z(3, 16, dt=F32), nd=z(3), ng=z(3), thresholds=z(6, dt=F32), curve=z(6, 4, dt=I64), unsorted=z(1))
    raster = lambda **kw: ops.eval_curve_batch(z(3, 16, dt=U8), z(3, 16, dt=U8), *[dict(ok, **kw)[k] for k in ("det_score", "nd", "ng")],
                                               z(3, 8, dt=U8), *[dict(ok, **kw)[k] for k in ("thresholds", "curve", "unsorted")],
                                               pool=kw.get("pool"))
    ic15 = lambda **kw: ops.eval_ic15_curve_batch(z(3, 16), z(3, 8), *[dict(ok, **kw)[k] for k in ok], pool=kw.get("pool"))
    for fn in (raster, ic15):
        with pytest.raises(ValueError, match="do not match"):
            fn(curve=z(5, 4, dt=I64))
        with pytest.raises(ValueError, match="do not match"):
            fn(det_score=z(3, 17, dt=F32))
        with pytest.raises(ValueError, match="do not match"):
            fn(pool=(z(3, 16, dt=F32), z(3, 16, dt=torch.int32), z(3)))
        with pytest.raises(ValueError, match="f32"):
            fn(thresholds=z(6, dt=torch.float64))
        with pytest.raises(ValueError, match="contiguous"):
            fn(det_score=z(16, 3, dt=F32).t())
    with pytest.raises(ValueError, match="do not match"):
        ops.eval_ap(z(3, 16, dt=F32), z(3, 16, 2), z(2), z(4, dt=I64), z(1, dt=torch.float64), None)
    with pytest.raises(ValueError, match="float64"):
        ops.eval_ap(z(3, 16, dt=F32), z(3, 16, 2), z(3), z(4, dt=I64), z(1, dt=F32), None)


def test_both_product_libraries_export_the_entries_and_check_their_arguments():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = ctypes.create_string_buffer(256)
    SZ = ctypes.c_size_t
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        assert lib.ocr_abi_version() == 7
        ws = lib.ocr_eval_ap_workspace
        ws.restype = ctypes.c_size_t
        assert ws(3, 70) == 8 and ws(3, 86) == 16 and ws(500, 1024) == 2000 * 8        # one f64 partial per 256 slots
        assert ws(0, 16) == 0 and ws(3, 0) == 0 and ws(-1, 16) == 0
        assert ws(65535, 1024) == 65535 * 4 * 8
        # (no GPU is touched: every argument is checked before anything is launched)
        ra = lambda tp=buf, fp=buf, sc=buf, nd=buf, ng=buf, ign=buf, thr=buf, n=3, d=70, g=5, T=6, cur=buf, uns=buf, ps=None, pc=None, pn=None: (
            tp, fp, sc, nd, ng, ign, thr, n, d, g, T, cur, uns, ps, pc, pn, None)
        ia = lambda dm=buf, gm=buf, sc=buf, nd=buf, ng=buf, thr=buf, n=3, d=70, g=5, T=6, cur=buf, uns=buf, ps=None, pc=None, pn=None: (
            dm, gm, sc, nd, ng, thr, n, d, g, T, cur, uns, ps, pc, pn, None)
        for fn, a, required in ((lib.ocr_eval_curve_batch, ra, ("tp", "fp", "sc", "nd", "ng", "ign", "thr", "cur", "uns")),
                                (lib.ocr_eval_ic15_curve_batch, ia, ("dm", "gm", "sc", "nd", "ng", "thr", "cur", "uns"))):
            for k in required:
                assert fn(*a(**{k: None})) == -1, k
            assert fn(*a(n=0)) == -1 and fn(*a(d=0)) == -1 and fn(*a(g=-1)) == -1
            assert fn(*a(ps=buf)) == -1 and fn(*a(ps=buf, pc=buf)) == -1 and fn(*a(pn=buf)) == -1     # a pool given in part
            assert fn(*a(d=1025)) == -2 and fn(*a(g=255)) == -2 and fn(*a(n=65536)) == -2
            assert fn(*a(T=0)) == -2 and fn(*a(T=65)) == -2 and fn(*a(T=-3)) == -2
        ap = lib.ocr_eval_ap
        aa = lambda ps=buf, pc=buf, pn=buf, n=3, d=70, rec=buf, out=buf, wsp=buf, wsb=64: (ps, pc, pn, n, d, rec, out, wsp, SZ(wsb), None)
        for k in ("ps", "pc", "pn", "rec", "out", "wsp"):
            assert ap(*aa(**{k: None})) == -1, k
        assert ap(*aa(n=0)) == -1 and ap(*aa(d=-2)) == -1
        assert ap(*aa(d=1025)) == -2 and ap(*aa(n=65536, wsb=1 << 40)) == -2
        assert ap(*aa(wsb=7)) == -4 and ap(*aa(wsb=0)) == -4
        init = lib.ocr_eval_curve_init
        assert init(None, 6, buf, None, None) == -1 and init(buf, 6, None, None, None) == -1
        assert init(buf, 0, buf, None, None) == -2 and init(buf, 65, buf, None, None) == -2


# ------------------------------------------------------------------------------------------------ flags, formatting
def test_eval_sweep_parses_in_the_four_scripts(capsys):
    from tensorflow_ocr_amd import evaluate
    sys.path.insert(0, ROOT)
    east, fast = importlib.import_module("test"), importlib.import_module("eval_pixellink_fast")
    mg, tp = importlib.import_module("multigpu_train"), importlib.import_module("train_pixellink")
    assert all(m.__file__.startswith(ROOT) for m in (east, fast, mg, tp))
    assert [m.parse([]).eval_sweep for m in (east, fast, mg, tp)] == [None] * 4
    rb = ["--net", "east", "--geometry", "RBOX", "--eval_data_path", "/data/val", "--eval_steps", "5"]
    lk = ["--eval_data_path", "/data/val", "--eval_steps", "5", "--using_moving_average"]
    want = [0.0, 0.25, 0.5, 0.75, 1.0]
    assert east.parse(["--geometry", "RBOX", "--gt_path", "/data/gt", "--eval_sweep", "0:1:5"]).eval_sweep == want
    assert fast.parse(["--eval_sweep", "0:1:5"]).eval_sweep == want
    assert mg.parse(rb + ["--eval_sweep", "0:1:5"]).eval_sweep == want
    assert tp.parse(lk + ["--eval_sweep", "0:1:5"]).eval_sweep == want
    assert fast.parse(["--eval_sweep", "0.9, 0.5,2"]).eval_sweep == [0.9, 0.5, 2.0]          # a comma list, in the order given
    assert evaluate.parse_sweep("0.5") == [0.5] and evaluate.parse_sweep("3:3:1") == [3.0]
    assert evaluate.parse_sweep("2:40:64")[0] == 2.0 and evaluate.parse_sweep("2:40:64")[-1] == 40.0
    assert len(evaluate.parse_sweep("0:1:64")) == 64
    for text in ("0:1", "0:1:0", "0:1:1", "0:1:65", "", "a,b", "0:1:2:3", ",".join(["1"] * 65)):
        with pytest.raises(ValueError):
            evaluate.parse_sweep(text)
    for mod, bad, message in ((east, ["--eval_sweep", "0:1:5"], "--eval_sweep needs --gt_path"),
                              (east, ["--geometry", "RBOX", "--gt_path", "/d", "--eval_sweep", "0:1"], "LO:HI:N"),
                              (mg, ["--net", "east", "--geometry", "RBOX", "--eval_sweep", "0:1:5"],
                               "--eval_sweep needs --eval_data_path and --eval_steps"),
                              (mg, rb[:-2] + ["--eval_sweep", "0:1:5"], "--eval_sweep needs --eval_data_path and --eval_steps"),
                              (tp, ["--eval_sweep", "0:1:5"], "--eval_sweep needs --eval_data_path and --eval_steps"),
                              (fast, ["--eval_sweep", "0:1:65"], "1 to 64 thresholds")):
        with pytest.raises(SystemExit):
            mod.parse(bad)
        err = capsys.readouterr().err
        assert message in err, (bad, err)


def test_evaluators_check_the_sweep_and_format_line_is_unchanged(tmp_path):
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import metrics
    np.save(os.path.join(str(tmp_path), "img_1.npy"), np.zeros((64, 64, 3), np.uint8))
    open(os.path.join(str(tmp_path), "gt_img_1.txt"), "w").write("1,1,9,1,9,6,1,6,text\r\n")
    for bad in ([], [0.5] * 65):
        with pytest.raises(ValueError, match="1 to 64 thresholds"):
            evaluate.Evaluator(object(), None, str(tmp_path), sweep=bad)
        with pytest.raises(ValueError, match="1 to 64 thresholds"):
            evaluate.LinkEvaluator(object(), None, str(tmp_path), sweep=bad)
    line =dict(precision=0.5, recall=0.25, hmean=1 / 3, num_gt=8, num_det=4)
    assert evaluate.format_line(line) == "precision 0.5000 recall 0.2500 hmean 0.3333 (gt 8 det 4)"
    rows = [[8, 2, 2, 4], [8, 2, 0, 2], [8, 0, 0, 0], [8, 2, 0, 3]]
    sweep, best = evaluate.sweep_rows([0.1, 0.5, 0.9, 0.4], rows)
    assert [r["threshold"] for r in sweep] == [0.1, 0.5, 0.9, 0.4] and best is sweep[1]           # ties go to the lowest index
    assert (sweep[0]["precision"], sweep[0]["recall"]) == metrics.precision_recall(8, 2, 2) == (0.5, 0.25)
    assert sweep[0]["hmean"] == metrics.fmean(0.5, 0.25) and sweep[2]["hmean"] == 0.0 and sweep[1]["hmean"] == 0.4
    assert sorted(sweep[0]) == sorted(["threshold", "precision", "recall", "hmean", "tp", "fp", "num_det"])
    with_sweep = dict(line, sweep=sweep, best=best, ap=0.21875)
    assert evaluate.format_line(with_sweep) == evaluate.format_line(line)                        # the line does not change
    text = evaluate.format_sweep(with_sweep).splitlines()
    assert len(text) == 5 and text[1].endswith(" *") and not text[0].endswith("*")
    assert text[1].split() == ["score", ">=", "0.5", "precision", "1.0000", "recall", "0.2500", "hmean", "0.4000", "(tp", "2", "fp", "0",
                               "det", "2)", "*"]
    assert text[4].strip() == "AP 0.2188, best hmean 0.4000 at score >= 0.5"
