"""CPU: host side of the link-geometry evaluation (csrc/link_boxes.hip, evaluate.LinkEvaluator) — the NumPy restatements
`component_scores_ref` / `link_boxes_ref` that tests/test_gpu_link_boxes.py and tests/test_gpu_link_eval_chain.py hold the
kernels to (checked here against answers worked out by hand), the C ABI's declarations, exports and argument checks, the
flags of train_pixellink.py and eval_pixellink_fast.py, and the evaluator's batching and scales on a fake forward.

Every test here needs the feature: the module imports the device entries it restates."""
import ctypes
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tensorflow_ocr_amd.tool.pixellink_fn import _box_points, _rotated_rect, detect_device, link_boxes_device  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32 = np.float32, np.float64, np.int32

NEW_SYMBOLS = ["ocr_component_scores", "ocr_component_scores_workspace", "ocr_link_boxes"]
BINDINGS = ["component_scores", "link_boxes"]


# ------------------------------------------------------------------------------------------------ restatements
def component_scores_ref(labels, pixel_score, ncomp, max_comps):
    """ocr_component_scores in NumPy / Python integers: labels int [n,h,w], pixel_score f32 [n,h,w], ncomp int [n] ->
    f32 [n,max_comps].  q = rint(clamp(s, 0, 1) * 2^24) per pixel (NaN -> 0; the product is exact: a power of two), exact
    integer sum and count per id, mean = f32(f64(sum) / f64(count) / 2^24); an id without pixels and every row at or
    beyond min(ncomp, max_comps) are 0."""
    labels = np.asarray(labels)
    s = np.asarray(pixel_score, f32)
    c = np.clip(np.where(np.isnan(s), f32(0), s), f32(0), f32(1)).astype(f64)
    q = np.rint(c * 16777216.0).astype(np.uint64)
    n = labels.shape[0]
    out = np.zeros((n, max_comps), f32)
    for b in range(n):
        for L in range(1, min(max(int(ncomp[b]), 0), max_comps) + 1):
            sel = labels[b] == L
            cnt = int(sel.sum())
            if cnt:
                total = sum(int(v) for v in q[b][sel])
                out[b, L - 1] = f32(f64(total) / f64(cnt) / 16777216.0)
    return out


def link_boxes_ref(hull_n, hull_head, calipers, comp_score, ncomp, min_side=0.0, min_area=0.0):
    """ocr_link_boxes on the host, built on pixellink_fn._rotated_rect / _box_points (the host half of
    min_area_rect_boxes): hull_n int [n,C], hull_head int [n,C,4], calipers f32 [n,C,6], comp_score f32 [n,C], ncomp int [n]
    -> (merged f32 [n,C,9], keep int32 [n,C], n_keep int32 [n], passed uint8 [n,C], total int32 [n])."""
    hull_n = np.asarray(hull_n)
    n, C = hull_n.shape
    merged = np.zeros((n, C, 9), f32)
    keep = np.tile(np.arange(C, dtype=i32), (n, 1))
    passed = np.zeros((n, C), np.uint8)
    n_keep = np.minimum(np.maximum(np.asarray(ncomp, i32), 0), C).astype(i32)
    for b in range(n):
        for c in range(int(n_keep[b])):
            nh = int(hull_n[b, c])
            rect = _rotated_rect(nh, hull_head[b, c], calipers[b, c])
            merged[b, c, :8] = _box_points(rect).astype(np.int64).reshape(8).astype(f32)        # np.int0: toward zero
            merged[b, c, 8] = comp_score[b, c]
            w, h = f32(rect[2]), f32(rect[3])
            passed[b, c] = nh > 0 and min(w, h) >= f32(min_side) and f32(w * h) >= f32(min_area)
    return merged, keep, n_keep, passed, np.asarray(ncomp, i32).copy()


def test_component_scores_restatement_by_hand():
    labels = np.zeros((2, 2, 4), i32)
    score = np.zeros((2, 2, 4), f32)
    labels[0] = [[1, 1, 0, 2], [3, 3, 3, 9]]                               # id 9 is beyond ncomp: no row of its own
    score[0] = [[0.5, 0.25, 0.9, np.nan], [1.5, -0.5, 1.0, 0.75]]
    labels[1] = [[1, 1, 1, 1], [1, 1, 1, 1]]
    score[1] = 1.0
    out = component_scores_ref(labels, score, [4, 1], 3)
    # id 1: (0.5 + 0.25) / 2; id 2: its only pixel is NaN -> 0; id 3: 1.5 -> 1, -0.5 -> 0, 1: 2 / 3; id 4 <= ncomp has no row (max_comps 3)
    assert out[0].tolist() == [0.375, 0.0, float(f32(2.0 / 3.0))]
    assert out[1].tolist() == [1.0, 0.0, 0.0]                              # rows at or beyond ncomp are 0
    assert component_scores_ref(labels, score, [0, 0], 3).tolist() == [[0.0] * 3] * 2
    # the quantum is 2^-24: two scores that differ below it give one integer, 2^-24 apart two
    a, b = f32(0.5), np.nextafter(f32(0.5), f32(1))                        # 0.5 + 2^-24
    assert float(b) - float(a) == 2.0 ** -24
    lab = np.ones((1, 1, 1), i32)
    ra = component_scores_ref(lab, np.full((1, 1, 1), a), [1], 1)[0, 0]
    rb = component_scores_ref(lab, np.full((1, 1, 1), b), [1], 1)[0, 0]
    below = f32(0.125) + f32(2.0 ** -26)                                   # one ulp above 0.125, a quarter of the quantum
    rc = component_scores_ref(lab, np.full((1, 1, 1), below), [1], 1)[0, 0]
    assert ra == a and rb == b and below != f32(0.125) and rc == f32(0.125)
    # an id with no pixel scores 0; a sum a 32-bit accumulator cannot hold comes out exact
    big = component_scores_ref(np.ones((1, 20, 300), i32), np.ones((1, 20, 300), f32), [2], 2)
    assert big.tolist() == [[1.0, 0.0]] and 6000 * 2 ** 24 > 2 ** 32


def test_link_boxes_restatement_by_hand():
    hull_n = np.array([[4, 2, 1, 0, 4]], i32)
    head = np.zeros((1, 5, 4), i32)
    cal = np.zeros((1, 5, 6), f32)
    cal[0, 0] = [2, 3, 8, 0, 0, 4]               # corner (2, 3), edges (8, 0) and (0, 4): the rectangle [2, 10] x [3, 7]
    head[0, 1] = [0, 0, 10, 0]                   # a horizontal segment
    head[0, 2] = [7, 9, 0, 0]                    # a point
    cal[0, 4] = [0, 0, 3, 0, 0, 3]               # beyond ncomp
    score = np.array([[0.9, 0.8, 0.7, 0.6, 0.5]], f32)
    merged, keep, n_keep, passed, total = link_boxes_ref(hull_n, head, cal, score, [4])
    assert merged[0, 0].tolist() == [2, 7, 2, 3, 10, 3, 10, 7, float(f32(0.9))]
    assert merged[0, 1].tolist() == [0, 0, 0, 0, 10, 0, 10, 0, float(f32(0.8))]
    assert merged[0, 2].tolist() == [7, 9, 7, 9, 7, 9, 7, 9, float(f32(0.7))]
    assert merged[0, 3].tolist() == [0] * 8 + [float(f32(0.6))] and (merged[0, 4] == 0).all()
    assert keep.tolist() == [[0, 1, 2, 3, 4]] and n_keep.tolist() == [4] and total.tolist() == [4]
    assert passed.tolist() == [[1, 1, 1, 0, 0]]                            # hull_n = 0 never passes; thresholds 0 filter nothing
    assert link_boxes_ref(hull_n, head, cal, score, [4], min_side=4.0)[3].tolist() == [[1, 0, 0, 0, 0]]
    assert link_boxes_ref(hull_n, head, cal, score, [4], min_side=4.5)[3].tolist() == [[0, 0, 0, 0, 0]]
    assert link_boxes_ref(hull_n, head, cal, score, [4], min_area=32.0)[3].tolist() == [[1, 0, 0, 0, 0]]
    assert link_boxes_ref(hull_n, head, cal, score, [4], min_area=32.5)[3].tolist() == [[0, 0, 0, 0, 0]]
    m2, _, nk2, p2, t2 = link_boxes_ref(hull_n, head, cal, score, [9])     # ncomp beyond the list
    assert nk2.tolist() == [5] and t2.tolist() == [9] and p2.tolist() == [[1, 1, 1, 0, 1]]
    assert m2[0, 4, :8].tolist() == [0, 3, 0, 0, 3, 0, 3, 3]
    # a rotated rectangle: negative coordinates truncate toward zero, not down
    cal[0, 0] = [-0.5, 2.5, 3, 3, -2, 2]
    m3 = link_boxes_ref(hull_n, head, cal, score, [1])[0]
    # centre (0, 5), 45 degrees: corners (-2.5, 4.5), (-0.5, 2.5), (2.5, 5.5), (0.5, 7.5) up to f32 noise
    assert m3[0, 0, :8].tolist() == [-2, 4, 0, 2, 2, 5, 0, 7]


# ------------------------------------------------------------------------------------------------ ABI, bindings
def test_header_declares_the_new_entries_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert not [s for s in NEW_SYMBOLS if s not in declared]
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert "ocr_component_scores: one detection score per component.  BUILD-DEFINED" in txt
    mk = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "Makefile")).read()
    assert "link_boxes" in re.search(r"^NOFMA := (.*)$", mk, flags=re.M).group(1).split()


def test_ops_and_tools_have_the_bindings():
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import pixellink_fn
    assert not [b for b in BINDINGS if not callable(getattr(ops, b, None))]
    assert callable(pixellink_fn.link_boxes_device) and callable(pixellink_fn.detect_device)
    assert issubclass(evaluate.LinkEvaluator, evaluate.Evaluator)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    I = torch.int32
    with pytest.raises(ValueError, match="do not match"):
        ops.component_scores(z(2, 4, 4, dt=I), z(2, 4, 5), z(2, dt=I), z(2, 3), None)
    with pytest.raises(ValueError, match="int32"):
        ops.component_scores(z(2, 4, 4), z(2, 4, 4), z(2, dt=I), z(2, 3), None)
    with pytest.raises(ValueError, match="do not match"):
        ops.link_boxes(z(2, 3, dt=I), z(2, 3, 4, dt=I), z(2, 3, 6), z(2, 3), z(2, dt=I), 0.0, 0.0, z(2, 3, 8), z(2, 3, dt=I),
                       z(2, dt=I), z(2, 3, dt=torch.uint8), z(2, dt=I))
    with pytest.raises(ValueError, match="uint8"):
        ops.link_boxes(z(2, 3, dt=I), z(2, 3, 4, dt=I), z(2, 3, 6), z(2, 3), z(2, dt=I), 0.0, 0.0, z(2, 3, 9), z(2, 3, dt=I),
                       z(2, dt=I), z(2, 3, dt=I), z(2, dt=I))


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
        assert lib.ocr_abi_version() == 7
        ws = lib.ocr_component_scores_workspace
        ws.restype = ctypes.c_size_t
        assert ws(3, 8) == 3 * 8 * 16 and ws(0, 8) == 0 and ws(3, 0) == 0 and ws(-1, 8) == 0
        assert ws(65535, 65535) == 65535 * 65535 * 16                       # no 32-bit overflow in the query
        # (no GPU is touched: every argument is checked before anything is launched)
        cs, lb = lib.ocr_component_scores, lib.ocr_link_boxes
        a = lambda lab=buf, ps=buf, nc=buf, n=3, h=20, w=300, mc=8, out=buf, wsp=buf, wsb=1 << 20: (
            lab, ps, nc, n, h, w, mc, out, wsp, SZ(wsb), None)
        for kw in (dict(lab=None), dict(ps=None), dict(nc=None), dict(out=None), dict(wsp=None), dict(n=0), dict(h=0),
                   dict(w=-1), dict(mc=0)):
            assert cs(*a(**kw)) == -1, kw
        for kw in (dict(n=65536), dict(mc=65536), dict(h=32769), dict(w=32769)):
            assert cs(*a(**kw)) == -2, kw
        assert cs(*a(wsb=3 * 8 * 16 - 1)) == -4
        b = lambda hn=buf, hd=buf, cal=buf, sc=buf, nc=buf, n=3, mc=8, m=buf, k=buf, nk=buf, p=buf, t=buf: (
            hn, hd, cal, sc, nc, n, mc, F(0), F(0), m, k, nk, p, t, None)
        for kw in (dict(hn=None), dict(hd=None), dict(cal=None), dict(sc=None), dict(nc=None), dict(m=None), dict(k=None),
                   dict(nk=None), dict(p=None), dict(t=None), dict(n=0), dict(mc=-3)):
            assert lb(*b(**kw)) == -1, kw
        assert lb(*b(n=65536)) == -2 and lb(*b(mc=65536)) == -2


# ------------------------------------------------------------------------------------------------ flags
def test_train_pixellink_parses_the_eval_flags(capsys):
    sys.path.insert(0, ROOT)
    T = importlib.import_module("train_pixellink")
    assert T.__file__.startswith(ROOT)
    d = T.parse([])
    assert (d.eval_data_path, d.eval_steps, d.eval_max_images, d.eval_weights) == (None, 0, None, "ema")
    assert (d.eval_image_height, d.eval_image_width) == (768, 1280)
    assert T.make_train_eval(d, None, None) is None                         # off by default: nothing is built
    f = T.parse(["--eval_data_path", "/data/val", "--eval_steps", "500", "--eval_max_images", "100", "--eval_weights", "raw"])
    assert (f.eval_data_path, f.eval_steps, f.eval_max_images, f.eval_weights) == ("/data/val", 500, 100, "raw")
    e = T.parse(["--eval_data_path", "/data/val", "--eval_steps", "5", "--using_moving_average"])
    assert e.eval_weights == "ema" and e.using_moving_average
    assert T.parse(["--eval_data_path", "/data/val"]).eval_steps == 0       # a path alone evaluates nothing
    messages = []
    for bad, message in ((["--eval_steps", "5", "--eval_weights", "raw"], "--eval_steps needs --eval_data_path"),
                         (["--eval_data_path", "/data/val", "--eval_steps", "-1"], "--eval_steps must not be negative"),
                         (["--eval_data_path", "/data/val", "--eval_steps", "5", "--eval_weights", "raw", "--eval_max_images", "0"],
                          "--eval_max_images must be positive"),
                         (["--eval_data_path", "/data/val", "--eval_steps", "5"], "--eval_weights ema needs --using_moving_average"),
                         (["--eval_data_path", "/data/val", "--eval_steps", "5", "--eval_weights", "best"], "invalid choice")):
        with pytest.raises(SystemExit):
            T.parse(bad)
        err = capsys.readouterr().err
        assert message in err, (bad, err)
        messages.append(err)
    # the same words as multigpu_train.py's
    M = importlib.import_module("multigpu_train")
    with pytest.raises(SystemExit):
        M.parse(["--net", "east", "--geometry", "RBOX", "--eval_steps", "5"])
    assert "--eval_steps needs --eval_data_path" in capsys.readouterr().err


def test_eval_pixellink_fast_parses_gt_path_and_the_filters(capsys):
    """the evaluation of test_pixellink_fast.py's decode is a script of its own; the flags the two share have one default"""
    sys.path.insert(0, ROOT)
    P = importlib.import_module("eval_pixellink_fast")
    assert P.__file__.startswith(ROOT)
    d = P.parse([])
    assert (d.gt_path, d.min_side, d.min_area, d.batch_size, d.synthetic) == (None, 0.0, 0.0, 8, 0)
    assert (d.eval_image_height, d.eval_image_width, d.pixel_conf_threshold, d.link_conf_threshold) == (768, 1280, 0.8, 0.9)
    assert (d.checkpoint_path, d.test_data_path, d.precision) == (None, "/tmp/images/", "f16")
    f = P.parse(["--gt_path", "/data/gt", "--min_side", "3.5", "--min_area", "40", "--synthetic", "2"])
    assert (f.gt_path, f.min_side, f.min_area, f.synthetic) == ("/data/gt", 3.5, 40.0, 2)
    for bad, message in ((["--min_side", "-1"], "must not be negative"), (["--min_area", "-0.5"], "must not be negative"),
                         (["--batch_size", "0"], "--batch_size must be positive"), (["--synthetic", "2"], "--synthetic needs --gt_path")):
        with pytest.raises(SystemExit):
            P.parse(bad)
        assert message in capsys.readouterr().err, bad
    # the shared flags carry test_pixellink_fast.py's defaults (read from its source: its parse() takes no argument list)
    src = open(os.path.join(ROOT, "test_pixellink_fast.py")).read()
    for flag, default in (("pixel_conf_threshold", "0.8"), ("link_conf_threshold", "0.9"), ("eval_image_width", "1280"),
                          ("eval_image_height", "768")):
        assert re.search(r"'--%s', type=\w+, default=%s\)" % (flag, re.escape(default)), src), flag


def test_the_east_scripts_still_refuse_link_geometry_evaluation(capsys):
    sys.path.insert(0, ROOT)
    east, M = importlib.import_module("test"), importlib.import_module("multigpu_train")
    with pytest.raises(SystemExit):
        east.parse(["--gt_path", "/data/gt"])
    assert "--gt_path needs --geometry RBOX" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        M.parse(["--net", "pixellink", "--eval_data_path", "/data/val", "--eval_steps", "5"])
    assert "need --net east --geometry RBOX" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ evaluator batching
def _write_gt(path, quads, tags):
    with open(path, "w") as f:
        for q, t in zip(quads, tags):
            f.write(",".join(str(int(v)) for v in np.asarray(q).reshape(-1)) + "," + t + "\r\n")


def test_link_evaluator_buckets_by_original_shape_and_scales_to_original_pixels(tmp_path, monkeypatch):
    """The whole pass on the host with every device entry replaced by a recorder: what reaches the forward, the decode
    and the collect step."""
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import bboxes, metrics, pixellink_fn
    d = str(tmp_path)
    shapes = {"a": (96, 128), "b": (96, 160), "c": (96, 128), "d": (96, 128), "e": (96, 160)}
    for name, (h, w) in shapes.items():
        np.save(os.path.join(d, name + ".npy"), np.zeros((h, w, 3), np.uint8))
        _write_gt(os.path.join(d, "gt_%s.txt" % name), [[1, 1, 9, 1, 9, 6, 1, 6]], ["text"])
    np.save(os.path.join(d, "f.npy"), np.zeros((96, 128, 3), np.uint8))     # no gt file: skipped

    class Acc:
        def __init__(self, graph):
            self.record, self.reads = torch.zeros(4, dtype=torch.int64), 0

        def reset(self):
            self.record.zero_()

        def value_with(self, extra):
            self.reads += 1
            return tuple(int(v) for v in self.record.tolist()), [int(v) for v in extra.tolist()]
    resized, decoded, collected = [], [], []
    monkeypatch.setattr(metrics, "DeviceTpFp", Acc)
    monkeypatch.setattr(ops, "resize_linear_u8", lambda src, dst: resized.append((tuple(src.shape), tuple(dst.shape))))
    monkeypatch.setattr(pixellink_fn, "pixel_scores", lambda t, graph=None: torch.zeros(tuple(t.shape)))
    monkeypatch.setattr(pixellink_fn, "link_scores", lambda t, graph=None: torch.zeros((8,) + tuple(t.shape[:3]) + (2,)))

    def detect_device(ps, ls, pixel_t, link_t, min_size, scale_x, scale_y, max_comps, min_side, min_area, graph):
        n = ps.shape[0]
        decoded.append(dict(maps=tuple(ps.shape), links=tuple(ls.shape), thresholds=(pixel_t, link_t), min_size=min_size,
                            scale=(scale_x, scale_y), max_comps=max_comps, filters=(min_side, min_area)))
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
        return z(n, max_comps, 9, dt=torch.float32), z(n, max_comps), z(n), z(n, max_comps, dt=torch.uint8), z(n)

    def eval_collect(merged, keep, n_keep, passed, inv_ratio, dets, det_score, nd, nd_total):
        collected.append((inv_ratio.tolist(), tuple(dets.shape)))
        nd.zero_()
        nd_total.zero_()

    def matching(dets, nd, gts, ng, gign, thr, record=None, graph=None, mask_hw=None):
        record += torch.tensor([int(ng.sum()), 0, 0, 0])
        return None, None, None
    monkeypatch.setattr(pixellink_fn, "detect_device", detect_device)
    monkeypatch.setattr(ops, "eval_collect", eval_collect)
    monkeypatch.setattr(bboxes, "bboxes_matching_batch", matching)
    forwarded = []

    def forward(x):
        forwarded.append(tuple(x.shape))
        n, h, w, _ = x.shape
        return torch.zeros((n, h // 4, w // 4, 2)), torch.zeros((n, h // 4, w // 4, 16))
    g = types.SimpleNamespace(device=torch.device("cpu"))
    ev = evaluate.LinkEvaluator(g, forward, d, batch_size=2, eval_image_height=128, eval_image_width=256, max_comps=64,
                                min_side=2.0, min_area=9.0)
    res = ev.run()
    # every image enters the network at the eval size; a batch holds images of ONE original shape
    assert forwarded == [(2, 128, 256, 3), (2, 128, 256, 3), (1, 128, 256, 3)]      # a c | b e | d (a full bucket goes first)
    assert [r[0] for r in resized] == [(96, 128, 3), (96, 128, 3), (96, 160, 3), (96, 160, 3), (96, 128, 3)]
    assert {r[1] for r in resized} == {(128, 256, 3)}
    # scale = original / (eval / 4): map cell -> original-image pixels, so the collect step divides by (1, 1)
    assert [c["scale"] for c in decoded] == [(128 / 64.0, 96 / 32.0), (160 / 64.0, 96 / 32.0), (128 / 64.0, 96 / 32.0)]
    assert all(c["maps"][1:] == (32, 64) and c["links"] == (8, c["maps"][0], 32, 64, 2) for c in decoded)
    assert all(c["thresholds"] == (0.8, 0.9) and c["min_size"] == 10 and c["max_comps"] == 64 and c["filters"] == (2.0, 9.0)
               for c in decoded)
    assert [c[0] for c in collected] == [[[1.0, 1.0]] * 2, [[1.0, 1.0]] * 2, [[1.0, 1.0]]]
    assert all(c[1][1:] == (ops.EVAL_MAX_D, 4, 2) for c in collected)
    assert sorted(res) == sorted(["precision", "recall", "hmean", "num_gt", "tp", "fp", "num_det", "images"])
    assert res["images"] == 5 and res["num_gt"] == 5 and ev.acc.reads == 1
    # the defaults are test_pixellink_fast.py's; an original smaller than the score maps is refused
    dflt = evaluate.LinkEvaluator(g, forward, d)
    assert dflt.eval_hw == (768, 1280) and (dflt.pixel_conf_threshold, dflt.link_conf_threshold) == (0.8, 0.9)
    assert (dflt.min_size, dflt.max_comps, dflt.max_d, dflt.min_side, dflt.min_area) == (10, 4096, ops.EVAL_MAX_D, 0.0, 0.0)
    assert dflt.scales(720, 1280) == (4.0, 3.75) and dflt.scales(192, 320) == (1.0, 1.0)
    with pytest.raises(ValueError, match="smaller than"):
        dflt.scales(96, 1280)
    with pytest.raises(ValueError, match="multiples of 4"):
        evaluate.LinkEvaluator(g, forward, d, eval_image_height=130)
    # the RBOX evaluator's sizing is what it was
    rb = evaluate.Evaluator(g, forward, d)
    assert rb.detector.resized(720, 1280) == (672, 1280) and rb.detector.ratio(720, 1280, 672, 1280) == (1.0, 672 / 720.0)
