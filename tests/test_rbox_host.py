"""CPU: host side of the EAST RBOX geometry — the C ABI's declarations and bindings, the float64 restatement of the
per-pixel decode that tests/test_gpu_rbox.py holds the kernel to (checked here against answers worked out by hand), the
three-way checkpoint split of the merged head variable, the synthetic label maps and the test.py flags.

The three test_decode_restatement_* tests check this file's own float64 helper and nothing of the package, so they pass
with or without the feature; every other test here needs it."""
import ctypes
import importlib
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ocr_rbox_head_fwd", "ocr_rbox_head_bwd", "ocr_rbox_loss_workspace", "ocr_rbox_loss_fwd", "ocr_rbox_loss_bwd",
               "ocr_rbox_loss_bwd_dyn", "ocr_rbox_decode_workspace", "ocr_rbox_decode"]
BINDINGS = ["rbox_head_fwd", "rbox_head_bwd", "rbox_loss_fwd", "rbox_loss_bwd", "rbox_loss_bwd_dyn", "rbox_decode"]


# ------------------------------------------------------------------------------------------------ float64 restatement
def decode_ref(score, geo, thresh, scale=4.0):
    """score [h,w], geo [h,w,5] (any float type; `thresh` compared in the score's own type) -> [k,9] float64 rows
    x1,y1,..,x4,y4,score of the pixels with score > thresh in raster order, from the formulas of include/ocr_hip.h:
    origin = (x scale, y scale), H = d0 + d2, W = d1 + d3, R(q) = (qx cos + qy sin, -qx sin + qy cos),
    theta >= 0: corners (0,-H) (W,-H) (W,0) (0,0), anchor (d3,-d2); theta < 0: (-W,-H) (0,-H) (0,0) (-W,0), anchor
    (-d1,-d2); corner = origin + R(corner) - R(anchor)."""
    score = np.asarray(score)
    h, w = score.shape
    ys, xs = np.nonzero(score > score.dtype.type(thresh))             # np.nonzero walks in raster order
    rows = np.zeros((len(ys), 9), np.float64)
    for r, (y, x) in enumerate(zip(ys, xs)):
        d0, d1, d2, d3, th = (float(v) for v in np.asarray(geo)[y, x])
        H, W = d0 + d2, d1 + d3
        c, s = math.cos(th), math.sin(th)

        def R(q):
            return np.array([q[0] * c + q[1] * s, -q[0] * s + q[1] * c])
        if th >= 0:
            local, anchor = [(0, -H), (W, -H), (W, 0), (0, 0)], (d3, -d2)
        else:
            local, anchor = [(-W, -H), (0, -H), (0, 0), (-W, 0)], (-d1, -d2)
        origin = np.array([x * scale, y * scale], np.float64)
        for k, q in enumerate(local):
            rows[r, 2 * k:2 * k + 2] = origin + R(q) - R(anchor)
        rows[r, 8] = float(score[y, x])
    return rows


def _one(d, theta, origin, scale=4.0):
    """the quad of one pixel at `origin` (a multiple of `scale` per axis)"""
    x, y = int(origin[0] / scale), int(origin[1] / scale)
    assert (x * scale, y * scale) == tuple(origin)
    score = np.zeros((y + 1, x + 1), np.float32)
    geo = np.zeros((y + 1, x + 1, 5), np.float64)
    score[y, x] = 1.0
    geo[y, x] = list(d) + [theta]
    rows = decode_ref(score, geo, 0.5, scale)
    assert rows.shape == (1, 9) and rows[0, 8] == 1.0
    return rows[0, :8].reshape(4, 2)


def _dist_to_line(p, a, b):
    (ax, ay), (bx, by) = a, b
    return abs((bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)) / math.hypot(bx - ax, by - ay)


def test_decode_restatement_meets_the_known_answer_and_its_mirror():
    q = _one((1, 2, 3, 4), 0.0, (10, 20), scale=2.0)
    assert np.array_equal(q, np.array([[6, 19], [12, 19], [12, 23], [6, 23]], np.float64))
    assert np.array_equal(_one((1, 2, 3, 4), 0.0, (12, 20)), q + [2, 0])
    # theta < 0 takes the other corner layout: as theta -> 0- it must give the same rectangle
    m = _one((1, 2, 3, 4), -1e-300, (10, 20), scale=2.0)
    assert np.allclose(m, q, rtol=0, atol=1e-12)


@pytest.mark.parametrize("theta", [math.pi / 6, -math.pi / 6])
def test_decode_restatement_at_thirty_degrees(theta):
    """By hand: a W x H rectangle whose right-pointing side is (cos, -sin) of theta (y down), the pixel d0 / d1 / d2 /
    d3 away from its top / right / bottom / left side."""
    d, origin = (5.0, 7.0, 3.0, 11.0), (40, 24)
    q = _one(d, theta, origin)
    W, H = d[1] + d[3], d[0] + d[2]
    side = lambda i, j: math.hypot(*(q[i] - q[j]))
    assert np.allclose([side(0, 1), side(2, 3)], W, rtol=0, atol=1e-12)
    assert np.allclose([side(1, 2), side(3, 0)], H, rtol=0, atol=1e-12)
    assert abs(np.dot(q[1] - q[0], q[2] - q[1])) < 1e-12                             # a rectangle
    top = (q[1] - q[0]) / W
    assert np.allclose(top, [math.cos(theta), -math.sin(theta)], rtol=0, atol=1e-12)
    got = [_dist_to_line(origin, q[0], q[1]), _dist_to_line(origin, q[1], q[2]),
           _dist_to_line(origin, q[2], q[3]), _dist_to_line(origin, q[3], q[0])]
    assert np.allclose(got, d, rtol=0, atol=1e-12)
    # the corner worked out on paper for theta = +30 degrees: q3 = origin + R((0,0)) - R((d3,-d2))
    if theta > 0:
        c, s = math.sqrt(3) / 2, 0.5
        assert np.allclose(q[3], [40 - (11 * c - 3 * s), 24 - (-11 * s - 3 * c)], rtol=0, atol=1e-12)


def test_decode_restatement_order_and_threshold():
    score = np.array([[0.9, 0.8, 0.81], [0.1, 0.95, 0.8]], np.float32)
    geo = np.ones((2, 3, 5), np.float32) * np.array([1, 1, 1, 1, 0], np.float32)
    rows = decode_ref(score, geo, 0.8)
    assert rows[:, 8].astype(np.float32).tolist() == [np.float32(0.9), np.float32(0.81), np.float32(0.95)]   # > is strict
    assert rows[:, 0].tolist() == [-1.0, 7.0, 3.0]


# ------------------------------------------------------------------------------------------------ ABI, bindings
def test_header_declares_every_new_symbol_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert not [s for s in NEW_SYMBOLS if s not in declared]
    assert sorted(s for s in declared if s.startswith("ocr_rbox_")) == sorted(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert "PARITY IS UNPINNED" in txt          # the loss is build-defined and the header says so


def test_ops_has_the_bindings():
    from tensorflow_ocr_amd import ops
    assert not [b for b in BINDINGS if not callable(getattr(ops, b, None))]


def test_both_product_libraries_export_the_new_symbols_and_check_their_arguments():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = ctypes.create_string_buffer(64)
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        dws, lws = lib.ocr_rbox_decode_workspace, lib.ocr_rbox_loss_workspace
        dws.restype = lws.restype = ctypes.c_size_t
        assert dws(2, 37, 53) == 2 * 8 * 4 and dws(1, 16, 16) == 4 and dws(1, 0, 5) == 0      # ceil(1961 / 256) = 8
        assert lws(1) == lws(1024) == 32 and lws(1025) == 64 and lws(1 << 30) == 1024 * 32 and lws(0) == 0
        # (no GPU is touched: every argument is checked before anything is launched)
        F = ctypes.c_float
        assert lib.ocr_rbox_head_fwd(None, 4, F(512), buf, buf, None) == -1
        assert lib.ocr_rbox_head_fwd(buf, 0, F(512), buf, buf, None) == -1
        assert lib.ocr_rbox_head_bwd(buf, None, buf, None, 4, F(512), None, None) == -1
        assert lib.ocr_rbox_loss_fwd(buf, buf, buf, buf, buf, 2000, buf, buf, buf, ctypes.c_size_t(63), None) == -4
        assert lib.ocr_rbox_loss_fwd(buf, buf, buf, buf, None, 4, buf, buf, buf, ctypes.c_size_t(64), None) == -1
        assert lib.ocr_rbox_loss_bwd(buf, buf, buf, buf, 0, buf, F(1), buf, buf, None) == -1
        assert lib.ocr_rbox_loss_bwd_dyn(buf, buf, buf, buf, 4, buf, F(1), None, buf, buf, None) == -1
        dec = lib.ocr_rbox_decode
        assert dec(buf, buf, 2, 37, 53, F(0.8), F(4), 16, buf, buf, buf, buf, ctypes.c_size_t(63), None) == -4
        assert dec(buf, buf, 2, 0, 53, F(0.8), F(4), 16, buf, buf, buf, buf, ctypes.c_size_t(64), None) == -1
        assert dec(buf, buf, 2, 37, 53, F(0.8), F(4), 0, buf, buf, buf, buf, ctypes.c_size_t(64), None) == -1
        assert dec(buf, None, 2, 37, 53, F(0.8), F(4), 16, buf, buf, buf, buf, ctypes.c_size_t(64), None) == -1
        assert dec(buf, buf, 70000, 4, 4, F(0.8), F(4), 16, buf, buf, buf, buf, ctypes.c_size_t(1 << 20), None) == -2


# ------------------------------------------------------------------------------------------------ checkpoint
def test_three_way_checkpoint_split_round_trips():
    from tensorflow_ocr_amd import checkpoint
    rng = np.random.default_rng(5)
    tf_sd = {"feature_fusion/Conv_7/weights": rng.standard_normal((1, 1, 32, 1)).astype(np.float32),
             "feature_fusion/Conv_8/weights": rng.standard_normal((1, 1, 32, 4)).astype(np.float32),
             "feature_fusion/Conv_9/weights": rng.standard_normal((1, 1, 32, 1)).astype(np.float32),
             "feature_fusion/Conv_7/biases": rng.standard_normal(1).astype(np.float32),
             "feature_fusion/Conv_8/biases": rng.standard_normal(4).astype(np.float32),
             "feature_fusion/Conv_9/biases": rng.standard_normal(1).astype(np.float32)}
    names = ["feature_fusion/Conv_7+Conv_8+Conv_9/weights", "feature_fusion/Conv_7+Conv_8+Conv_9/biases"]
    isd = checkpoint.tf_to_internal(names, tf_sd)
    assert isd[names[0]].shape == (32, 6) and isd[names[1]].shape == (6,)
    assert np.array_equal(isd[names[0]][:, 1:5], tf_sd["feature_fusion/Conv_8/weights"][0, 0])
    assert np.array_equal(isd[names[1]][5:], tf_sd["feature_fusion/Conv_9/biases"])
    back = checkpoint.internal_to_tf(isd)
    assert sorted(back) == sorted(tf_sd)
    for k, v in tf_sd.items():
        assert back[k].shape == v.shape and np.array_equal(back[k], v), k
    # a checkpoint that lacks one of the three leaves the merged variable alone
    del tf_sd["feature_fusion/Conv_9/weights"]
    assert names[0] not in checkpoint.tf_to_internal(names, tf_sd)
    # the two-way splits are what they were
    assert checkpoint._guess_widths(9, 2) == (1, 8) and checkpoint._guess_widths(18, 2) == (2, 16)


# ------------------------------------------------------------------------------------------------ labels, flags
def test_synthetic_rbox_labels_invert_through_the_decode():
    """every labelled pixel of a rectangle decodes to that rectangle's corners"""
    from tensorflow_ocr_amd import synthetic
    score, geo, mask = synthetic.rbox_labels(2, 64, np.random.default_rng(3), rects=1)
    assert score.shape == (2, 16, 16, 1) and geo.shape == (2, 16, 16, 5) and mask.shape == (2, 16, 16, 1)
    assert score.dtype == geo.dtype == mask.dtype == np.float32 and (mask == 1).all()
    assert set(np.unique(score)) == {0.0, 1.0} and (geo[score[..., 0] == 0] == 0).all()
    for b in range(2):
        inside = score[b, ..., 0] == 1
        assert inside.sum() >= 4 and (geo[b][inside][:, :4] >= 0).all() and (np.abs(geo[b][inside][:, 4]) < math.pi / 4).all()
        rows = decode_ref(score[b, ..., 0], geo[b], 0.5)
        assert len(rows) == inside.sum()
        assert np.abs(rows[:, :8] - rows[0, :8]).max() < 1e-3          # f32 labels: one rectangle, seen from every pixel


def test_test_py_parses_the_geometry_flag():
    sys.path.insert(0, ROOT)
    east = importlib.import_module("test")
    assert east.__file__.startswith(ROOT)
    d = east.parse([])
    assert d.geometry == "link" and d.text_scale == 512
    r = east.parse(["--geometry", "RBOX", "--text_scale", "256", "--precision", "f16x2"])
    assert (r.geometry, r.text_scale, r.precision) == ("RBOX", 256, "f16x2")
    with pytest.raises(SystemExit):
        east.parse(["--geometry", "QUAD"])
