"""CPU: host side of multi-scale RBOX inference (csrc/multiscale.hip, include/ocr_multiscale.h, tool/rbox.py's
detect_multiscale, evaluate.Evaluator's `scales`).  The hand cases pin the reference of tests/ms_ref.py — which the GPU
tests compare the device with — to results worked out by hand; then the sizing of the scales, the flags of the scripts,
the C ABI's declarations and bindings, and a condition on the case generators that keeps the GPU cases from being vacuous."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

import ms_ref as M
from oracle import lanms as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ("ocr_ms_pool_append", "ocr_quad_fuse_workspace", "ocr_quad_fuse")


# ------------------------------------------------------------------------------------------------ the reference, by hand
def test_chain_b_is_claimed_by_a_so_c_is_kept():
    pool, thr = M.hand_cases()["chain"]
    assert OL.iou(pool[0, :8], pool[1, :8]) > thr and OL.iou(pool[1, :8], pool[2, :8]) > thr
    assert OL.iou(pool[0, :8], pool[2, :8]) == 0.0
    fused, keep, owner = M.fuse_ref(pool, thr, "nms")
    assert keep.tolist() == [0, 2] and owner.tolist() == [0, 0, 2]
    assert np.array_equal(fused.view(np.int32), pool.view(np.int32))
    # vote: A = (A * 0.9 + B * 0.8) / 1.7 in float64, C alone stays what it is (its weight cancels up to rounding)
    voted, keep1, owner1 = M.fuse_ref(pool, thr, "vote")
    assert keep1.tolist() == [0, 2] and owner1.tolist() == [0, 0, 2]
    sa, sb = float(f32(0.9)), float(f32(0.8))
    want = [f32((sa * float(pool[0, c]) + sb * float(pool[1, c])) / (sa + sb)) for c in range(8)]
    assert voted[0, :8].tolist() == want and voted[0, 8] == pool[0, 8]
    assert np.array_equal(voted[1], pool[1]) and np.allclose(voted[2], pool[2], rtol=1e-6)


def test_equal_scores_resolve_by_pool_order():
    pool, thr = M.hand_cases()["ties"]
    assert M.rank(pool[:, 8]).tolist() == [0, 1, 2, 3]
    assert M.rank(np.array([0.5, np.nan, 0.75, 0.5, np.nan], f32)).tolist() == [2, 0, 3, 1, 4]          # NaN last, stable
    _, keep, owner = M.fuse_ref(pool, thr, "nms")
    assert keep.tolist() == [0, 2] and owner.tolist() == [0, 0, 2, 2]
    _, keep, owner = M.fuse_ref(pool[::-1].copy(), thr, "nms")               # the same quads the other way round
    assert keep.tolist() == [2, 0] and owner.tolist() == [0, 0, 2, 2]


def test_a_member_stored_one_corner_round_votes_after_its_shift():
    pool, thr = M.hand_cases()["rolled"]
    assert M.best_shift(pool[1], pool[0]) == 3 and M.best_shift(pool[0], pool[0]) == 0
    voted, keep, owner = M.fuse_ref(pool, thr, "vote")
    assert keep.tolist() == [0] and owner.tolist() == [0, 0]
    # weights 1 and 0.5: every corner moves a third of the way to the member's MATCHING corner, (4, 2) further out
    want = np.array([0, 0, 100, 0, 100, 20, 0, 20], np.float64) + np.tile([4 / 3.0, 2 / 3.0], 4)
    assert np.allclose(voted[0, :8], want, rtol=0, atol=1e-5)
    unshifted = (pool[0, :8].astype(np.float64) + 0.5 * pool[1, :8]) / 1.5
    assert np.abs(unshifted - want).max() > 30                               # without the shift the corners would rotate
    assert np.array_equal(voted[1], pool[1])


def test_zero_weight_leaves_the_coordinates():
    pool, thr = M.hand_cases()["zero_weight"]
    voted, keep, owner = M.fuse_ref(pool, thr, "vote")
    assert keep.tolist() == [0] and owner.tolist() == [0, 0]
    assert np.array_equal(voted.view(np.int32), pool.view(np.int32))


def test_append_reference_by_hand():
    merged = np.zeros((4, 9), f32)
    merged[:, :8] = np.arange(32, dtype=f32).reshape(4, 8) * 3
    merged[:, 8] = [10, 20, 30, 40]                                          # LANMS's sums: not what is pooled
    merged[2, 5] = np.nan
    keep, mean = np.array([3, 2, 0, 1], np.int32), np.array([0.9, 0.8, 0.7, 0.6], f32)
    pool, scale, counters = np.full((2, 9), -1, f32), np.full(2, -1, np.int32), [0, 0, 0]
    M.append_ref(pool, scale, counters, merged, keep, 3, None, mean, np.array([1.5, 0.75], f32), 4)
    # slots 0 (row 3), 1 (row 2: NaN, dropped), 2 (row 0); slot 3 is beyond n_keep
    assert counters == [2, 2, 1] and scale.tolist() == [4, 4]
    assert pool[0].tolist() == [f32(v) / f32(0.75 if k & 1 else 1.5) for k, v in enumerate(merged[3, :8])] + [f32(0.9)]
    assert pool[1, 8] == f32(0.7)
    M.append_ref(pool, scale, counters, merged, keep, 4, np.array([1, 0, 0, 1], bool), mean, np.array([1, 1], f32), 5)
    assert counters == [2, 4, 1] and scale.tolist() == [4, 4] and pool[1, 8] == f32(0.7)         # overflow: counted, not written


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("thr", M.FUSE_THRESHOLDS)
def test_generated_cases_are_not_vacuous(thr):
    """what tests/test_gpu_multiscale.py relies on: for every case with P >= 63 the reference keeps at least a quarter of
    the pooled quads and claims at least a quarter, and some cluster has a member claimed by a quad that is not the
    cluster's top-scoring one; equal scores and shifted corners are there"""
    for (pool, scale, cluster), P in zip(M.fuse_batch(), M.FUSE_COUNTS):
        assert pool.shape == (P, 9) and (np.diff(scale) >= 0).all()          # scale-major
        if P < 63:
            continue
        fused, keep, owner = M.fuse_ref(pool, thr, "vote")
        claimed = P - len(keep)
        assert 4 * len(keep) >= P and 4 * claimed >= P, (P, thr, len(keep))
        order = M.rank(pool[:, 8])
        top = {}
        for j in order:
            top.setdefault(int(cluster[j]), int(j))
        assert any(owner[j] != j and owner[j] != top[int(cluster[j])] for j in range(P)), (P, thr)
        assert len(np.unique(pool[:, 8])) < P / 2                            # ties
        assert any(M.best_shift(pool[j], pool[owner[j]]) != 0 for j in range(P) if owner[j] != j)
        moved = [k for k in keep if not np.array_equal(fused[k, :8], pool[k, :8])]
        assert len(moved) >= len(keep) // 4                                  # the vote has something to move


# ------------------------------------------------------------------------------------------------ scale_sizes
def test_scale_sizes_follow_the_resize_rule():
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import rbox
    h, w = 720, 1280
    scales = [0.5, 1, 2, 1.3]
    want = [evaluate.resize_rule(int(round(h * s)), int(round(w * s)), 3000) for s in scales]
    assert rbox.scale_sizes(h, w, scales) == want == [(320, 640), (672, 1280), (1440, 2560), (896, 1664)]
    assert rbox.scale_sizes(h, w, [4]) == [evaluate.resize_rule(2880, 5120, 3000)]        # the longer side is limited
    assert rbox.scale_sizes(h, w, [1], max_side_len=640) == [evaluate.resize_rule(h, w, 640)]
    assert rbox.scale_sizes(64, 96, (1.0,)) == [(64, 96)]
    for bad in ([], [1] * 9, [0], [-1], [float("nan")], [float("inf")], [1, 1], 3):
        with pytest.raises(ValueError):
            rbox.scale_sizes(h, w, bad)
    with pytest.raises(ValueError, match="again"):
        rbox.scale_sizes(h, w, [1.01, 1.02])                                 # two scales, one size (672 x 1248) after the rule
    with pytest.raises(ValueError, match="scale 0.01"):
        rbox.scale_sizes(h, w, [1, 0.01])                                    # the rule's error, naming the scale
    assert rbox.parse_scales("0.5,1,2") == [0.5, 1.0, 2.0]
    for bad in ("", "1,1", "0", "a", "1,-2"):
        with pytest.raises(ValueError):
            rbox.parse_scales(bad)


# ------------------------------------------------------------------------------------------------ scripts
def test_scales_and_fuse_parse_in_the_scripts(capsys):
    sys.path.insert(0, ROOT)
    east, mg = importlib.import_module("test"), importlib.import_module("multigpu_train")
    assert all(m.__file__.startswith(ROOT) for m in (east, mg))
    none = east.parse([])
    assert none.scales is None and none.fuse == "nms"
    F = east.parse(["--geometry", "RBOX", "--scales", "0.5,1,2", "--fuse", "vote"])
    assert F.scales == [0.5, 1.0, 2.0] and F.fuse == "vote"
    assert east.parse(["--geometry", "RBOX", "--scales", "1"]).fuse == "nms"
    for argv in (["--scales", "0.5,1"], ["--geometry", "link", "--scales", "1,2"], ["--geometry", "RBOX", "--fuse", "vote"],
                 ["--geometry", "RBOX", "--scales", "1,1"], ["--geometry", "RBOX", "--scales", "0"],
                 ["--geometry", "RBOX", "--scales", "1", "--fuse", "mean"]):
        with pytest.raises(SystemExit):
            east.parse(argv)
    rb = ["--net", "east", "--geometry", "RBOX", "--eval_data_path", "/data/val", "--eval_steps", "5"]
    T = mg.parse(rb)
    assert T.eval_scales is None and T.eval_fuse == "nms"
    T = mg.parse(rb + ["--eval_scales", "0.5,1,2", "--eval_fuse", "vote"])
    assert T.eval_scales == [0.5, 1.0, 2.0] and T.eval_fuse == "vote"
    for argv in (["--eval_scales", "1,2"], rb + ["--eval_fuse", "vote"], rb + ["--eval_scales", "x"]):
        with pytest.raises(SystemExit):
            mg.parse(argv)
    capsys.readouterr()


def test_evaluators_check_the_options(tmp_path):
    from tensorflow_ocr_amd import evaluate
    with pytest.raises(ValueError, match="RBOX geometry only"):
        evaluate.LinkEvaluator(None, None, str(tmp_path), scales=[0.5, 1])
    for kw in (dict(scales=[]), dict(scales=[0]), dict(scales=[1] * 9), dict(fuse="mean"), dict(max_pool=0), dict(max_pool=4097)):
        with pytest.raises(ValueError):
            evaluate.Evaluator(None, None, str(tmp_path), **kw)
    with pytest.raises(FileNotFoundError):                                   # good options get as far as the empty directory
        evaluate.Evaluator(None, None, str(tmp_path), scales=[0.5, 1, 2], fuse="vote", max_pool=4096)


# ------------------------------------------------------------------------------------------------ ABI, bindings
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_exactly_the_new_entries_and_keeps_the_abi_version():
    hip = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    assert re.search(r'^#include "ocr_multiscale\.h"$', hip, flags=re.M)
    assert _declared("ocr_multiscale.h") == set(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", hip)
    txt = open(os.path.join(ROOT, "include", "ocr_multiscale.h")).read()
    for word in ("BUILD-DEFINED", "mean pixel score", "pool order", "cyclic", "unpinned", "unmeasured"):
        assert word in txt, word
    mk = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "Makefile")).read()
    assert "multiscale" in re.search(r"^NOFMA := (.*)$", mk, flags=re.M).group(1).split()
    assert "ocr_multiscale.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1)
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7


def test_ops_bindings_check_shapes_and_dtypes():
    import torch
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import rbox
    for name in ("ms_pool_append", "quad_fuse"):
        assert callable(getattr(ops, name, None)), name
    for name in ("scale_sizes", "detect_multiscale_device", "detect_multiscale"):
        assert callable(getattr(rbox, name, None)), name
    assert ops.FUSE_MAX_POOL == 4096
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
    F, U8 = torch.float32, torch.uint8
    n, k, p = 2, 5, 7
    ok = dict(merged=z(n, k, 9, dt=F), keep_idx=z(n, k), n_keep=z(n), passed=z(n, k, dt=U8), mean=z(n, k, dt=F),
              ratio=z(n, 2, dt=F), scale_id=0, pool=z(n, p, 9, dt=F), pool_scale=z(n, p), pool_count=z(n), pool_total=z(n),
              pool_nonfinite=z(n))
    for kw in (dict(keep_idx=z(n, k + 1)), dict(mean=z(n, k + 1, dt=F)), dict(ratio=z(n, 3, dt=F)), dict(pool=z(n, p, 8, dt=F)),
               dict(pool_scale=z(n, p + 1)), dict(pool_count=z(n + 1)), dict(passed=z(n, k + 1, dt=U8)),
               dict(passed=z(n, k, dt=torch.bool)), dict(mean=z(n, k)), dict(keep_idx=z(n, k, dt=torch.int64)),
               dict(pool=z(n, p, 9, dt=torch.float64)), dict(merged=z(n, 9, k, dt=F).transpose(1, 2))):
        with pytest.raises(ValueError, match="ms_pool_append"):
            ops.ms_pool_append(**dict(ok, **kw))
    fok = dict(pool=z(n, p, 9, dt=F), pool_count=z(n), iou_thresh=0.2, mode="nms", fused=z(n, p, 9, dt=F), keep_idx=z(n, p),
               n_keep=z(n), owner=z(n, p), ws=None)
    for kw in (dict(mode=2), dict(mode="mean"), dict(fused=z(n, p + 1, 9, dt=F)), dict(keep_idx=z(n, p + 1)), dict(owner=z(n, p, dt=F)),
               dict(n_keep=z(n + 1)), dict(pool_count=z(n, dt=torch.int64)), dict(fused=fok["pool"]),
               dict(pool=z(n, 4097, 9, dt=F), fused=z(n, 4097, 9, dt=F), keep_idx=z(n, 4097), owner=z(n, 4097))):
        with pytest.raises(ValueError, match="quad_fuse"):
            ops.quad_fuse(**dict(fok, **kw))


def test_both_product_libraries_export_the_entries_and_check_their_arguments():
    import ctypes
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = ctypes.create_string_buffer(256)
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        assert lib.ocr_abi_version() == 7
        ws = lib.ocr_quad_fuse_workspace
        ws.restype = ctypes.c_size_t
        assert ws(0, 64) == 0 and ws(2, 0) == 0 and ws(1, 4097) == 0
        # the mask alone: n * max_pool rows of ceil(max_pool / 64) words
        assert ws(8, 4096) >= 8 * 4096 * 64 * 8 and ws(3, 100) >= 3 * 100 * 2 * 8
        fuse = lambda *a: lib.ocr_quad_fuse(*[ctypes.c_float(v) if isinstance(v, float) else
                                              (ctypes.c_size_t(v[0]) if isinstance(v, tuple) else v) for v in a])
        # refusals are decided before anything is launched: host memory stands in for the device pointers
        assert fuse(None, buf, 1, 64, 0.2, 0, buf, buf, buf, buf, buf, (1 << 30,), None) == -1
        assert fuse(buf, buf, 1, 64, 0.2, 2, buf, buf, buf, buf, buf, (1 << 30,), None) == -1
        assert fuse(buf, buf, 0, 64, 0.2, 0, buf, buf, buf, buf, buf, (1 << 30,), None) == -1
        assert fuse(buf, buf, 1, 4097, 0.2, 0, buf, buf, buf, buf, buf, (1 << 30,), None) == -2
        assert fuse(buf, buf, 1, 64, 0.2, 1, buf, buf, buf, buf, buf, (ws(1, 64) - 1,), None) == -4
        app = lib.ocr_ms_pool_append
        assert app(buf, buf, buf, None, buf, buf, 0, 1, 8, 0, buf, buf, buf, buf, buf, None) == -1
        assert app(buf, buf, buf, None, None, buf, 0, 1, 8, 8, buf, buf, buf, buf, buf, None) == -1
        assert app(buf, buf, buf, None, buf, buf, -1, 1, 8, 8, buf, buf, buf, buf, buf, None) == -1
