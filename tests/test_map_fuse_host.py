"""CPU: host side of score-map fusion for the link geometry (csrc/map_fuse.hip, include/ocr_map_fuse.h,
pixellink_fn.fuse_score_maps, evaluate.LinkEvaluator's map_scales / flip).  The build wiring, the mirrored direction
pairing re-derived from decode.hip's own table, hand cases that pin the reference of tests/mapfuse_ref.py — which the GPU
tests compare the device with — and the sizes, options and flags."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

import mapfuse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ("ocr_link_map_accumulate",)


# ------------------------------------------------------------------------------------------------ build wiring
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_is_included_declares_the_entry_and_the_makefile_knows_it():
    hip = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    assert re.search(r'^#include "ocr_map_fuse\.h"$', hip, flags=re.M)
    assert _declared("ocr_map_fuse.h") == set(NEW_SYMBOLS)
    assert re.search(r"#define OCR_ABI_VERSION 7\b", hip)
    txt = open(os.path.join(ROOT, "include", "ocr_map_fuse.h")).read()
    for word in ("BUILD-DEFINED", "not logits", "unmeasured", "half-pixel", "NORMALISED"):
        assert word in txt, word
    mk = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "Makefile")).read()
    assert "map_fuse" in re.search(r"^NOFMA := (.*)$", mk, flags=re.M).group(1).split()
    assert "ocr_map_fuse.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1)
    assert os.path.exists(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "map_fuse.hip"))
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7


def test_both_product_libraries_export_the_entry_and_check_its_arguments():
    import ctypes
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(base.value + 4)
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        fn = lib.ocr_link_map_accumulate
        call = lambda px, lk, n, hs, ws, flip, wt, first, acc, hf, wf: fn(
            px, lk, n, hs, ws, flip, ctypes.c_float(wt), first, acc, hf, wf, None)
        # refusals are decided before anything is launched: host memory stands in for the device pointers
        assert call(None, base, 1, 4, 4, 0, 1.0, 1, base, 4, 4) == -1
        assert call(base, None, 1, 4, 4, 0, 1.0, 1, base, 4, 4) == -1
        assert call(base, base, 1, 4, 4, 0, 1.0, 1, None, 4, 4) == -1
        assert call(base, odd, 1, 4, 4, 0, 1.0, 1, base, 4, 4) == -1                  # a link row is read with 16-byte loads
        for bad in ((0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 0, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, -1)):
            n, hs, ws, hf, wf = bad
            assert call(base, base, n, hs, ws, 0, 1.0, 1, base, hf, wf) == -1, bad
        for wt in (0.0, -0.5, float("inf"), float("nan")):
            assert call(base, base, 1, 4, 4, 0, wt, 1, base, 4, 4) == -1, wt
        assert call(base, base, 65536, 1, 1, 0, 1.0, 1, base, 1, 1) == -2
        assert call(base, base, 2, 32768, 32768, 0, 1.0, 1, base, 4, 4) == -2
        assert call(base, base, 2, 4, 4, 0, 1.0, 1, base, 32768, 32768) == -2


def test_grid_cap_is_below_the_size_the_gpu_test_loops_at():
    """tests/test_gpu_map_fuse.py's grid-cap case (600 x 700 cells) needs a second pass of the grid-stride loop"""
    src = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "map_fuse.hip")).read()
    cap = int(re.search(r"constexpr unsigned kMaxBlocks = (\d+);", src).group(1))
    assert 600 * 700 > cap * 256 and re.search(r"b > kMaxBlocks", src)


# ------------------------------------------------------------------------------------------------ the mirrored pairing
def test_perm_rederived_from_decode_hip_mirrors_dx_keeps_dy_and_is_an_involution():
    dx, dy = R.parse_tables("decode.hip")
    assert sorted(zip(dx, dy)) == sorted((a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0))
    perm = R.mirror_perm(dx, dy)
    assert sorted(perm) == list(range(8))
    for d in range(8):
        assert dx[perm[d]] == -dx[d] and dy[perm[d]] == dy[d] and perm[perm[d]] == d
    # map_fuse.hip derives its own at compile time from a copy of the table: the copy is decode.hip's
    assert R.parse_tables("map_fuse.hip") == (dx, dy)
    src = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", "map_fuse.hip")).read()
    assert "kDx[e] == -kDx[d] && kDy[e] == kDy[d]" in src and "static_assert(perm_is_involution(mirror_perm())" in src
    assert not re.search(r"\{\s*3\s*,\s*4\s*,\s*5\s*,\s*0\s*,\s*1\s*,\s*2\s*,\s*6\s*,\s*7\s*\}", src)      # derived, not copied


# ------------------------------------------------------------------------------------------------ the reference, by hand
def _planes(a):
    """one map [h,w] -> P [9,1,h,w] with plane k = map + k (so the planes are told apart)"""
    a = np.asarray(a, f32)
    return np.stack([a + f32(k) for k in range(9)])[:, None]


def test_identity_size_returns_the_input():
    rng = np.random.default_rng(1)
    P = rng.random((9, 2, 7, 9)).astype(f32)
    assert np.array_equal(R.sample_f32(P, 7, 9).view(np.int32), P.view(np.int32))
    y0, y1, ty = R.axis_taps(7, 7)
    assert y0.tolist() == list(range(7)) and not ty.any()
    out = R.accumulate_f32(P, 7, 9, False, 0.25, True)
    assert np.array_equal(out, f32(0.25) * P)
    out2 = R.accumulate_f32(P, 7, 9, False, 0.75, False, acc=out)
    assert np.array_equal(out2, out + f32(0.75) * P)


def test_double_size_source_gives_the_2x2_box_mean():
    a = np.arange(4 * 6, dtype=f32).reshape(4, 6) * f32(0.125)                # exact in binary
    got = R.sample_f32(_planes(a), 2, 3)
    want = a.reshape(2, 2, 3, 2).mean(axis=(1, 3))
    for k in range(9):
        assert np.array_equal(got[k, 0], want + k)
    y0, y1, ty = R.axis_taps(2, 4)
    assert y0.tolist() == [0, 2] and y1.tolist() == [1, 3] and ty.tolist() == [0.5, 0.5]


def test_half_size_source_gives_quarter_offsets_and_clamps_at_the_edges():
    y0, y1, ty = R.axis_taps(4, 2)
    assert y0.tolist() == [0, 0, 0, 1] and ty.tolist() == [0.0, 0.25, 0.75, 0.0]
    a = np.array([[0.0, 1.0]], f32)                                            # 1 x 2 -> 1 x 4
    got = R.sample_f32(_planes(a), 1, 4)
    assert got[0, 0, 0].tolist() == [0.0, 0.25, 0.75, 1.0]
    assert got[5, 0, 0].tolist() == [5.0, 5.25, 5.75, 6.0]


def test_one_row_or_one_column_sources_clamp():
    for n_out in (1, 3, 8):
        i0, i1, t = R.axis_taps(n_out, 1)
        assert not i0.any() and not i1.any() and not t.any()
    col = np.array([[1.0], [2.0], [4.0]], f32)                                 # ws = 1
    got = R.sample_f32(_planes(col), 3, 5)
    assert np.array_equal(got[0, 0], np.repeat(col, 5, axis=1))
    got = R.sample_f32(_planes(col.T.copy()), 4, 3)                            # hs = 1
    assert np.array_equal(got[0, 0], np.repeat(col.T, 4, axis=0))


def test_a_zero_weight_tap_is_not_used():
    a = np.ones((3, 4), f32)
    a[1, 2] = np.nan
    got = R.sample_f32(_planes(a), 3, 4)                                       # identity: every second tap has weight 0
    assert np.argwhere(np.isnan(got[0, 0])).tolist() == [[1, 2]]
    # 1/2 x source: rows 1..4 sample source row 1 (s = 0.25, 0.75, 1.25, 1.75), columns 3..6 source column 2
    got = R.sample_f32(_planes(a), 6, 8)
    nan = np.isnan(got[3, 0])
    assert nan[1:5, 3:7].all() and nan.sum() == 16


def test_flip_reads_mirrored_columns_and_paired_planes():
    perm = R.decode_perm()
    rng = np.random.default_rng(2)
    P = rng.random((9, 1, 4, 6)).astype(f32)
    mirrored = P[R.plane_order(True, perm)][..., ::-1]                         # what the mirrored image's pass would give
    # the flipped pass reads the same logical taps with the same weights: bit-equal at every size
    for hf, wf in ((4, 6), (7, 9), (2, 3), (1, 1)):
        got = R.sample_f32(mirrored, hf, wf, flip=True, perm=perm)
        assert np.array_equal(got.view(np.int32), R.sample_f32(P, hf, wf).view(np.int32)), (hf, wf)
    assert not np.array_equal(R.sample_f32(mirrored, 4, 6, flip=False), P)     # ... and the flag matters


def test_float64_version_agrees_within_its_bound():
    rng = np.random.default_rng(3)
    perm = R.decode_perm()
    px = rng.normal(0, 3, (2, 5, 7, 2)).astype(f32)
    lk = rng.normal(0, 3, (2, 5, 7, 16)).astype(f32)
    sm = lambda x: np.exp(x.astype(np.float64) - x.max(-1, keepdims=True))
    pp = (sm(px) / sm(px).sum(-1, keepdims=True)).astype(f32)
    lp = np.stack([(sm(lk[..., 2 * d:2 * d + 2]) / sm(lk[..., 2 * d:2 * d + 2]).sum(-1, keepdims=True)) for d in range(8)]).astype(f32)
    gap = float(max(np.abs(px[..., 0] - px[..., 1]).max(), np.abs(lk[..., 0::2] - lk[..., 1::2]).max()))
    for flip in (False, True):
        a32 = R.accumulate_f32(R.stack_probs(pp, lp), 8, 12, flip, 0.25, True, perm=perm)
        a64 = R.accumulate_f64(px, lk, 8, 12, flip, 0.25, True, perm=perm)
        assert np.abs(a32 - a64).max() <= R.f64_bound(gap, 5, 7, 1)


# ------------------------------------------------------------------------------------------------ sizes, options, flags
def test_map_scale_sizes():
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    assert P.map_scale_sizes(768, 1280, [0.5, 1, 2]) == [(384, 640), (768, 1280), (1536, 2560)]
    assert P.map_scale_sizes(128, 128, [0.5, 1, 2]) == [(64, 64), (128, 128), (256, 256)]
    assert P.map_scale_sizes(768, 1280, [0.75]) == [(576, 960)]
    assert P.map_scale_sizes(720, 1280, [1]) == [(736, 1280)]                  # 22.5 rounds half up
    assert P.map_scale_sizes(64, 64, [0.1, 0.7, 1.3]) == [(32, 32), (32, 32), (96, 96)]      # never below 32
    for s, side in ((0.3, 768), (1.7, 100), (2.0, 36)):
        want = max(32, int(np.floor(side * s / 32 + 0.5)) * 32)
        assert P.map_scale_sizes(side, side, [s]) == [(want, want)] and want % 32 == 0
    for bad in ([], [0], [-1], [float("nan")], [float("inf")], [1] * 9, 3):
        with pytest.raises(ValueError):
            P.map_scale_sizes(768, 1280, bad)
    assert P.pass_weights([1, 1]) == [0.5, 0.5] and P.pass_weights([1, 3], flip=True) == [0.125, 0.125, 0.375, 0.375]
    w = P.pass_weights([1, 1, 1])
    assert w == [float(np.float32(1.0 / 3.0))] * 3
    assert P.parse_map_scales("0.5,1,2") == [0.5, 1.0, 2.0]
    with pytest.raises(ValueError):
        P.parse_map_scales("0.5,x")


def test_fuse_score_maps_checks_its_weights_before_anything_runs():
    from tensorflow_ocr_amd.tool import pixellink_fn as P

    class NoGraph:
        device = "cpu"
    for bad in ([], [0.0], [1.0, float("nan")], [-1.0]):
        with pytest.raises(ValueError, match="weights"):
            P.fuse_score_maps(iter(()), bad, (4, 4), graph=NoGraph())
    with pytest.raises(ValueError, match="0 forward passes for 2 weights"):
        P.fuse_score_maps(iter(()), [1.0, 1.0], (4, 4), graph=NoGraph())


def test_link_evaluator_checks_the_options(tmp_path):
    from tensorflow_ocr_amd import evaluate
    d = str(tmp_path)
    with pytest.raises(ValueError, match="RBOX geometry only"):              # as before this option existed
        evaluate.LinkEvaluator(None, None, d, scales=[0.5, 1])
    with pytest.raises(ValueError, match="RBOX geometry only"):
        evaluate.LinkEvaluator(None, None, d, scales=[1], map_scales=[1])
    for kw in (dict(map_scales=[]), dict(map_scales=[0]), dict(map_scales=[1, -2]), dict(map_scales=[float("nan")]),
               dict(map_scales=[float("inf")]), dict(map_scales=[1] * 9), dict(map_scales=[1, 2], scale_weights=[1]),
               dict(map_scales=[1, 2], scale_weights=[1, 0]), dict(map_scales=[1], scale_weights=[float("inf")]),
               dict(scale_weights=[1]), dict(flip=True, scale_weights=[1, 1])):
        with pytest.raises(ValueError):
            evaluate.LinkEvaluator(None, None, d, **kw)
    for kw in (dict(map_scales=[0.5, 1, 2], flip=True, scale_weights=[1, 2, 1]), dict(flip=True), dict(map_scales=[2]),
               dict(map_scales=[1] * 8), dict()):
        with pytest.raises(FileNotFoundError):                                  # good options get as far as the empty directory
            evaluate.LinkEvaluator(None, None, d, **kw)


def test_scripts_take_the_new_flags(capsys):
    sys.path.insert(0, ROOT)
    ev = importlib.import_module("eval_pixellink_fast")
    F = ev.parse([])
    assert F.map_scales is None and F.flip is False
    F = ev.parse(["--map_scales", "0.5,1,2", "--flip"])
    assert F.map_scales == [0.5, 1.0, 2.0] and F.flip is True
    assert ev.parse(["--flip"]).map_scales is None
    for argv in (["--map_scales", "0"], ["--map_scales", "x"], ["--map_scales", ",".join(["1"] * 9)], ["--map_scales", ""]):
        with pytest.raises(SystemExit):
            ev.parse(argv)
    tr = importlib.import_module("train_pixellink")
    F = tr.parse([])
    assert F.eval_map_scales is None and F.eval_flip is False
    on = ["--eval_data_path", "/x", "--eval_steps", "10", "--using_moving_average"]
    F = tr.parse(on + ["--eval_map_scales", "0.5,1,2", "--eval_flip"])
    assert F.eval_map_scales == [0.5, 1.0, 2.0] and F.eval_flip is True
    for argv in (["--eval_map_scales", "1,2"], ["--eval_flip"], on + ["--eval_map_scales", "-1"],
                 ["--eval_data_path", "/x", "--eval_flip"]):
        with pytest.raises(SystemExit):
            tr.parse(argv)
    capsys.readouterr()
    # test_pixellink_fast.py has no such flag: it is the reference's script
    src = open(os.path.join(ROOT, "test_pixellink_fast.py")).read()
    assert "map_scales" not in src and "--flip" not in src


def test_train_eval_signature_is_unchanged_and_passes_the_options_on():
    import inspect
    from tensorflow_ocr_amd import evaluate
    assert list(inspect.signature(evaluate.TrainEval.__init__).parameters) == [
        "self", "graph", "step", "network", "data", "every", "max_images", "weights", "batch_size", "evaluator", "sweep",
        "scales", "fuse", "max_pool", "evaluator_kw"]
    seen = {}

    class Probe:
        def __init__(self, graph, forward, data, **kw):
            seen.update(kw)
    evaluate.TrainEval(None, None, None, "/x", 5, evaluator=Probe, map_scales=[0.5, 1], flip=True)
    assert seen["map_scales"] == [0.5, 1] and seen["flip"] is True and "scales" not in seen
    params = inspect.signature(evaluate.LinkEvaluator.__init__).parameters
    assert [params[k].default for k in ("map_scales", "flip", "scale_weights")] == [None, False, None]


def test_ops_binding_checks_shapes_and_dtypes():
    import torch
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    for name in ("map_scale_sizes", "fuse_score_maps", "detect_device_multiscale"):
        assert callable(getattr(P, name, None)), name
    F = torch.float32
    z = lambda *s, dt=F: torch.zeros(s, dtype=dt)
    ok = dict(pixel_logits=z(2, 4, 6, 2), link_logits=z(2, 4, 6, 16), flip=False, weight=0.5, first=True, acc=z(9, 2, 7, 9))
    for kw in (dict(pixel_logits=z(2, 4, 6, 1)), dict(link_logits=z(2, 4, 6, 8)), dict(link_logits=z(2, 4, 5, 16)),
               dict(acc=z(8, 2, 7, 9)), dict(acc=z(9, 3, 7, 9)), dict(acc=z(9, 2, 7)), dict(pixel_logits=z(2, 4, 6, 2, dt=torch.float16)),
               dict(acc=z(9, 2, 7, 9, dt=torch.float64)), dict(link_logits=z(2, 4, 16, 6).transpose(2, 3)), dict(weight=0.0),
               dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-1.0)):
        with pytest.raises(ValueError, match="link_map_accumulate"):
            ops.link_map_accumulate(**dict(ok, **kw))
