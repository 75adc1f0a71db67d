"""Host side of PixelLink's instance-balanced loss (no GPU): the C ABI's declarations, the kernel inventory of the two
pinned loss files, the properties of the reference weight map the GPU tests compare against, and the training script's
flags."""
import os
import re

import numpy as np

import balanced_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ocr_pixellink_instance_weights", "ocr_balanced_loss_workspace", "ocr_balanced_loss_fwd",
           "ocr_balanced_loss_selected", "ocr_balanced_loss_bwd", "ocr_balanced_loss_bwd_dyn"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_entries_at_abi_7():
    from tensorflow_ocr_amd import _lib
    hdr = _read("include", "ocr_hip.h")
    src = _read("tensorflow_ocr_amd", "csrc", "pixellink_balance.hip")
    for s in SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % s, hdr), s
        assert re.search(r'extern "C" (int|size_t) %s\(' % s, src), s
    assert "} ocr_balanced_loss_desc;" in hdr
    assert re.search(r"#define OCR_ABI_VERSION 7\b", hdr) and _lib.ABI_VERSION == 7
    assert "UNPINNED" in hdr[hdr.index("INSTANCE-BALANCED"):hdr.index("ocr_balanced_loss_desc;")]
    # the descriptor of the host layer has the header's fields in the header's order
    assert [n for n, _ in _lib.BalancedLossDesc._fields_] == ["n", "hw", "focal", "neg_ratio", "alpha", "gamma"]


def test_pinned_loss_files_keep_their_inventory():
    """the new file brings its own kernels and entries and shares the per-element helpers through loss_math.h: one
    definition of each"""
    pinned = _read("tensorflow_ocr_amd", "csrc", "loss_softmax.hip") + _read("tensorflow_ocr_amd", "csrc", "loss_dice.hip")
    assert len(re.findall(r"__global__", pinned)) == 17 and len(re.findall(r'extern "C"', pinned)) == 15
    assert "balanced" not in pinned
    new = _read("tensorflow_ocr_amd", "csrc", "pixellink_balance.hip")
    math = _read("tensorflow_ocr_amd", "csrc", "loss_math.h")
    for helper in ("det_exp", "neg_score", "ce2", "focal2", "is_pos", "is_neg"):
        define = r"__device__ __forceinline__ \w+ %s\(" % helper
        assert len(re.findall(define, math)) == 1, helper
        assert not re.search(define, new) and not re.search(define, pinned), helper
    assert '#include "loss_math.h"' in new and '#include "loss_math.h"' in pinned
    assert "asm" not in new


def _scene():
    """two images at 64 x 64 -> 16 x 16: overlapping rectangles, one hidden completely, one ignored, one too small to
    reach a label cell; and an image without polygons"""
    rects = [(4, 4, 40, 30), (20, 16, 59, 50), (44, 52, 50, 58), (42, 50, 56, 60), (0, 40, 12, 60), (17, 57, 18, 58)]
    ignore = np.zeros((2, 6), np.uint8)
    ignore[0, 4] = 1
    cover = np.stack([B.paint_cover(64, 64, rects, ignore[0]), B.paint_cover(64, 64, [])])
    return cover, ignore


def test_reference_weight_map_properties():
    cover, ignore = _scene()
    area, weight, live = B.instance_weights(cover, ignore, 16, 16)
    own = B.owner_map(cover, 16, 16, 6)
    assert area[0].tolist() == [np.sum(own[0] == j + 1) for j in range(6)]
    assert area[0, 2] == 0 and area[0, 5] == 0 and area[0, 4] > 0            # hidden, below one cell, ignored
    assert live[0].tolist() == [True, True, False, True, False, False] and not live[1].any()
    N, S = 3, int(area[0, [0, 1, 3]].sum())
    u = 2.0 ** -24
    for j in (0, 1, 3):
        w = weight[0][own[0] == j + 1].astype(np.float64)
        assert (w == w[0]).all() and w[0] > 0
        # S_j equal terms, each S / (N S_j) rounded once: the sum is S / N within u relative
        assert abs(w.sum() - S / N) <= u * S / N
    assert abs(weight[0].astype(np.float64).sum() - S) <= u * S
    for j in (2, 4, 5):
        assert (weight[0][own[0] == j + 1] == 0).all()
    assert (weight[0][own[0] == 0] == 0).all() and (weight[1] == 0).all() and (area[1] == 0).all()
    # the instance of 1/4 of another's area weighs 4 times as much per cell
    c2 = B.paint_cover(32, 32, [(0, 0, 15, 15), (16, 16, 23, 23)])[None]
    a2, w2, _ = B.instance_weights(c2, np.zeros((1, 2), np.uint8), 32, 32)
    assert a2[0].tolist() == [256, 64] and w2[0, 0, 0] == np.float32(320 / 512) and w2[0, 16, 16] == np.float32(2.5)


def test_reference_mining_count_is_the_double_product():
    assert B.count(10, np.float32(0.7), 100) == 6 and B.count(10, 3.0, 7) == 7 and B.count(0, 3.0, 7) == 0


def test_train_flags():
    import train_pixellink
    F = train_pixellink.parse([])
    assert F.pixel_loss == "mean" and F.max_neg_pos_ratio == 3.0
    F = train_pixellink.parse(["--pixel_loss", "instance_balanced", "--max_neg_pos_ratio", "2.5"])
    assert F.pixel_loss == "instance_balanced" and F.max_neg_pos_ratio == 2.5
    for bad in (["--pixel_loss", "other"], ["--max_neg_pos_ratio", "-1"], ["--max_neg_pos_ratio", "nan"]):
        try:
            train_pixellink.parse(bad)
        except SystemExit:
            continue
        raise AssertionError(bad)


def test_synthetic_ids_are_the_label_owners():
    from tensorflow_ocr_amd import synthetic
    a = synthetic.make_batch(np.random.default_rng(3), 2, 64)
    b = synthetic.make_batch(np.random.default_rng(3), 2, 64, return_ids=True)
    assert len(a) == 4 and len(b) == 5
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    ids = b[4]
    assert ids.dtype == np.int32 and ids.shape == (2, 16, 16) and np.array_equal(ids > 0, b[1][..., 0] > 0)
    # ids * 257 is a cover raster whose owner map is ids itself
    assert np.array_equal(B.owner_map(ids * 257, 16, 16, 8), ids)
