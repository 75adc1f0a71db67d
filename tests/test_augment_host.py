"""CPU: the host side of the device augmentation — the C ABI's declarations, the policy's text form, crop_area's
guarantees, plan()'s determinism and the accuracy of its fixed-point inverse map.  (The warp itself runs on the device:
tests/test_gpu_augment.py.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout(rng, n, h, w):
    """n axis-aligned boxes (clockwise from the top-left, as validated polygons are), float32 [n,4,2]."""
    out = []
    for _ in range(n):
        x0, y0 = rng.randint(0, w - 12), rng.randint(0, h - 12)
        x1, y1 = x0 + rng.randint(4, 12), y0 + rng.randint(4, 12)
        out.append([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    return np.array(out, np.float32).reshape(-1, 4, 2)


def test_header_declares_the_entry_point_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ocr_augment_u8_batch" in set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    m = re.search(r"typedef struct \{([^}]*)\}\s*ocr_augment_desc;", code)
    assert m
    fields = re.findall(r"\b(int64_t|int32_t|float)\s+([^;]+);", m.group(1))
    assert fields == [("int64_t", "src_off"), ("int32_t", "H, W"), ("int64_t", "A[6]"), ("float", "col[3][4]")]
    from tensorflow_ocr_amd.datasets.augment import DESC_DTYPE
    assert DESC_DTYPE.itemsize == 8 + 4 + 4 + 6 * 8 + 12 * 4
    assert [DESC_DTYPE.fields[k][1] for k in ("src_off", "H", "W", "A", "col")] == [0, 8, 12, 16, 64]
    from tensorflow_ocr_amd import _lib
    assert _lib.ABI_VERSION == 7


def test_the_policy_module_does_not_import_torch():
    code = ("import sys; import tensorflow_ocr_amd.datasets.augment as a; "
            "assert 'torch' not in sys.modules, 'torch imported'; print(a.Augment.parse('east').spec())")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "random_scale=0.5:1.0:2.0:3.0" in out.stdout


def test_parse_presets_round_trip():
    from tensorflow_ocr_amd.datasets.augment import Augment
    assert Augment.parse("none") is None and Augment.parse(None) is None and Augment.parse("") is None
    east = Augment.parse("east")
    assert east == Augment()
    assert (east.random_scale, east.crop, east.min_crop_side_ratio, east.background_ratio) == ((0.5, 1.0, 2.0, 3.0), True, 0.1, 0.375)
    assert (east.rotate90_prob, east.max_rotate_deg, east.brightness, east.contrast, east.saturation) == (0, 0, 0, 0, 0)
    pl = Augment.parse("pixellink")
    assert pl == Augment(rotate90_prob=0.2, brightness=32 / 255, contrast=0.5, saturation=0.5) and pl != east
    for a in (east, pl, Augment(random_scale=(1,), crop=False, max_rotate_deg=7.5)):
        again = Augment.parse(a.spec())
        assert again == a and again.spec() == a.spec()
    kv = Augment.parse("random_scale=1:1.5, crop=false, background_ratio=1/4, max_rotate_deg=10")
    assert kv.random_scale == (1.0, 1.5) and kv.crop is False and kv.background_ratio == 0.25 and kv.max_rotate_deg == 10.0
    assert Augment.parse("pixellink,rotate90_prob=0.5").rotate90_prob == 0.5
    for bad in ("west", "east,foo=1", "crop=maybe", "brightness=-1", "rotate90_prob=2", "random_scale=0:1", "east,crop"):
        with pytest.raises(ValueError):
            Augment.parse(bad)


def test_scripts_parse_the_augment_flag():
    import importlib
    from tensorflow_ocr_amd.datasets.augment import Augment
    mod = importlib.import_module("multigpu_train")
    assert mod.parse([]).augment is None and mod.parse(["--augment", "none"]).augment is None
    assert mod.parse(["--augment", "pixellink"]).augment == Augment.parse("pixellink")
    assert mod.parse(["--augment", "crop=false,max_rotate_deg=5"]).augment.max_rotate_deg == 5.0
    with pytest.raises(SystemExit):
        mod.parse(["--augment", "west"])


def test_crop_area_never_cuts_a_kept_polygon_and_keeps_the_minimum_side():
    from tensorflow_ocr_amd.datasets.augment import crop_area
    seen_crop = 0
    for seed in range(300):
        rng = np.random.RandomState(seed)
        h, w = int(rng.randint(40, 200)), int(rng.randint(40, 200))
        polys = _layout(rng, int(rng.randint(1, 5)), h, w)
        tags = rng.rand(len(polys)) < 0.3
        ratio = (0.1, 0.3)[seed % 2]
        xmin, ymin, xmax, ymax, kept, ktags = crop_area((h, w), polys, tags, rng, min_crop_side_ratio=ratio)
        assert 0 <= xmin <= xmax <= w - 1 and 0 <= ymin <= ymax <= h - 1
        assert len(kept) == len(ktags)
        if (xmin, ymin, xmax, ymax) == (0, 0, w - 1, h - 1):
            continue                                            # the fall-back: everything kept, nothing moved
        seen_crop += 1
        assert xmax - xmin >= ratio * w and ymax - ymin >= ratio * h
        assert len(kept) >= 1                                   # a text crop holds text
        assert kept[:, :, 0].min() >= 0 and kept[:, :, 0].max() <= xmax - xmin
        assert kept[:, :, 1].min() >= 0 and kept[:, :, 1].max() <= ymax - ymin
        # the kept ones are exactly the source polygons with all four vertices inside, shifted
        inside = ((polys[:, :, 0] >= xmin) & (polys[:, :, 0] <= xmax) & (polys[:, :, 1] >= ymin) & (polys[:, :, 1] <= ymax)).all(axis=1)
        assert np.array_equal(kept, polys[inside] - np.array([xmin, ymin], np.float32))
        assert np.array_equal(ktags, tags[inside])
    assert seen_crop > 200


def test_crop_area_without_a_free_row_or_column_returns_the_whole_image():
    from tensorflow_ocr_amd.datasets.augment import crop_area
    h, w = 50, 80
    # the projection arrays are padded by h//10, w//10 on both sides; a polygon whose rounded extent covers
    # [-pad, size+pad) leaves no free position on that axis
    wide = np.array([[[-8, 10], [88, 10], [88, 20], [-8, 20]]], np.float32)
    tall = np.array([[[10, -5], [20, -5], [20, 55], [10, 55]]], np.float32)
    for polys in (wide, tall):
        for seed in range(20):
            rng = np.random.RandomState(seed)
            state = rng.get_state()[1].copy()
            got = crop_area((h, w), polys, np.array([False]), rng)
            assert got[:4] == (0, 0, w - 1, h - 1) and got[4] is polys
            assert np.array_equal(rng.get_state()[1], state)   # and nothing was drawn


def test_crop_area_background_mode_returns_zero_polygons():
    from tensorflow_ocr_amd.datasets.augment import crop_area
    found = 0
    for seed in range(300):
        rng = np.random.RandomState(1000 + seed)
        h, w = int(rng.randint(60, 200)), int(rng.randint(60, 200))
        polys = _layout(rng, int(rng.randint(1, 4)), h, w)
        tags = np.zeros(len(polys), bool)
        xmin, ymin, xmax, ymax, kept, ktags = crop_area((h, w), polys, tags, rng, crop_background=True)
        if len(kept) == 0:
            found += 1
            assert kept.shape == (0, 4, 2) and ktags.shape == (0,)
            assert xmax - xmin >= 0.1 * w and ymax - ymin >= 0.1 * h
            inside = ((polys[:, :, 0] >= xmin) & (polys[:, :, 0] <= xmax) & (polys[:, :, 1] >= ymin) & (polys[:, :, 1] <= ymax)).all(axis=1)
            assert not inside.any()
        else:             # icdar.py:186-197: a try that holds text returns as a text crop (the caller then skips the sample)
            assert kept[:, :, 0].min() >= 0 and kept[:, :, 0].max() <= xmax - xmin
            assert kept[:, :, 1].min() >= 0 and kept[:, :, 1].max() <= ymax - ymin
    assert found > 150
    # and through plan(): a background draw yields zero polygons or no sample at all
    from tensorflow_ocr_amd.datasets.augment import Augment
    aug = Augment(background_ratio=1.0)
    rng, lay = np.random.RandomState(5), np.random.RandomState(6)
    plans = [aug.plan(rng, 120, 150, _layout(lay, 2, 120, 150), np.zeros(2, bool), 64) for _ in range(200)]
    assert all(p is None or (p[2].shape == (0, 4, 2) and p[3].shape == (0,)) for p in plans)
    assert sum(p is not None for p in plans) > 50 and any(p is None for p in plans)


def test_plan_is_deterministic_per_seed_and_skips_like_the_reference():
    from tensorflow_ocr_amd.datasets.augment import Augment
    aug = Augment.parse("pixellink,max_rotate_deg=10")
    lay = np.random.RandomState(7)
    h, w, S = 90, 160, 64
    polys = _layout(lay, 3, h, w)
    tags = np.array([False, True, False])
    outs, skipped, background = [], 0, 0
    for rep in range(2):
        rng = np.random.RandomState(42)
        out = [aug.plan(rng, h, w, polys.copy(), tags.copy(), S) for _ in range(200)]
        outs.append(out)
    for a, b in zip(*outs):
        assert (a is None) == (b is None)
        if a is None:
            skipped += 1
            continue
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        A, col, pp, tt = a
        assert A.dtype == np.int64 and A.shape == (6,) and col.dtype == np.float32 and col.shape == (3, 4)
        assert pp.dtype == np.float32 and pp.shape[1:] == (4, 2) and tt.dtype == bool and tt.shape == (len(pp),)
        background += len(pp) == 0
    assert 0 < skipped < 400 and background > 0
    other = [aug.plan(np.random.RandomState(43), h, w, polys, tags, S) for _ in range(1)][0]
    first = outs[0][0]
    assert other is None or first is None or not np.array_equal(other[0], first[0]) or not np.array_equal(other[1], first[1])
    # the inputs are left alone
    assert np.array_equal(polys, _layout(np.random.RandomState(7), 3, h, w))


@pytest.mark.parametrize("spec", ["east", "pixellink", "pixellink,max_rotate_deg=15", "random_scale=1:1.5,crop=false,rotate90_prob=1"])
def test_fixed_point_inverse_returns_the_planned_vertices_to_their_source(spec):
    """A applied to a transformed vertex lands within 2^-5 source pixel (the kernel's coordinate quantum) of the original.
    The budget: A is rounded to 2^-17 per entry and multiplies coordinates below 2^9 (|error| < 2^-7), the planned
    vertices are rounded to float32 (relative 2^-24, times a zoom-out of at most 12 here): well inside 2^-5."""
    from tensorflow_ocr_amd.datasets.augment import Augment, apply_fixed
    aug = Augment.parse(spec)
    checked = 0
    for seed in range(120):
        lay = np.random.RandomState(500 + seed)
        h, w = int(lay.randint(60, 400)), int(lay.randint(60, 400))
        S = (64, 320, 512)[seed % 3]
        polys = _layout(lay, 4, h, w)
        tags = np.zeros(4, bool)
        plan = aug.plan(np.random.RandomState(seed), h, w, polys, tags, S)
        if plan is None or len(plan[2]) == 0:
            continue
        A, _, pp, _ = plan
        back = apply_fixed(A, pp.astype(np.float64))            # [k,4,2] source positions
        # every planned polygon is one of the source polygons (crop and rotation drop some, never reorder vertices)
        for q in back:
            d = np.abs(polys.astype(np.float64) - q).max(axis=(1, 2))
            assert d.min() <= 2.0 ** -5, (seed, d.min())
            checked += 1
    assert checked > 40


def test_identity_policy_gives_the_identity_map_and_colour_matrix_exactly():
    from tensorflow_ocr_amd.datasets.augment import Augment, colour_matrix
    aug = Augment(random_scale=(1,), crop=False)
    polys = np.array([[[3, 4], [40, 4], [40, 20], [3, 20]]], np.float32)
    for S in (64, 512):
        A, col, pp, tt = aug.plan(np.random.RandomState(0), S, S, polys, np.array([True]), S)
        assert A.tolist() == [65536, 0, 0, 0, 65536, 0]
        assert col.tobytes() == np.eye(3, 4, dtype=np.float32).tobytes()
        assert np.array_equal(pp, polys) and tt.tolist() == [True]
    assert colour_matrix().tobytes() == np.eye(3, 4, dtype=np.float32).tobytes()
    # a plain stretch (what the un-augmented path does) in the same terms: 1280 x 720 -> 512 x 512 pads to 1280 first
    A, _, pp, _ = aug.plan(np.random.RandomState(0), 720, 1280, polys, np.array([False]), 512)
    assert A.tolist() == [163840, 0, 49152, 0, 163840, 49152]   # 2.5 in 16.16; 2.5*0.5 - 0.5 = 0.75


def test_rot90_fixed_is_a_pixel_permutation():
    from tensorflow_ocr_amd.datasets.augment import rot90_fixed
    S = 7
    A = np.array([65536 * 2 + 17, -33, 1000, 45, 65536 - 5, -70000], np.int64)
    dy, dx = np.mgrid[0:S, 0:S]

    def coords(a):
        return np.stack([a[0] * dx + a[1] * dy + a[2], a[3] * dx + a[4] * dy + a[5]], -1)
    base = coords(A)
    for k in range(5):
        assert np.array_equal(coords(rot90_fixed(A, S, k)), np.rot90(base, k))


def test_pack_desc_refuses_an_image_outside_the_slab():
    from tensorflow_ocr_amd.datasets.augment import DESC_DTYPE, pack_desc
    plan = (np.array([65536, 0, 0, 0, 65536, 0], np.int64), np.eye(3, 4, dtype=np.float32))
    d = pack_desc([0, 30], [(2, 5, 3), (3, 3, 3)], [plan, plan], 57)
    assert d.dtype == DESC_DTYPE and d["src_off"].tolist() == [0, 30] and d["H"].tolist() == [2, 3] and d["W"].tolist() == [5, 3]
    assert d["A"][1].tolist() == plan[0].tolist() and np.array_equal(d["col"][0], plan[1])
    for offs, shapes, nbytes in (([0, 30], [(2, 5, 3), (3, 3, 3)], 56), ([-1], [(2, 5, 3)], 100), ([0], [(2, 5, 4)], 100),
                                 ([0], [(0, 5, 3)], 100)):
        with pytest.raises(ValueError):
            pack_desc(offs, shapes, [plan] * len(offs), nbytes)


def test_load_sample_leaves_the_polygons_in_source_pixels_on_request(tmp_path):
    from tensorflow_ocr_amd.datasets import _decode
    im = np.zeros((40, 80, 3), np.uint8)
    np.save(os.path.join(tmp_path, "a.npy"), im)
    with open(os.path.join(tmp_path, "gt_a.txt"), "w") as f:
        f.write("10,5,30,5,30,15,10,15,word\n")
    fn = os.path.join(str(tmp_path), "a.npy")
    scaled = _decode.load_sample((fn, 160))
    raw = _decode.load_sample((fn, 160, True))
    assert np.array_equal(raw[2][0], np.array([[10, 5], [30, 5], [30, 15], [10, 15]], np.float32))
    assert np.array_equal(scaled[2][0], raw[2][0] * np.array([2, 4], np.float32))
    assert np.array_equal(_decode.load_sample((fn, 160, False))[2], scaled[2])
