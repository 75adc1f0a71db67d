"""Host half of tests/test_gpu_nms_matrix.py, no device: the rows of its table against the extern "C" entries of
csrc/lanms.hip, csrc/iou.hip, csrc/resize.hip and the fusion entries of csrc/multiscale.hip, the constants its rows are named
after against the sources, and — with the oracle alone — that every row's inputs have the pattern the row promises: a row
whose quads do not reach its edge fails here, not silently on the GPU."""
import os
import re

import numpy as np
import pytest

from oracle import lanms as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def M():
    import test_gpu_nms_matrix as M
    return M


def _images(M, kind):
    """(row name, thr, image, oracle merged, oracle keep) of every ocr_lanms image of one kind, counts above max_k clamped"""
    for name in M.LANMS_ROWS:
        row, want = M.lanms_oracle(name)
        for im, (om, ok) in zip(row["images"], want):
            if im.kind == kind:
                yield name, row["thr"], im, om, ok


def test_every_entry_is_named_by_a_row(M):
    entries = set()
    for f in ("lanms.hip", "iou.hip", "resize.hip"):
        entries |= set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', _read("tensorflow_ocr_amd", "csrc", f)))
    assert entries == {"ocr_lanms", "ocr_lanms_workspace", "ocr_quad_iou", "ocr_resize_linear_u8", "ocr_resize_cubic_f32"}
    entries |= {"ocr_quad_fuse", "ocr_quad_fuse_workspace"}
    assert entries <= set(re.findall(r"\b(ocr_\w+)\(", _read("include", "ocr_hip.h") + _read("include", "ocr_multiscale.h")))
    named = {e for r in M.ROWS.values() for e in r.entries}
    assert named == entries, sorted(entries ^ named)
    test = _read("tests", "test_gpu_nms_matrix.py")
    assert all('"%s"' % e in test for e in entries), "an entry that no test calls by name"


def test_the_constants_the_rows_are_named_after_are_the_sources(M):
    common, lanms, multi, iou = [_read("tensorflow_ocr_amd", "csrc", f) for f in ("common.h", "lanms.hip", "multiscale.hip", "iou.hip")]
    header = _read("include", "ocr_hip.h")
    # OCR_CHECK_SHAPE returns OCR_ERR_UNSUPPORTED = -2, the status of the max_k = 32769 row
    assert re.search(r"#define OCR_CHECK_SHAPE\(cond\)[^#]*?return OCR_ERR_UNSUPPORTED;", common, re.S)
    assert re.search(r"OCR_ERR_UNSUPPORTED = (-?\d+)", header).group(1) == str(M.SHAPE_REFUSAL)
    assert "OCR_CHECK_SHAPE(max_k <= 64 * 64 * 8)" in lanms and 64 * 64 * 8 == 32768
    # the two path switches: 73 bytes per quad against 144 KB, one mask word per lane against 64 lanes
    assert "stage_bytes <= 144 * 1024" in lanms and "(size_t)max_k * 9 * sizeof(float) * 2 + (size_t)max_k" in lanms
    assert 2019 * 73 <= 144 * 1024 < 2020 * 73
    assert "words <= 64 ? lanms_sweep64_kernel : lanms_sweep_kernel" in lanms and (4096 + 63) // 64 == 64 < (4097 + 63) // 64
    assert M.PATH_MAX_K == (2019, 2020, 4096, 4097)
    assert "s_score[2048]" in lanms and "s_keep[4096]" in lanms
    assert "constexpr int kMaxPool = 4096;" in multi and "constexpr int kMaxV = 8;" in iou
    assert "nd <= 65535 && mask_h <= 32768 && mask_w <= 32768" in iou
    # the header says what the rows pin
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*size_t ocr_lanms_workspace", header, re.S).group(1)
    for word in ("clamped", "2019", "2020", "4096", "4097", "32768", "OCR_ERR_WORKSPACE"):
        assert word in doc, word


def test_rows_are_the_ones_the_matrix_names(M):
    names = list(M.ROWS)
    for k in M.PATH_MAX_K:
        row, want = M.lanms_oracle("lanms/path/%d" % k)
        assert row["max_k"] == k and len(row["images"][0].q) == k and abs(len(row["images"][1].q) - k / 3) < 1
        assert len(want[1][0]) < len(row["images"][1].q) and len(want[1][1]) < len(want[1][0])   # the clustered image merges and suppresses
    for thr in M.THRS:
        for part in (0, 1):
            for s in list(M.VERDICT_SETS) + [None]:
                assert ("lanms/verdict/%s/thr%g/%d" % (s, thr, part) if s else "lanms/rejoin/thr%g/%d" % (thr, part)) in names
        assert "lanms/runs/thr%g" % thr in names
    ks = sorted({len(im.q) for _, _, im, _, _ in _images(M, "verdict")} - {330})
    assert tuple(ks) == M.VERDICT_K == (66, 130, 200)
    assert M.VERDICT_SETS["edges"](200) == {0, 62, 63, 64, 127, 128, 198}
    assert all("lanms/rank/%d" % m in names for m in (2047, 2048, 2049, 2100))
    assert sorted(M.INTERLEAVED) == [64, 65, 128, 129, 4096]
    assert {n for n in names if n.startswith("fuse/")} == {"fuse/%d/mode%d" % (p, m) for p in (64, 65, 4096) for m in (0, 1)}
    assert {n for n in names if n.startswith("iou/")} == {"iou/v%d/%dx%d" % (v, h, w) for v in (3, 4, 5, 8) for h, w in ((40, 56), (300, 520))}
    assert M.IOU_GRIDS == ((1, 1), (1, 7), (5, 1), (6, 4)) and M.LINEAR_CN == (1, 3, 4) and M.CUBIC_PLANES == (1, 3)
    assert sorted(M.LINEAR_SHAPES.values()) == sorted([(37, 53, 37, 53), (36, 52, 18, 26), (37, 53, 64, 64), (50, 70, 1, 70), (50, 70, 50, 1),
                                                       (1, 9, 5, 20), (9, 1, 20, 5), (3, 3, 97, 131)])
    assert M.CUBIC_SHAPES == ((4, 5, 13, 17), (32, 32, 128, 128), (45, 80, 5, 9), (1, 1, 3, 3), (7, 9, 7, 9))
    assert M.CUBIC_SCALES == ((1.0, 1.0), (255.0, 1.0), (1.0, 255.0))
    # ragged counts with a 0 and a 1 in the batches, finite coordinates, scores in (0, 1]
    counts = set()
    for name in M.LANMS_ROWS:
        row = M.ROWS[name].build() if name not in M._ORACLE else M._ORACLE[name][0]
        assert 2 <= len(row["images"]) <= 3, name
        counts |= {len(im.q) for im in row["images"]}
        for im in row["images"]:
            assert np.isfinite(im.q).all() and (im.q[:, 8] > 0).all() and (im.q[:, 8] <= 1).all(), name
    assert {0, 1} <= counts


def test_verdict_rows_merge_exactly_where_they_say(M):
    seen = set()
    for name, thr, im, om, ok in _images(M, "verdict"):
        k = len(im.q)
        got = {i for i in range(k - 1) if OL.iou(im.q[i + 1], im.q[i]) > thr}
        assert got == im.hits, name
        seen.add((k, tuple(sorted(im.hits))))
    for k in M.VERDICT_K:
        for s in M.VERDICT_SETS.values():
            assert (k, tuple(sorted(i for i in s(k) if i <= k - 2))) in seen
        assert (k, ()) in seen and (k, tuple(range(k - 1))) in seen and (k, (k - 2,)) in seen
    # the runs row: from the quad behind each merge, exactly 63, 64, 65 and 128 verdicts without a hit
    assert (330, M.RUN_HITS) in seen
    starts = [0] + [h + 2 for h in M.RUN_HITS[:-1]]
    assert [h - s for h, s in zip(M.RUN_HITS, starts)] == [63, 64, 65, 128]


def test_rejoin_rows_restart_behind_a_merged_quad(M):
    n = 0
    for name, thr, im, om, ok in _images(M, "rejoin"):
        k = len(im.q)
        assert len(om) == im.n_merged, name
        for g in range(k // 4):
            a, b, c, d = im.q[4 * g:4 * g + 4]
            assert OL.iou(b, a) > thr and OL.iou(c, b) > thr and OL.iou(d, c) > thr      # all three input verdicts are 1
            ab = om[2 * g]
            assert ab[8] == a[8] + b[8] and a[0] < ab[0] < b[0]                          # a + b merged
            assert not OL.iou(c, ab) > thr                                               # which c does not join,
            assert om[2 * g + 1][8] == c[8] + d[8]                                       # but d joins c
            n += 1
    assert n == 2 * (16 + 32 + 50)


def test_interleaved_rows_merge_nothing_and_keep_one_quad_per_cluster(M):
    seen = set()
    for name, thr, im, om, ok in _images(M, "interleaved"):
        k = min(len(im.q), M._ORACLE[name][0]["max_k"])
        assert len(om) == k and len(ok) == min(im.c, k), name
        seen.add(k)
    assert seen >= {64, 65, 128, 129, 4096}
    for name in (n for n in M.ROWS if n.startswith("fuse/")):
        row, want = M.fuse_oracle(name)
        for im, (_, keep, owner) in zip(row["images"], want):
            if im.kind == "interleaved":
                assert len(keep) == im.c and sorted(set(owner.tolist())) == sorted(keep.tolist())


def test_pos63_rows_put_the_leader_at_sorted_position_63(M):
    n = 0
    for kind, pos in (("pos63", 63), ("last", 0)):
        for name, thr, im, om, ok in _images(M, kind):
            m = len(im.q)
            assert len(om) == m and np.array_equal(om, im.q)                # nothing merges: merged index == input index
            order = np.argsort(-om[:, 8], kind="stable")
            assert order[pos] == im.leader
            want = {64, m - 1} if kind == "pos63" else {m - 1}
            assert {int(np.nonzero(order == v)[0][0]) for v in im.victims} == want
            assert sorted(set(range(m)) - set(ok.tolist())) == sorted(im.victims) and im.leader in ok
            n += 1
    assert n == 2 * len(M.POS63_M) + 1
    for name in ("fuse/65/mode0", "fuse/4096/mode1"):
        row, want = M.fuse_oracle(name)
        im, (_, keep, owner) = row["images"][1], want[1]
        assert im.kind == "pos63" and list(keep).index(im.leader) == 63
        assert all(owner[v] == im.leader for v in im.victims) and len(keep) == len(im.q) - len(im.victims)


def test_far_apart_rows_keep_everything_and_rank_rows_tie_across_2048(M):
    sizes = set()
    for name, thr, im, om, ok in _images(M, "far"):
        k = len(im.q)
        assert len(om) == k and len(ok) == k, name
        assert np.array_equal(ok, np.argsort(-im.q[:, 8], kind="stable")), name
        sizes.add(k)
        if name.startswith("lanms/rank/") and k > 1:
            assert set(np.unique(im.q[:, 8]).tolist()) == {0.5, 0.75}
            for p in (2047, 2048):
                assert p >= k or im.q[p, 8] == im.forced
    assert sizes >= {1, 2019, 2020, 4096, 4097, 2047, 2048, 2049, 2100}
    forced = {(len(im.q), float(im.forced)) for name, _, im, _, _ in _images(M, "far") if name.startswith("lanms/rank/") and len(im.q) > 1}
    assert forced == {(m, v) for m in M.RANK_M for v in (0.5, 0.75)}


def test_clamp_rows_ask_for_more_than_the_buffers_hold(M):
    for name, over in (("lanms/clamp/130", [7, 130]), ("lanms/clamp/2100", [7, 2100])):
        row, want = M.lanms_oracle(name)
        assert [c - row["max_k"] for c in row["counts"][:2]] == over
        assert all(len(im.q) == row["max_k"] for im in row["images"][:2])
        assert all(0 < len(ok) <= len(om) <= row["max_k"] for om, ok in want)


def test_iou_rows_hold_the_polygons_they_promise(M):
    row = M.ROWS["iou/v5/300x520"].build()
    assert [(len(d), len(g)) for d, g in row["grids"][:4]] == list(M.IOU_GRIDS)
    allp = np.concatenate([np.concatenate([d, g]) for d, g in row["grids"][:4]])
    assert allp.min() >= -12 and allp.max() < 520 + 12 and allp.min() < 0 and allp.max() > 520
    assert any((p[:, 1] == p[0, 1]).all() for p in allp) and any((p[0] == p[1]).all() for p in allp)
    dets, gts = row["grids"][4]
    fixed = dict(zip(row["fixed"], zip(dets, gts)))
    for k in ("left of the mask", "above the mask"):
        assert all(p[:, 0].max() < -1 or p[:, 1].max() < -1 for p in fixed[k])
    both = np.concatenate(fixed["whole mask"])
    assert both.min(0).tolist() == [0, 0] and both.max(0).tolist() == [519, 299]
    small = np.concatenate(fixed["3x3 box"])
    assert (small.max(0) - small.min(0)).tolist() == [2, 2]
    assert np.array_equal(*fixed["identical"])
    inter, uni = M.iou_ref(dets, gts, 300, 520)
    assert inter[0, 0] == uni[0, 0] == inter[1, 1] == uni[1, 1] == 0 and inter[4, 4] == uni[4, 4] > 0
