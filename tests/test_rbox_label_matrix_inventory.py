"""Host half of tests/test_gpu_rbox_label_matrix.py, no device: the rows of its table against the extern "C" entries of
csrc/rbox.hip and csrc/labels.hip, the constants its rows are named after against the sources, and — with the oracles
alone — that every row's inputs have the pattern the row promises: a row that does not reach its edge fails here, not
silently on the GPU.  The vectorised restatements the large rows use (decode_vec, icdar_vec, pixellink_vec) are held to
tests/test_rbox_host.decode_ref and oracle/labels.py here, on the small rows."""
import math
import os
import re

import numpy as np
import pytest

import test_rbox_host as H
from oracle import labels as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32 = np.float32, np.float64, np.int32

ENTRIES = {"ocr_rbox_head_fwd", "ocr_rbox_head_bwd", "ocr_rbox_loss_workspace", "ocr_rbox_loss_fwd", "ocr_rbox_loss_bwd",
           "ocr_rbox_loss_bwd_dyn", "ocr_rbox_decode_workspace", "ocr_rbox_decode", "ocr_quad_mean_score", "ocr_poly_cover",
           "ocr_icdar_labels", "ocr_pixellink_labels", "ocr_icdar_rbox_labels"}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def M():
    import test_gpu_rbox_label_matrix as M
    return M


def test_every_entry_is_named_by_a_row(M):
    found = {f: set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', _read("tensorflow_ocr_amd", "csrc", f))) for f in ("rbox.hip", "labels.hip")}
    assert len(found["rbox.hip"]) == 9 and len(found["labels.hip"]) == 4
    entries = found["rbox.hip"] | found["labels.hip"]
    assert entries == ENTRIES and len(ENTRIES) == 13
    assert entries <= set(re.findall(r"\b(ocr_\w+)\(", _read("include", "ocr_hip.h")))
    named = {e for r in M.ROWS.values() for e in r.entries}
    assert named == entries, sorted(entries ^ named)
    test = _read("tests", "test_gpu_rbox_label_matrix.py")
    assert all('"%s"' % e in test for e in entries), "an entry that no test calls by name"


def test_the_constants_the_rows_are_named_after_are_the_sources(M):
    rbox, labels = _read("tensorflow_ocr_amd", "csrc", "rbox.hip"), _read("tensorflow_ocr_amd", "csrc", "labels.hip")
    common, header = _read("tensorflow_ocr_amd", "csrc", "common.h"), _read("include", "ocr_hip.h")
    assert re.search(r"#define OCR_CHECK_SHAPE\(cond\)[^#]*?return OCR_ERR_UNSUPPORTED;", common, re.S)
    assert re.search(r"OCR_ERR_UNSUPPORTED = (-?\d+)", header).group(1) == str(M.UNSUPPORTED)
    # loss: 1024 pixels per workgroup, at most 1024 workgroups, 32 row groups in the finaliser, 8 floats per partial row
    assert "int b = ocr_cdiv(P, 256 * 4);" in rbox and "if (b > 1024) b = 1024;" in rbox
    assert "for (int t = g; t < T; t += 32)" in rbox and "constexpr int kLossCols = 8, kLossSums = 5;" in rbox
    assert [M.loss_blocks(P) for P in M.LOSS_P] == [1, 1, 1, 2, 33, 1024] and M._cdiv(M.LOSS_P[-1], 1024) == 1025 > 1024
    assert M.LOSS_P == (1, 255, 1024, 1025, 32 * 1024 + 1, 1024 * 1024 + 1)
    assert M._cdiv(M.LOSS_P[-1], 256 * 1024) >= 2 and M._cdiv(M.LOSS_P[-1], 256 * 2048) >= 2            # reduce and bwd: further trips
    assert "dim3(loss_blocks(P) * 2)" in rbox
    assert "1e-5f" in rbox and "1e-5)" in rbox and "q[k] < g[k] ?" in rbox
    # decode: 256 positions per workgroup, the scan walks the workgroup counts 256 at a time
    assert "for (int base = 0; base < d.blocks; base += 256)" in rbox and "ocr_cdiv(h * w, 256)" in rbox
    blocks = [M._cdiv(hw, 256) for hw in M.DECODE_HW]
    assert list(M.DECODE_HW) == [1, 255, 256, 257, 257 * 256, 2 * 65536 + 300] and blocks == [1, 1, 1, 2, 257, 514]
    assert all(h * w == hw and (w != h or hw == 1) for hw, (h, w) in M.DECODE_HW.items())
    assert "constexpr float kCoordLimit = 4194304.f;" in rbox and M.LIMIT == 4194304.0 == 2.0 ** 22
    assert "h <= 32768 && w <= 32768 && inv_scale > 0.f && inv_scale <= 1.f" in rbox
    # labels
    assert "constexpr int kChunk = 32;" in labels and "constexpr int kMaxPolys = 254;" in labels and "constexpr int kMaxV = 8;" in labels
    assert "constexpr int kTileW = 64, kTileH = 4;" in labels
    assert "if (b > 16384) b = 16384;" in labels and M.LGRID_THREADS == 16384 * 256
    assert "max_polys >= 1 && max_polys <= 254 && verts >= 3 && verts <= kMaxV && n <= 65535" in labels
    assert "h <= 16384 && w <= 16384" in labels
    assert "-ffp-contract=off" in _read("tensorflow_ocr_amd", "csrc", "Makefile") and "#pragma clang fp contract(off)" in labels
    assert M.HEAD_P == (1, 255, 256, 257, 1000) and M.RBOXLAB_P == (1, 12, 254)
    assert M.COVER_SHAPES == ((3, 63), (4, 64), (5, 65), (37, 130)) and M.COVER_VERTS == (3, 4, 5, 8)
    assert M.MEAN_MASKS == ((1, 1), (40, 56), (300, 520)) and M.MEAN_INV == (1.0, 0.5, 0.25)
    assert M.RBOXLAB_SHAPES == ((64, 64, 1), (37, 53, 4), (130, 97, 4))


def test_head_rows_hold_the_directed_values(M):
    want = {f32(v) for v in (0, 1e-4, -1e-4, 17, -17, 30, -30, 88, -88, 89, -89, 104, -104)}
    for P in M.HEAD_P:
        c = M.case("head/%d" % P)
        assert c["z"].shape == (P, 6) and c["z"].dtype == f32
        if P >= 13:
            for col in range(6):
                assert want <= set(c["z"][:13, col].tolist()), (P, col)
            assert (c["z"][13:, 5] == 0).sum() >= 30 and (np.abs(c["z"][13:]) <= 4).all()
        assert np.isfinite(c["fwd"]).all() and np.isfinite(c["bwd"]).all() and (c["bwd_bound"] > 0).all()
    # the saturated columns: expf overflows from 88.73 on, sigma is subnormal there; f32 stores the last value below 1 at 17
    # and 1 (the angle: +-f32(pi/4)) at 30
    assert math.exp(89) > 3.4028235e38 > math.exp(88) and M._sigma(f64(-88.0)) < 2.0 ** -126
    assert f32(M._sigma(f64(17.0))) == np.nextafter(f32(1), f32(0)) and f32(M._sigma(f64(30.0))) == 1
    assert f32(np.tanh(30.0 / 2) * math.pi / 4) == f32(math.pi / 4)


def test_loss_rows_tie_exactly_where_they_say(M):
    P = 1025
    y, p, gt, gp, m = M.case("loss/1025/ties")["inputs"]
    tie = gp[:, :4] == gt[:, :4]
    assert np.array_equal(tie, M.tie_pattern(P))
    n = tie.sum(1)
    idx = np.arange(P)
    assert (n[idx % 8 == 1] == 1).all() and (n[idx % 8 == 2] == 2).all() and (n[idx % 8 == 3] == 4).all() and (n[idx % 8 > 3] == 0).all()
    assert (n[idx % 8 == 0] == 0).all() and all(tie[:, k].sum() > 100 for k in range(4))
    assert (y[n > 0] == 1).all() and (m[n > 0] == 1).all()
    # the strict rule is visible: at a tie the reference gradient differs from the 1/2 share of an averaged subgradient
    for name in ["loss/%d" % q for q in M.LOSS_P] + ["loss/1025/%s" % c for c in M.LOSS_CONTENT if c != "ties"]:
        yy, _, g, q, _ = M.case(name)["inputs"]
        if name != "loss/1025/zero-gt":
            assert not (g[:, :4] == q[:, :4]).any(), name
    y, p, gt, gp, m = M.case("loss/1025/zero-gt")["inputs"]
    assert (gt[:, :4] == 0).all() and (gp[:, :4] > 0).all()
    y, p, gt, gp, m = M.case("loss/1025/big")["inputs"]
    assert gt[:, :4].min() >= 480 and gp[:, :4].max() <= 512
    y, p, gt, gp, m = M.case("loss/1025/angles")["inputs"]
    x = gp[:, 4].astype(f64) - gt[:, 4]
    assert (x[0::3] == 0).all() and (np.abs(x[1::3] - 1e-4) < 1e-7).all() and (np.abs(x[2::3] - math.pi / 2) < 1e-6).all()
    c = M.case("loss/1025/no-positive")
    assert (c["inputs"][0] == 0).all() and not c["live"].any() and c["out"].tolist()[2:] == [0.0, 0.0] and abs(c["out"][0] - 0.01) < 1e-15
    c = M.case("loss/1025/all-masked")
    assert (c["inputs"][4] == 0).all() and (c["sums"] == 0).all() and (c["d_cls"] == 0).all() and (c["d_geo"] == 0).all()
    for q in M.LOSS_P:
        c = M.case("loss/%d" % q)
        assert c["T"] == M.loss_blocks(q) and c["live"].any() and np.isfinite(c["out"]).all() and (c["sums_b"] > 0).all()
        assert (c["sums"][3:] > 0).all()                                  # both geometry terms are live


def test_decode_rows_select_exactly_the_stated_lanes(M):
    seen = set()
    for hw, (h, w) in M.DECODE_HW.items():
        i = np.arange(hw)
        for pat in M.PATTERNS:
            c = M.case("decode/%d/%s" % (hw, pat))
            sel = c["sel"]
            with np.errstate(invalid="ignore"):
                assert np.array_equal(c["score"].reshape(3, hw) > M.THR, sel), (hw, pat)
            want = {"all": np.ones(hw, bool), "none": np.zeros(hw, bool), "last": i == hw - 1, "lane63": i % 64 == 63, "lane0": i % 64 == 0,
                    "runs": (i % 64 == 63) | ((i % 64 == 0) & (i > 0))}.get(pat)
            if want is not None:
                assert np.array_equal(sel[0], want), (hw, pat)
            elif hw >= 255:
                assert 0.2 < sel[0].mean() < 0.4
            if pat == "threshold":
                assert (c["score"].reshape(3, hw)[0][~sel[0]] == M.THR).all()
            if pat == "nan":
                assert np.isnan(c["score"].reshape(3, hw)[0][~sel[0]]).all() and (hw == 1 or np.isnan(c["score"]).any())
            t = c["totals"]
            assert t == [int(s.sum()) for s in sel] and 0 in t
            assert hw == 1 or len(set(t)) == 3, (hw, pat, t)
            T = max(t)
            assert T >= 1 and c["max_ks"] == sorted({k for k in (1, T - 1, T, T + 1) if k >= 1})
            assert c["score"].shape == (3, h, w) and c["geo"].shape == (3, h, w, 5)
            seen.add((hw, pat))
            if hw >= 255:
                a = c["geo"].reshape(3, hw, 5)[sel][:, 4]
                for v in M.ANGLES:
                    assert (a.view(i32) == f32(v).view(i32)).any(), (hw, pat, v)        # +0.0 and -0.0 told apart
    assert len(seen) == 6 * 9
    # the runs pattern crosses waves and workgroups, and the large maps cross scan chunks with selected pixels in every chunk
    c = M.case("decode/%d/runs" % (2 * 65536 + 300))
    s = c["sel"][0]
    assert s[63] and s[64] and s[255] and s[256] and not s[0] and not s[65]
    for hw in (257 * 256, 2 * 65536 + 300):
        for pat in ("all", "lane0", "lane63", "random"):
            per_block = np.add.reduceat(M.case("decode/%d/%s" % (hw, pat))["sel"][0].astype(int), np.arange(0, hw, 256))
            assert len(per_block) == M._cdiv(hw, 256) > 256 and (per_block[:-1] > 0).all()      # (the last workgroup may be short of lane 63)


def test_decode_vec_is_decode_ref(M):
    worst = 0.0
    for hw in (255, 256, 257):
        for pat in ("random", "all", "runs"):
            c = M.case("decode/%d/%s" % (hw, pat))
            for b in range(3):
                a = H.decode_ref(c["score"][b], c["geo"][b], M.THR, M.SCALE)
                v = M.decode_vec(c["score"][b], c["geo"][b], M.THR, M.SCALE)
                assert a.shape == v.shape == (c["totals"][b], 9)
                worst = max(worst, float(np.abs(a - v).max()) if len(a) else 0.0)
    assert worst <= 1e-10, worst                            # float64 both; the bound they serve is 16 f32 ulp


def test_mean_rows_have_the_rasters_they_promise(M):
    for h, w in M.MEAN_MASKS:
        for inv in M.MEAN_INV:
            c = M.case("mean/%dx%d/%g" % (h, w, inv))
            at = {k: j for j, k in enumerate(c["names"])}
            for k in ("off left", "off right", "off above", "off below", "nan", "inf"):
                assert c["count"][at[k]] == 0 and c["ref"][at[k]] == 0, (h, w, inv, k)
            assert np.isnan(c["quads"][at["nan"]]).sum() == 1 and np.isinf(c["quads"][at["inf"]]).sum() == 1
            for k in ("whole", "2^22", "1e9"):
                assert c["count"][at[k]] == h * w, (h, w, inv, k)
            assert np.array_equal(M.mean_verts(c["quads"][at["1e9"]], inv), M.mean_verts(c["quads"][at["2^22"]], inv))
            assert np.abs(M.mean_verts(c["quads"][at["2^22"]], inv)).max() == 2 ** 22 * inv
            v = M.mean_verts(c["quads"][at["negative fractions"]], inv)
            q = c["quads"][at["negative fractions"]].astype(f64).reshape(4, 2)
            assert (v != np.floor(q * inv)).any()                           # trunc then floor, not floor alone
            assert c["count"][at["point"]] == 1 and c["count"][at["band 1e9"]] >= w
            if (h, w) != (1, 1):
                assert 1 < c["count"][at["hline"]] <= w and 1 < c["count"][at["vline"]] <= h
                assert sum(0 < c["count"][at["random%d" % j]] < h * w for j in range(6)) >= 4
    assert 300 * 520 / 256 > 600


def test_cover_rows_reach_every_chunk(M):
    counts, owners, seen_mp = set(), set(), set()
    for h, w in M.COVER_SHAPES:
        for V in M.COVER_VERTS:
            c = M.case("cover/%dx%d/v%d" % (h, w, V))
            mp = c["max_polys"]
            seen_mp.add(mp)
            assert c["polys"].shape == (4, mp, V, 2) and c["counts"][3] == mp + 7 > mp and (c["counts"][:3] <= mp).all()
            counts |= set(c["counts"][:3].tolist())
            last = (c["ref"] >> 8) & 255
            owners |= set(np.unique(last).tolist())
            assert last[3].max() == mp                      # the clamped image still draws polygon max_polys - 1
            assert ((c["ref"] >> 16) & 1).any() and (c["ref"] == 0).any() or h * w < 300
            p = c["polys"][0, :c["counts"][0]]
            if len(p) >= 8:
                assert (p[6, :, 0] < -1000).all() and (p[5] == p[5, 0]).all() and (p[3, :, 1] == p[3, 0, 1]).all() and (p[2, 0] == p[2, 1]).all()
                assert p.min() < 0 and p[:, :, 0].max() >= w
    assert counts == {0, 1, 32, 33, 64, 65, 254} and seen_mp == {254, 65, 33, 64}
    assert 254 in owners and any(33 <= o for o in owners) and any(65 <= o < 254 for o in owners)     # indices 253, >= 32, >= 64
    assert M.COVER_SHAPES[0][1] % 64 and M.COVER_SHAPES[0][0] % 4 and not M.COVER_SHAPES[1][1] % 64 and not M.COVER_SHAPES[1][0] % 4


def test_label_restatements_are_the_oracle_and_rows_reach_their_edges(M):
    for key, (n, size, step) in M.ICDAR_ROWS.items():
        c = M.case("icdar/" + key)
        last, first = (c["cover"] >> 8) & 255, c["cover"] & 255
        assert (last[:, 0, :] > 0).any() and (last[:, :, 0] > 0).any()                 # row 0 and column 0 are owned ...
        assert ((last[0][:, 0] > 0) & (first[0][:, size - 1] > 0)).any()               # ... and so is a wrapped neighbour
        sampled = last[0][::step, ::step]
        assert (sampled[:, -1] > 0).any() and ((size - 1) % step == 0) == (key in ("64/1", "65/1", "65/4", "420/1"))
        assert ((c["cover"] >> 16) & 1).any()
        if size <= 65:
            s, g, m = OL.icdar_generate_rbox((size, size), c["polys"][0], c["tags"][0])
            assert np.array_equal(c["ref"][0][0, ..., 0], s[::step, ::step].astype(f32))
            assert np.array_equal(c["ref"][1][0], g[::step, ::step]) and np.array_equal(c["ref"][2][0, ..., 0], m[::step, ::step].astype(f32))
            assert 0 < g.mean() < 1
        else:
            assert n * M._cdiv(size, step) ** 2 * 8 > M.LGRID_THREADS and n * size * size > 524288
            assert (last[2] == 0).all() and last[1].any()
    for key, (n, h, w, nh, nw) in M.PIXELLINK_ROWS.items():
        c = M.case("pixellink/" + key)
        if (nh, nw) == (h // 4, w // 4):
            xs, ys = c["norm"][0]
            s, lk, _ = OL.pixellink_generate_rbox(h, w, xs, ys, np.zeros((len(xs), 4), f32), np.zeros(len(xs), i32))
            assert np.array_equal(c["ref"][0][0], s) and np.array_equal(c["ref"][1][0], lk) and 0 < lk.mean() < 1 and (lk == 0).any()
        assert c["ref"][0].shape == (n, nh, nw) and c["ref"][1].shape == (n, nh, nw, 8)
        assert c["ref"][0][0].any() or (nh, nw) == (1, 1)
    assert 3 * 420 * 420 * 8 > M.LGRID_THREADS and M.pixellink_case.__defaults__ is None
    # the second pin of pixellink_vec: another quarter-size map, against the oracle
    c = M.pixellink_case(1, 64, 96, 16, 24)
    xs, ys = c["norm"][0]
    s, lk, _ = OL.pixellink_generate_rbox(64, 96, xs, ys, np.zeros((len(xs), 4), f32), np.zeros(len(xs), i32))
    assert np.array_equal(c["ref"][0][0], s) and np.array_equal(c["ref"][1][0], lk)


def test_rbox_label_rows_fill_the_table_and_leave_a_ragged_workgroup(M):
    for P in M.RBOXLAB_P:
        for h, w, step in M.RBOXLAB_SHAPES:
            c = M.case("rboxlab/%d/%dx%ds%d" % (P, h, w, step))
            assert c["rects"].shape == (3, P, 5, 3) and c["owner"].max() == P == c["raw_owner"].max()       # the table's last row is read
            assert (c["owner"] == 0).any() and (c["mask"] == 0).any() and (c["mask"] == 1).any()
            assert (c["owner"][2] == 0).all()
            if P == 254:
                assert len(np.unique(c["owner"])) > (20 if step == 4 else 100)
            assert np.abs(c["geo64"]).max() < 4096 and (np.abs(c["geo"][..., :4].astype(f64) - c["geo64"]) <= 2e-3).all()
    cells = [M._cdiv(h, s) * M._cdiv(w, s) for h, w, s in M.RBOXLAB_SHAPES]
    assert cells == [4096, 140, 825] and 825 % 256 == 57 and 37 % 4 and 53 % 4
    c = M.case("rboxlab/above")
    assert c["P"] == 12 and c["raw_owner"].max() > 12 and (c["owner"][c["raw_owner"] > 12] == 0).all()
    assert (c["geo"][c["raw_owner"] > 12] == 0).all() and (c["score"][c["raw_owner"] > 12] == 0).all() and (c["owner"] > 0).any()
    # separate multiplies and adds are not the fused form: the f32 restatement differs from a single rounding somewhere
    c = M.case("rboxlab/254/64x64s1")
    fused = c["geo64"].astype(f32)
    assert (fused != c["geo"][..., :4]).any()
