"""Host half of tests/test_gpu_train_side_matrix.py, no device: the rows of its table against the extern "C" entries of
csrc/pixellink_balance.hip, csrc/summary.hip and csrc/augment.hip, the constants its rows are named after against the sources,
and — with the references alone (tests/balanced_ref.py, the restatements of tests/test_gpu_summary.py and
tests/test_gpu_augment.py) — that every row's inputs have the pattern the row promises: a row that does not reach its edge
fails here, not silently on the GPU.  The GPU file introduces no vectorised restatement of its own (the references it
imports are NumPy over whole arrays already), so there is none to pin; what is pinned instead is image_ref, the one place
where it says more than TS._image_rule does."""
import os
import re

import numpy as np
import pytest

import balanced_ref as B
from oracle import ocr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, u32 = np.float32, np.float64, np.uint32

ENTRIES = {
    "pixellink_balance.hip": {"ocr_pixellink_instance_weights", "ocr_balanced_loss_workspace", "ocr_balanced_loss_fwd", "ocr_balanced_loss_selected",
                              "ocr_balanced_loss_bwd", "ocr_balanced_loss_bwd_dyn"},
    "summary.hip": {"ocr_tensor_stats_num_buckets", "ocr_tensor_stats_chunk", "ocr_tensor_stats_record_bytes", "ocr_tensor_stats_workspace",
                    "ocr_tensor_stats_table_bytes", "ocr_tensor_stats_limits", "ocr_tensor_stats_table", "ocr_tensor_stats_f32",
                    "ocr_summary_image_workspace", "ocr_summary_image_u8"},
    "augment.hip": {"ocr_augment_u8_batch"},
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def M():
    import test_gpu_train_side_matrix as M
    return M


def test_every_entry_is_named_by_a_row(M):
    found = {f: set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', _read("tensorflow_ocr_amd", "csrc", f))) for f in ENTRIES}
    assert found == ENTRIES and [len(found[f]) for f in ENTRIES] == [6, 10, 1]
    entries = set().union(*found.values())
    assert len(entries) == 17 and entries <= set(re.findall(r"\b(ocr_\w+)\(", _read("include", "ocr_hip.h")))
    named = {e for r in M.ROWS.values() for e in r.entries}
    assert named == entries, sorted(entries ^ named)
    test = _read("tests", "test_gpu_train_side_matrix.py")
    assert all('"%s"' % e in test for e in entries), "an entry that no test calls by name"
    assert M.pytestmark.name == "gpu"


def test_the_constants_the_rows_are_named_after_are_the_sources(M):
    bal, summ, aug = (_read("tensorflow_ocr_amd", "csrc", f) for f in ENTRIES)
    header = _read("include", "ocr_hip.h")
    # balanced loss: 1024 pixels per workgroup, at most 1024 workgroups, 1024 mining threads, 4 row groups, 34 sums
    assert "size_t b = (total + 256 * 4 - 1) / (256 * 4);" in bal and "if (b > 1024) b = 1024;" in bal
    assert M.BL_PER_BLOCK == 256 * 4 == 1024 and M.BL_CAP == 1024
    assert bal.count("for (int i = threadIdx.x; i < p.hw; i += 1024)") == 2 and "dim3(p.n), dim3(1024)" in bal and M.MINE_THREADS == 1024
    assert "for (int t = g; t < T; t += 4)" in bal and M.FINAL_GROUPS == 4 and "constexpr int NS = 34;" in bal and M.NS34 == 34
    assert "const int T = bl_blocks((size_t)p.n * p.hw) * 2;" in bal
    # weight map: 1024 cells per workgroup, at most 256 workgroups
    assert "int64_t b = ((int64_t)new_h * new_w + 256 * 4 - 1) / (256 * 4);" in bal and "if (b > 256) b = 256;" in bal
    assert M.WM_PER_BLOCK == 1024 and M.WM_CAP == 256 and "max_polys >= 1 && max_polys <= 254" in bal
    # summaries
    assert "constexpr unsigned kStatsGrid = 2048;" in summ and M.STATS_GRID == 2048
    assert re.search(r"#define OCR_TENSOR_STATS_CHUNK (\d+)", header).group(1) == str(M.CHUNK)
    assert re.search(r"#define OCR_TENSOR_STATS_BUCKETS (\d+)", header).group(1) == str(M.BUCKETS)
    assert re.search(r"#define OCR_TENSOR_STATS_POS_LIMITS (\d+)", header).group(1) == str(M.POS_LIMITS)
    assert "ocr_tensor_stats_record;       /* %d bytes" % M.RECORD_BYTES in header
    assert "sizeof(StatsHeader) == %d && sizeof(StatsSeg) == %d && sizeof(Partial) == %d" % (M.HEADER_BYTES, M.SEG_BYTES, M.PARTIAL_BYTES) in summ
    assert "constexpr unsigned kMagic = 0x%xu;" % M.MAGIC in summ
    assert "for (int i = threadIdx.x; i < s.n_chunks; i += 256)" in summ and M.FINAL_THREADS == 256
    assert "for (int c = blockIdx.x; c < h.n_chunks; c += gridDim.x)" in summ
    assert "constexpr int kImgGrid = 64;" in summ and M.IMG_GRID == 64 and M.IMG_TRIP == 64 * 256
    assert "if (grid > 1024) grid = 1024;" in summ and M.IMG_U8_CAP == 1024
    assert "(c == 1 || c == 3 || c == 4)" in summ and "(long long)h * w * c <= (1ll << 30)" in summ
    # augmentation
    assert "constexpr int PX = 4;" in aug and M.PX == 4 and "if (S % PX == 0 && ((uintptr_t)dst_f32 & 15) == 0)" in aug
    nofma = re.search(r"^NOFMA := (.*)$", _read("tensorflow_ocr_amd", "csrc", "Makefile"), re.M).group(1).split()
    assert "summary" in nofma and "augment" in nofma and "-ffp-contract=off" in _read("tensorflow_ocr_amd", "csrc", "Makefile")
    # the status codes the refusals are held to
    assert re.search(r"OCR_ERR_INVALID_ARG = (-?\d+)", header).group(1) == str(M.INVALID_ARG)


def test_weight_rows_reach_their_grids(M):
    assert list(M.WM_CELLS) == [1, 1023, 1024, 1025, 262656] and all(h * w == c for c, (h, w) in M.WM_CELLS.items())
    assert [M.wm_blocks(c) for c in M.WM_CELLS] == [1, 1, 1, 2, 256] and M._cdiv(262656, 1024) == 257 > 256 and 262656 > 256 * 256
    for cells, (nh, nw) in M.WM_CELLS.items():
        c = M.case("weights/cells%d" % cells)
        assert c["weight"].shape == (2, nh, nw) and c["cover"].shape == (2, 64, 64) and c["area"].sum() > 0
        if cells >= 1023:
            assert c["live"][0].sum() >= 4 and not c["live"][0, 3] and c["area"][0, 3] > 0 and (c["weight"] == 0).any()
    c = M.case("weights/cells1025")                           # both workgroups count cells of one polygon: the global atomic merges
    wg = (np.arange(1025) // 256) % 2
    own = c["owner"][0].ravel()
    assert any(len(set(wg[own == j].tolist())) == 2 for j in range(1, 7))
    c = M.case("weights/cells262656")
    assert c["nh"] > c["h"] and c["nw"] > c["w"] and c["area"].max() > 65536
    c = M.case("weights/ratio")
    assert (c["h"], c["w"], c["nh"], c["nw"]) == (48, 80, 13, 21) and 48 % 13 and 80 % 21 and c["n"] == 2
    c = M.case("weights/p254")
    assert c["P"] == 254 and c["live"].all() and len(set(c["area"][0].tolist())) >= 8 and len(np.unique(c["weight"])) >= 9
    c = M.case("weights/counts")
    assert c["n"] == 3 and c["P"] == 254 and c["live"].sum(1).tolist() == [0, 1, 254] and (c["weight"][0] == 0).all()
    c = M.case("weights/above")
    assert c["P"] == 12 and c["raw_owner"].max() == 20 and (c["owner"][c["raw_owner"] > 12] == 0).all() and (c["weight"][c["raw_owner"] > 12] == 0).all()
    assert c["owner"].max() == 12 and c["ignore"].shape == (2, 12)
    c = M.case("weights/ignore-bytes")
    assert sorted(set(c["ignore"].ravel().tolist())) == [0, 2, 255] and c["area"][0, 0] > 0 and c["area"][0, 2] > 0
    assert not c["live"][0, 0] and not c["live"][0, 2] and (c["weight"][0][np.isin(c["owner"][0], (1, 3))] == 0).all() and c["live"][0].sum() >= 2
    c = M.case("weights/split")
    cells = np.flatnonzero(c["owner"][0].ravel() == 1)
    assert c["nh"] * c["nw"] == 1025 and M.wm_blocks(1025) == 2 and cells.min() == 205 and cells.max() == 327
    assert set(((cells // 256) % 2).tolist()) == {0, 1}
    for name in M.WM_ROWS:
        c = M.case("weights/" + name)
        assert c["cover"].dtype == u32 and not (c["cover"] >> 17).any()


def test_loss_rows_reach_their_block_counts(M):
    totals = [n * hw for n, hw in M.LOSS_TOTALS]
    assert totals == [1, 1023, 1024, 1025, 3075, 33000, 1048578]
    assert [B.blocks(t) for t in totals] == [1, 1, 1, 2, 4, 33, 1024]
    assert M._cdiv(1048578, 1024) == 1025 > 1024 and 1048578 > 2 ** 20
    assert M._cdiv(1048578, 1024 * 256) == 5 and M._cdiv(1048578, 2048 * 256) == 3 and B.m_sum(1048578) == 5 + 10
    assert M._cdiv(33, M.FINAL_GROUPS) == 9 and M._cdiv(3, M.FINAL_GROUPS) == 1
    assert M._cdiv(4097, M.MINE_THREADS) == 5 and M._cdiv(1025, M.MINE_THREADS) == 2 and (1, 4097) in M.LOSS_SMALL
    # image boundaries inside a workgroup's 256-pixel trips
    assert 1025 % 256 and (2 * 1025) % 256 and 349526 % 256 and 11000 % 256
    for n, hw in M.LOSS_SMALL:
        for focal in (0, 1):
            c = M.case("loss/n%d_hw%d_f%d" % (n, hw, focal))
            assert (c.n, c.hw, c.focal) == (n, hw, focal) and c.pl.shape == (n, hw, 2) and c.ll.shape == (n, hw, 16)
            if hw > 1:
                assert ((c.plab > 0) & (c.w == 0)).any() and (c.w > 0).any()
    assert "loss/n3_hw349526_f0" in M.ROWS and "loss/n3_hw349526_f1" not in M.ROWS


def test_mining_rows_have_their_kth_score_where_they_say(M):
    assert set(M.MINE_ROWS) == {"lowbyte", "ties", "kmax", "floor", "nan-label", "nan-weight"}
    for kind in M.MINE_ROWS:
        c = M.case("mine/" + kind)
        thr, W, P, mined, ks = B.mine(c)
        with np.errstate(invalid="ignore"):
            neg = ~(c.plab[0] > 0)
        score = O.neg_score_f32(c.pl[0, :, 0], c.pl[0, :, 1])
        u = score.view(u32)
        k = ks[0]
        assert c.hw == 4097 and c.n == 1 and 0 < k <= neg.sum() and thr[0] == np.sort(score[neg])[k - 1]
        if kind == "lowbyte":
            assert len(set((u[neg] >> 8).tolist())) == 1 and len(set((u[neg] & 255).tolist())) >= 200
            assert k == 1500 < neg.sum() and 0 < mined.sum() - k < 40          # the k-th place lies inside the block; a few equal scores
        if kind == "ties":
            s = np.sort(score[neg])
            assert k == 300 and s[199] < s[200] == s[299] == s[499] < s[500] and mined.sum() == 500
        if kind == "kmax":
            assert k == neg.sum() == 4097 - 1100 and (mined == neg[None]).all() and P.sum() * 3 > k
        if kind == "floor":
            floor = O.neg_score_f32(f32(0), f32(80))
            assert k == 1 and thr[0] == floor > 0 and mined.sum() == 3 and (score >= floor).all()
            # the clamp of det_exp: no difference, however large, scores below the floor, so a score of exactly 0 does not exist
            assert (O.neg_score_f32(np.zeros(4, f32), np.array([80, 100, 1000, 3e38], f32)) == floor).all()
            assert set(c.pl[0, mined[0], 1].tolist()) == {80.0, 100.0, 1000.0}
        if kind == "nan-label":
            nan = np.isnan(c.plab[0])
            assert nan.sum() > 500 and neg[nan].all() and mined[0][nan].any() and not mined[0][nan].all() and neg.sum() == 4097 - 400
        if kind == "nan-weight":
            nan = np.isnan(c.w[0])
            text = c.plab[0] > 0
            assert (nan & text).sum() == 100 and (nan & ~text).sum() > 500 and not P[0][nan].any() and P.sum() == 300
            assert (W[0][nan & text] == 0).all() and mined[0][nan & ~text].any() and k == 900


def test_stats_rows_reach_their_chunks(M):
    import test_gpu_summary as TS
    c = M.case("stats/4100")
    assert len(c["offs"]) == 4100 == c["n_chunks"] > 2 * M.STATS_GRID and 4100 - 2 * M.STATS_GRID == 4
    assert set(c["sizes"]) == set(range(1, 10)) and sum(o % 4 != 0 for o in c["offs"]) > 2500
    ends = np.array(c["offs"]) + np.array(c["sizes"])
    assert (np.array(c["offs"])[1:] > ends[:-1]).all() and ends[-1] <= c["x"].size
    used = np.zeros(c["x"].size, bool)
    for o, s in zip(c["offs"], c["sizes"]):
        used[o:o + s] = True
    assert (c["x"][~used] == TS.PAD).all() and not (c["x"][used] == TS.PAD).any()
    occ = np.stack([r["bucket"] > 0 for r in c["refs"]])
    assert all(r["num"] == s and r["nonfinite"] == 0 for r, s in zip(c["refs"], c["sizes"]))
    for step in (1, M.STATS_GRID, 2 * M.STATS_GRID):             # the next segment, and the next chunks of the same workgroup
        assert not (occ[:-step] & occ[step:]).any(), step
    assert c["mul"] == (0.5, 3.0)
    c = M.case("stats/301")
    assert c["n_chunks"] == 301 > M.FINAL_THREADS and c["sizes"] == [300 * M.CHUNK + 5] and c["refs"][0]["nonfinite"] >= 3
    assert (c["refs"][0]["bucket"] > 0).sum() > 300 and c["refs"][0]["min"] == -5e7 and c["refs"][0]["max"] < 5e7
    assert len(M.case("stats/one")["offs"]) == 1 and M.case("stats/one")["n_chunks"] == 2
    c = M.case("stats/overlap")
    assert c["offs"][1] < c["offs"][0] + c["sizes"][0] and c["offs"][0] % 4 and c["n_chunks"] == 2
    c = M.case("stats/last")
    assert c["offs"][-1] + c["sizes"][-1] == c["x"].size and c["offs"][-1] % 4 and M.XBAND > 0


def test_image_rows_hold_their_extremes_where_they_say(M):
    import test_gpu_summary as TS
    assert list(M.IMAGE_SHAPES) == [1, 16383, 16384, 16385, 262144, 262656] and all(h * w * c == n for n, (h, w, c) in M.IMAGE_SHAPES.items())
    assert {s[2] for s in M.IMAGE_SHAPES.values()} == {1, 3, 4} and M.IMG_TRIP == 16384
    assert [min(M._cdiv(n, 256), M.IMG_U8_CAP) for n in M.IMAGE_SHAPES] == [1, 64, 64, 65, 1024, 1024] and M._cdiv(262656, 256) == 1026
    for n in M.IMAGE_SHAPES:
        c = M.case("image/n%d" % n)
        assert np.isfinite(c["x"]).all() and np.array_equal(c["ref"], TS._image_rule(c["x"]))     # image_ref is the rule where the rule speaks
        assert (c["x"].min() < 0) == bool(n % 2) and (n == 1 or len(np.unique(c["ref"])) > 100)
    n = 16385
    flat = lambda k: M.case("image/" + k)["x"].ravel()
    c = M.case("image/nonfinite")
    x = c["x"].ravel()
    assert np.isinf(x).sum() == 200 and np.isnan(x).sum() == 100 and (c["ref"].ravel()[~np.isfinite(x)] == 0).all()
    clean = np.where(np.isfinite(x), x, 0).astype(f32)
    assert np.array_equal(c["ref"].ravel()[np.isfinite(x)], TS._image_rule(clean)[np.isfinite(x)]) and clean.min() < 0
    c = M.case("image/no-finite")
    assert not np.isfinite(c["x"]).any() and np.isnan(c["x"]).any() and np.isinf(c["x"]).any() and (c["ref"] == 0).all()
    assert not M.case("image/zeros")["x"].any() and (M.case("image/zeros")["ref"] == 0).all()
    c = M.case("image/tiny")
    assert c["x"].min() >= 0 and c["x"].max() == f32(9e-7) < f32(1e-6) and (c["ref"] == 0).all()
    c = M.case("image/tiny-signed")
    assert c["x"].min() == f32(-9e-7) and c["x"].max() == f32(9e-7) and (c["ref"] == 128).all()
    c = M.case("image/neg-zero")
    x = c["x"].ravel()
    assert np.signbit(x[x == 0]).all() and (x == 0).sum() > 2000 and x.min() == 0 and c["ref"].max() >= 254 and (c["ref"].ravel()[x == 0] == 0).all()
    for k, at, arg in (("max-last", n - 1, np.argmax), ("min-last", n - 1, np.argmin), ("max-wg63", M.IMG_TRIP - 1, np.argmax),
                       ("min-wg63", M.IMG_TRIP - 1, np.argmin)):
        x = flat(k)
        rest = np.delete(x, at)
        assert arg(x) == at == M.case("image/" + k)["at"] and x.size == n
        assert abs(x[at]) > 4 * np.abs(rest).max()                        # an extreme that is missed changes nearly every byte
        assert (at // 256) % M.IMG_GRID == (0 if at == n - 1 else 63) and at // M.IMG_TRIP == (1 if at == n - 1 else 0)
    assert flat("max-last").min() >= 0 and flat("min-last").max() > 0
    x = flat("mn-gt-mx")
    assert x.min() == -250 and x.max() == 90 and M.case("image/mn-gt-mx")["ref"].min() <= 1 and M.case("image/mn-gt-mx")["ref"].max() < 200
    x = flat("mn-lt-mx")
    assert x.min() == -90 and x.max() == 250 and M.case("image/mn-lt-mx")["ref"].max() == 255 and M.case("image/mn-lt-mx")["ref"].min() > 60


def test_augment_rows_reach_their_paths(M):
    assert M.AUG_S == (1, 2, 3, 4, 5, 36, 37, 128) and [M._cdiv(S, M.PX) for S in (1, 2, 3, 4, 5)] == [1, 1, 1, 1, 2]
    q = M.aug_quads(36)
    assert q == 324 and M._cdiv(q, 256) == 2 and q - 256 == 68 and 36 % 4 == 0 and 37 % 4 and 128 % 4 == 0
    assert M._cdiv(M.aug_quads(128), 256) == 16 and M.aug_quads(128) % 256 == 0
    for S in M.AUG_S:
        c = M.case("augment/S%d" % S)
        assert c["ref"].shape == (3, S, S, 3) and len({c["ims"][i].shape for i, _, _ in c["recs"]}) == 3
        assert all(o % 2 == 1 for o in c["offs"]) and sum(o % 4 != 0 for o in c["offs"]) >= 2
        if S >= 36:
            sat = c["ref"][1]
            assert (sat == 0).any() and (sat == 255).any() and ((sat > 0) & (sat < 255)).any() and (c["ref"][2] == 0).any() and c["ref"][0].any()
        # the surroundings of every image differ from what a tap off its end would have to read as: zero
        slab = c["slab"]
        for i, o in zip([r[0] for r in c["recs"]], c["offs"]):
            assert slab[o - 1] == 0xFB and slab[o + c["ims"][i].size] == 0xFB
    for S, (H, W) in M.MAP_S.items():
        case = lambda k: M.case("augment/%s/S%d" % (k, S))
        c = case("identity")
        assert W < S and H < S and np.array_equal(c["ref"][0, :H, :W], c["ims"][0].astype(f32)) and not c["ref"][0, H:].any() and not c["ref"][0, :, W:].any()
        c = case("half")
        sx, sy = M.map_coords(c)
        assert sx[0, 0] == -1 and sx[0, W] == W - 1 and (sy[:, 0] == np.arange(S)).all()
        assert c["ref"][0, 0, 0].any() and c["ref"][0, 0, W].any() and not c["ref"][0, :, W + 1:].any()
        assert np.array_equal(c["ref"][0, :H, 0], c["ims"][0][:, 0].astype(f32) * f32(0.5))                 # exactly one live column, weight 16 / 32
        c = case("outside")
        sx, sy = M.map_coords(c)
        assert (sx > W).all() and (sy < -2).all() and (c["ref"][0] == np.array([0, 255, 77.5], f32)).all()
        c = case("big")
        sx, sy = M.map_coords(c)
        assert (sx > W).any() and (sx < -2).any() and (sy > H).any() and (sy < -2).any() and np.abs(sx).max() >= 2 ** 24 and 2 ** 40 in c["recs"][0][1]
        assert (0 <= sx[0, 0] < W) and (0 <= sy[0, 0] < H) and c["ref"][0, 0, 0].any() and np.count_nonzero(c["ref"][0].any(-1)) == 1
        c = case("negfrac")
        A = c["recs"][0][1]
        X16 = A[2] + 1024
        assert X16 < 0 and X16 % 2048 and (X16 >> 11) == -(-X16 // 2048) - 1 and M.map_coords(c)[0][0, 0] == -2       # floor, not truncation
        assert (A[5] + 1024) < 0 and (A[5] + 1024) % 2048 and c["ref"][0].any()
        assert case("src1x1")["ims"][0].shape == (1, 1, 3) and case("src1x1")["ref"].any()
        assert case("src1xW")["ims"][0].shape == (1, W, 3) and case("src1xW")["ref"].any()
        c = case("sat0")
        assert (c["ref"][0][:H, :W] == 0).mean() > 0.9 and (c["ref"][0] >= 0).all() and (c["ref"][0][H:] == np.array([10, 3, 0], f32)).all()
        c = case("sat255")
        assert (c["ref"][0][:H, :W] == 255).mean() > 0.7 and (c["ref"][0] <= 255).all() and (c["ref"][0][H:, :, 0] == 100).all()
    c = M.case("augment/unaligned")
    assert c["S"] == 36 and c["ref"].shape == (3, 36, 36, 3)
    assert len(M.AUG_ROWS) == 8 + 9 * 2 and len(M.ROWS) == len({*M.ROWS})
