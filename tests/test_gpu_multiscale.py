"""GPU: multi-scale RBOX inference (csrc/multiscale.hip) against the sequential NumPy reference of tests/ms_ref.py —
ocr_ms_pool_append bit for bit, ocr_quad_fuse exact in keep_idx / n_keep / owner and bit-equal in `fused` for both modes —
then the status codes, rbox.detect_multiscale at one scale against rbox.detect, and evaluate.Evaluator(scales=...) against
the host composition rbox.detect per scale -> ms_ref -> oracle/evalboxes.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import ms_ref as M
from oracle import evalboxes as OE

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
SENT_I, SENT_F = -123456, f32(-12345.5)


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


def _up(device):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(i32)


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("with_mask", [False, True])
def test_append_equals_the_reference_bit_for_bit(device, with_mask):
    from tensorflow_ocr_amd import ops
    up = _up(device)
    n, max_k, max_pool, n_keep = 3, 70, 128, np.array([0, 1, 70], i32)
    rng = np.random.default_rng(31 + with_mask)
    pool_d = torch.full((n, max_pool, 9), float(SENT_F), dtype=torch.float32, device=device)
    scale_d = torch.full((n, max_pool), SENT_I, dtype=torch.int32, device=device)
    counters = torch.zeros((3, n + 1), dtype=torch.int32, device=device)
    counters[:, n] = SENT_I                                                  # a guard column behind the n images
    want_pool = np.full((n, max_pool, 9), SENT_F, f32)
    want_scale = np.full((n, max_pool), SENT_I, i32)
    want_cnt = [[0, 0, 0] for _ in range(n)]
    for s, ratio in enumerate([(0.5, 0.5), (0.75, 1.5), (2.0, 1.25)]):
        merged = rng.uniform(-300, 900, (n, max_k, 9)).astype(f32)
        keep = np.stack([rng.permutation(max_k) for _ in range(n)]).astype(i32)
        mean = rng.integers(0, 33, (n, max_k)).astype(f32) / f32(32)
        passed = (rng.uniform(0, 1, (n, max_k)) < 0.8) if with_mask else None
        if s == 1:
            merged[2, keep[2, 5], 3] = np.nan                                # one row with a NaN coordinate, in a surviving slot
            if with_mask:
                passed[2, 5] = True
        ratios = np.tile(np.array(ratio, f32), (n, 1))
        ratios[1] = ratios[1][::-1]                                          # ratios differ per image too
        ops.ms_pool_append(up(merged), up(keep), up(n_keep), None if passed is None else up(passed.astype(np.uint8)), up(mean),
                           up(ratios), s, pool_d, scale_d, counters[0, :n], counters[1, :n], counters[2, :n])
        for i in range(n):
            M.append_ref(want_pool[i], want_scale[i], want_cnt[i], merged[i], keep[i], n_keep[i],
                         None if passed is None else passed[i], mean[i], ratios[i], s)
    torch.cuda.synchronize()
    got_cnt = counters.cpu().numpy()
    assert got_cnt[:, :n].T.tolist() == want_cnt and (got_cnt[:, n] == SENT_I).all()
    assert want_cnt[0] == [0, 0, 0] and want_cnt[1][0] == want_cnt[1][1] <= 3
    assert want_cnt[2][0] == max_pool < want_cnt[2][1] and want_cnt[2][2] == 1          # the overflow keeps the true count; one NaN row
    if not with_mask:
        assert want_cnt[1] == [3, 3, 0] and want_cnt[2][1] == 3 * 70 - 1
    assert np.array_equal(_bits(pool_d.cpu().numpy()), _bits(want_pool))     # rows beyond each count still hold the sentinel
    assert np.array_equal(scale_d.cpu().numpy(), want_scale)


def test_append_writes_nothing_at_or_beyond_max_pool(device):
    """the pool of the LAST image ends where the allocation's guard rows begin: max_pool = 128 rows are followed by sentinel
    rows, which the overflowing image (210 candidates) must leave alone"""
    from tensorflow_ocr_amd import ops
    up = _up(device)
    n, max_k, max_pool = 1, 70, 128
    rng = np.random.default_rng(5)
    buf = torch.full((max_pool + 64, 9), float(SENT_F), dtype=torch.float32, device=device)
    sbuf = torch.full((max_pool + 64,), SENT_I, dtype=torch.int32, device=device)
    counters = torch.zeros((3, n), dtype=torch.int32, device=device)
    for s in range(3):
        merged = rng.uniform(0, 500, (n, max_k, 9)).astype(f32)
        keep = np.arange(max_k, dtype=i32)[None]
        ops.ms_pool_append(up(merged), up(keep), up(np.array([70], i32)), None, up(np.full((n, max_k), 0.5, f32)),
                           up(np.ones((n, 2), f32)), s, buf[:max_pool][None], sbuf[:max_pool][None], counters[0], counters[1],
                           counters[2])
    torch.cuda.synchronize()
    assert counters.cpu().numpy().reshape(-1).tolist() == [128, 210, 0]
    assert (buf[max_pool:] == float(SENT_F)).all() and (sbuf[max_pool:] == SENT_I).all()
    assert (sbuf[:max_pool].cpu().numpy() == np.repeat([0, 1, 2], 70)[:max_pool]).all()


# ------------------------------------------------------------------------------------------------ fuse
@functools.lru_cache(maxsize=None)
def _fuse_reference(case, thr, mode):
    """the reference of a named batch, computed once: [(fused, keep, owner)] per image.  The sweep does not depend on the
    mode and mode 0's rows are the pool rows, so 'nms' is read off the 'vote' run"""
    if mode == "nms":
        return [(np.ascontiguousarray(pool, f32), keep, owner)
                for pool, (_, keep, owner) in zip(_fuse_pools(case), _fuse_reference(case, thr, "vote"))]
    return [M.fuse_ref(pool, thr, mode) for pool in _fuse_pools(case)]


@functools.lru_cache(maxsize=None)
def _fuse_pools(case):
    if case == "mixed":
        return [p for p, _, _ in M.fuse_batch()]
    if case == "wide":
        return [M.cluster_case(1000, 2000)[0]]
    return [p for p, _ in M.hand_cases().values()]


def _run_fuse(device, graph, pools, max_pool, thr, mode):
    from tensorflow_ocr_amd import ops
    n = len(pools)
    pool = np.full((n, max_pool, 9), SENT_F, f32)
    for i, p in enumerate(pools):
        pool[i, :len(p)] = p
    count = np.array([len(p) for p in pools], i32)
    fused = torch.full((n, max_pool, 9), float(SENT_F), dtype=torch.float32, device=device)
    keep = torch.full((n, max_pool), SENT_I, dtype=torch.int32, device=device)
    owner = torch.full((n, max_pool), SENT_I, dtype=torch.int32, device=device)
    n_keep = torch.full((n,), SENT_I, dtype=torch.int32, device=device)
    up = _up(device)
    ops.quad_fuse(up(pool), up(count), thr, mode, fused, keep, n_keep, owner, graph.workspace())
    torch.cuda.synchronize()
    return fused.cpu().numpy(), keep.cpu().numpy(), n_keep.cpu().numpy(), owner.cpu().numpy()


def _check_fuse(got, pools, want, max_pool):
    fused, keep, n_keep, owner = got
    for i, (p, (w_fused, w_keep, w_owner)) in enumerate(zip(pools, want)):
        P = len(p)
        assert n_keep[i] == len(w_keep), (i, P)
        assert np.array_equal(keep[i, :n_keep[i]], w_keep), (i, P)
        assert (keep[i, n_keep[i]:] == SENT_I).all()
        assert np.array_equal(owner[i, :P], w_owner) and (owner[i, P:] == -1).all(), (i, P)
        assert np.array_equal(_bits(fused[i, :P]), _bits(w_fused)), (i, P)
        assert (fused[i, P:] == SENT_F).all()                                # rows at and beyond the count are not written
        scores = fused[i, keep[i, :n_keep[i]], 8]
        assert (np.diff(scores) <= 0).all()                                  # the kept list is in descending score order


@pytest.mark.parametrize("mode", ["nms", "vote"])
@pytest.mark.parametrize("thr", M.FUSE_THRESHOLDS)
def test_fuse_mixed_counts_equal_the_reference(device, graph, thr, mode):
    pools = _fuse_pools("mixed")
    assert tuple(len(p) for p in pools) == M.FUSE_COUNTS
    got = _run_fuse(device, graph, pools, 1024, thr, mode)
    _check_fuse(got, pools, _fuse_reference("mixed", thr, mode), 1024)
    if mode == "vote":                                                       # the vote moved something, in every big case
        for i, p in enumerate(pools):
            assert len(p) < 63 or not np.array_equal(_bits(got[0][i, :len(p)]), _bits(p))


@pytest.mark.parametrize("mode", ["nms", "vote"])
def test_fuse_at_the_largest_pool_width(device, graph, mode):
    pools = _fuse_pools("wide")
    _check_fuse(_run_fuse(device, graph, pools, 4096, 0.2, mode), pools, _fuse_reference("wide", 0.2, mode), 4096)


@pytest.mark.parametrize("mode", ["nms", "vote"])
def test_fuse_hand_cases(device, graph, mode):
    pools = _fuse_pools("hand")
    assert {thr for _, thr in M.hand_cases().values()} == {0.2}
    got = _run_fuse(device, graph, pools, 8, 0.2, mode)
    _check_fuse(got, pools, _fuse_reference("hand", 0.2, mode), 8)
    names = list(M.hand_cases())
    chain, ties = names.index("chain"), names.index("ties")
    assert got[1][chain, :2].tolist() == [0, 2] and got[3][chain, :3].tolist() == [0, 0, 2]
    assert got[1][ties, :2].tolist() == [0, 2] and got[3][ties, :4].tolist() == [0, 0, 2, 2]


def test_fuse_status_codes_leave_the_outputs_alone(device):
    from tensorflow_ocr_amd import _lib as L
    n, max_pool = 2, 64
    pools = [M.cluster_case(40, 7)[0], M.cluster_case(64, 8)[0]]
    pool = np.zeros((n, max_pool, 9), f32)
    for i, p in enumerate(pools):
        pool[i, :len(p)] = p
    up = _up(device)
    pl, cnt = up(pool), up(np.array([40, 64], i32))
    fused = torch.full((n, max_pool, 9), float(SENT_F), dtype=torch.float32, device=device)
    outs = [torch.full(s, SENT_I, dtype=torch.int32, device=device) for s in ((n, max_pool), (n,), (n, max_pool))]
    size = L.call_size("ocr_quad_fuse_workspace", ctypes.c_int(n), ctypes.c_int(max_pool))
    ws = torch.zeros(size, dtype=torch.uint8, device=device)
    fn, p = L._fn("ocr_quad_fuse", ctypes.c_int), L.ptr

    def call(pl=pl, cnt=cnt, n=n, mp=max_pool, mode=0, fused=fused, keep=outs[0], nk=outs[1], owner=outs[2], ws=ws, size=size):
        return fn(p(pl), p(cnt), n, mp, ctypes.c_float(0.2), mode, p(fused), p(keep), p(nk), p(owner), p(ws),
                  ctypes.c_size_t(size), L.stream_ptr())
    for kw in (dict(pl=None), dict(cnt=None), dict(fused=None), dict(keep=None), dict(nk=None), dict(owner=None), dict(ws=None),
               dict(n=0), dict(mp=0), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == -1, kw
    assert call(mp=4097) == -2
    assert call(size=size - 1) == -4
    torch.cuda.synchronize()
    assert (fused == float(SENT_F)).all() and all((o == SENT_I).all() for o in outs)
    assert call(mode=1) == 0
    torch.cuda.synchronize()
    want = [M.fuse_ref(q, 0.2, "vote") for q in pools]
    assert outs[1].tolist() == [len(w[1]) for w in want]
    # all counts zero: fine, nothing kept
    assert call(cnt=up(np.zeros(n, i32))) == 0
    torch.cuda.synchronize()
    assert outs[1].tolist() == [0, 0] and (outs[2] == -1).all()


# ------------------------------------------------------------------------------------------------ detect_multiscale
def _plant(qh, qw, rects):
    """RBOX maps [qh,qw] (synthetic.rbox_labels' convention, angle 0) with the axis-aligned words `rects` = (x0, y0, x1, y1)
    in image pixels: score 1 inside, geo = distances to the top, right, bottom, left edge"""
    score, geo = np.zeros((qh, qw, 1), f32), np.zeros((qh, qw, 5), f32)
    ys, xs = np.mgrid[0:qh, 0:qw]
    px, py = 4.0 * xs, 4.0 * ys
    for x0, y0, x1, y1 in rects:
        inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        d = np.stack([py - y0, x1 - px, y1 - py, px - x0, np.zeros_like(px)], axis=-1)
        score[inside, 0] = 1.0
        geo[inside] = d[inside].astype(f32)
    return score, geo


def test_detect_multiscale_at_one_scale_equals_detect(device, graph):
    """scales = [1.0] on planted 48 x 64-cell maps: the quads of rbox.detect(box_thresh=...) divided by the ratios, the f32
    coordinates bit-equal — the same-threshold NMS over an already NMS'd list keeps everything — and only the score
    column differs (the mean pixel score instead of LANMS's sum).  The ratios are powers of two whose product is 1, so
    the divided quads have the areas, and the pair IoUs, of the undivided ones bit for bit."""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.tool import rbox
    rng = np.random.default_rng(123)
    s, g, _ = synthetic.rbox_labels(2, 256, rng, rects=4)
    score, geo = s[:, :48].copy(), g[:, :48].copy()                          # [2,48,64,..]
    score[0, 20:24, 30:34, 0] = 0.05                                         # a dent, so that not every mean is 1
    ratios = np.array([[2.0, 0.5], [1.0, 1.0]], f32)
    single = rbox.detect(score, geo, graph=graph, box_thresh=0.1)
    multi = rbox.detect_multiscale([(score, geo)], [torch.from_numpy(ratios).to(device)], box_thresh=0.1, graph=graph)
    assert len(single) == len(multi) == 2
    for i in range(2):
        assert len(single[i]) >= 2
        want = single[i][:, :8].astype(f32).copy()
        want[:, 0::2] /= ratios[i, 0]
        want[:, 1::2] /= ratios[i, 1]
        got = multi[i]
        assert got.shape == (len(want), 9)
        a = got[np.lexsort(got[:, :8].T[::-1])]
        b = want[np.lexsort(want.T[::-1])]
        assert np.array_equal(_bits(a[:, :8]), _bits(b)), i
        assert (np.diff(got[:, 8]) <= 0).all() and (got[:, 8] > 0.1).all() and (got[:, 8] <= 1).all()
        assert not np.array_equal(np.sort(got[:, 8]), np.sort(single[i][:, 8]))
    with pytest.raises(ValueError, match="max_pool"):
        rbox.detect_multiscale([(score, geo)], [torch.from_numpy(ratios).to(device)], graph=graph, max_pool=1)


# ------------------------------------------------------------------------------------------------ Evaluator
SCALES = [0.5, 1, 2]
SIDE = 128
BAND = (2.5, 7.5)             # a word shows at the scales where its height, in map cells, is inside this band


def _words(i):
    """image i's words (x0, y0, x1, y1) in original pixels: A (12 high: scales 1 and 2), B (6 high: scale 2 only), C (40 high:
    scale 0.5 only)"""
    dx = 4 * i
    return [(10 + dx, 10, 70 + dx, 22), (80, 40, 120, 46), (8, 70, 120 - dx, 110)]


def _stub_maps(i, side):
    """the maps a network "sees" for image i resized to side x side: every word whose height in cells is inside BAND, at its
    place at that scale; at scale 2 word A sits 2 original pixels off, as another scale's estimate would"""
    s = side / float(SIDE)
    rects = []
    for k, (x0, y0, x1, y1) in enumerate(_words(i)):
        if BAND[0] <= (y1 - y0) * s / 4.0 <= BAND[1]:
            off = 2 if (k == 0 and s == 2) else 0
            rects.append(((x0 + off) * s, (y0 + off) * s, (x1 + off) * s, (y1 + off) * s))
    return _plant(side // 4, side // 4, rects)


@pytest.fixture(scope="module")
def ms_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ms_eval"))
    rng = np.random.default_rng(9)
    for i in range(3):
        np.save(os.path.join(d, "img_%d.npy" % i), rng.integers(0, 256, (SIDE, SIDE, 3)).astype(np.uint8))
        with open(os.path.join(d, "gt_img_%d.txt" % i), "w") as f:
            for x0, y0, x1, y1 in _words(i):
                f.write("%d,%d,%d,%d,%d,%d,%d,%d,text\r\n" % (x0, y0, x1, y0, x1, y1, x0, y1))
    return d


def _stub_forward(device):
    """batches of 2 hold images 0 and 1, batches of 1 hold image 2 (name order, batch_size 2)"""
    calls = []

    def forward(x):
        calls.append(tuple(x.shape))
        ids = {2: [0, 1], 1: [2]}[x.shape[0]]
        maps = [_stub_maps(i, x.shape[1]) for i in ids]
        up = _up(device)
        return up(np.stack([m[0] for m in maps])), up(np.stack([m[1] for m in maps]))
    return forward, calls


def _host_composition(device, graph, d, fuse):
    """rbox.detect per scale -> ms_ref (append, fuse) -> the oracle matching: the record [num_gt, tp, fp, num_det]"""
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import rbox
    up = _up(device)
    want = np.zeros(4, np.int64)
    for i in range(3):
        pool, scale, counters = np.zeros((1024, 9), f32), np.zeros(1024, i32), [0, 0, 0]
        for s, (rh, rw) in enumerate(rbox.scale_sizes(SIDE, SIDE, SCALES)):
            score, geo = _stub_maps(i, rh)
            quads = rbox.detect(score[None], geo[None], graph=graph)[0]
            mean = torch.zeros((max(len(quads), 1),), dtype=torch.float32, device=device)
            if len(quads):
                ops.quad_mean_score(up(quads[:, :8].copy()), up(score[..., 0].copy()), 0.25, mean)
            M.append_ref(pool, scale, counters, np.concatenate([quads, np.zeros((1, 9), f32)]), np.arange(len(quads) + 1),
                         len(quads), None, mean.cpu().numpy(), np.array([rw / float(SIDE), rh / float(SIDE)], f32), s)
        assert counters[2] == 0 and counters[1] <= 1024
        fused, keep, _ = M.fuse_ref(pool[:counters[0]], 0.2, fuse)
        boxes = fused[keep, :8].astype(i32)
        gts, ign = evaluate.load_ground_truth(os.path.join(d, "img_%d.npy" % i))
        n_g, tp, fp = OE.bboxes_matching(boxes.reshape(-1, 8), gts[:, :, 0], gts[:, :, 1], ign, 0.5)
        want += [n_g, int(tp.sum()), int(fp.sum()), len(boxes)]
    return want.tolist()


@pytest.mark.parametrize("fuse", ["nms", "vote"])
def test_evaluator_multiscale_counts_equal_the_host_composition(device, graph, ms_dir, fuse):
    from tensorflow_ocr_amd import evaluate
    forward, calls = _stub_forward(device)
    ev = evaluate.Evaluator(graph, forward, ms_dir, batch_size=2, scales=SCALES, fuse=fuse)
    res = ev.run()
    assert sorted(calls) == sorted((n, s, s, 3) for n in (1, 2) for s in (64, 128, 256)) and ev.acc.reads == 1
    want = _host_composition(device, graph, ms_dir, fuse)
    print("multi-scale (%s): %s, host composition %s" % (fuse, evaluate.format_line(res), want))
    assert [res["num_gt"], res["tp"], res["fp"], res["num_det"]] == want
    # every word is found at some scale: 9 of 9; one scale sees word A only: 3 of 9
    assert res["tp"] == 9 and res["num_gt"] == 9 and res["recall"] == 1.0
    single = evaluate.Evaluator(graph, forward, ms_dir, batch_size=2).run()
    assert single["tp"] == 3 and single["num_gt"] == 9 and res["recall"] > single["recall"]
    assert ev.run() == res                                                   # a second pass starts from zero
    with pytest.raises(ValueError, match="max_pool = 1"):
        evaluate.Evaluator(graph, forward, ms_dir, batch_size=2, scales=SCALES, fuse=fuse, max_pool=1).run()
