"""GPU: score-map fusion for the link geometry (csrc/map_fuse.hip) against the NumPy references of tests/mapfuse_ref.py.
ocr_link_map_accumulate must equal the float32 rule BIT FOR BIT when the rule is fed the device's own tap probabilities
(ocr_softmax_pairs / ocr_link_softmax_stack) — that is the test that decides; the float64 reference from logits bounds it
from outside.  Then the status codes, pixellink_fn.detect_device_multiscale against its parts, evaluate.LinkEvaluator's
map_scales / flip against the single-scale pass and against the same calls composed by hand, the script, and a training
run whose recorded step and weights are the same with a fused evaluation and without one."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import eval_support as E
import mapfuse_ref as R
from eval_support import EVAL, SHAPES            # the link directory: the eval size (a fusion grid of 32 x 32), the originals' (h, w)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


@pytest.fixture(scope="module")
def perm():
    return R.decode_perm()


def _up(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _logits(rng, n, hs, ws, spread=3.0):
    return rng.normal(0, spread, (n, hs, ws, 2)).astype(f32), rng.normal(0, spread, (n, hs, ws, 16)).astype(f32)


def _device_probs(device, graph, px, lk):
    """the device's own softmaxes of the logits, as the nine tap planes [9,n,hs,ws] (NumPy)"""
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    pp = P.pixel_scores(_up(device, px), graph=graph)
    lp = P.link_scores(_up(device, lk), graph=graph)
    return R.stack_probs(pp.cpu().numpy(), lp.cpu().numpy())


def _accumulate(device, px, lk, flip, weight, first, acc):
    from tensorflow_ocr_amd import ops
    ops.link_map_accumulate(_up(device, px), _up(device, lk), flip, weight, first, acc)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(i32)


def _gap(px, lk):
    return float(max(np.abs(px[..., 0] - px[..., 1]).max(), np.abs(lk[..., 0::2] - lk[..., 1::2]).max()))


# ------------------------------------------------------------------------------------------------ the kernel
def test_identity_equals_the_two_softmax_entries_bit_for_bit(device, graph):
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    rng = np.random.default_rng(21)
    px, lk = _logits(rng, 2, 7, 9)
    acc = torch.full((9, 2, 7, 9), -7.0, dtype=torch.float32, device=device)
    _accumulate(device, px, lk, False, 1.0, True, acc)
    pixel = P.pixel_scores(_up(device, px), graph=graph)[..., 1]
    link = P.link_scores(_up(device, lk), graph=graph)[..., 1]
    assert torch.equal(acc[0].view(torch.int32), pixel.contiguous().view(torch.int32))
    assert torch.equal(acc[1:].contiguous().view(torch.int32), link.contiguous().view(torch.int32))


GRIDS = [(7, 9), (8, 12), (1, 1), (5, 1)]
SOURCES = [(4, 6), (16, 24), (12, 20), (3, 17), (1, 1)]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_matrix_equals_the_float32_rule_on_the_device_probabilities(device, graph, perm, grid, capsys):
    hf, wf = grid
    worst = 0.0
    for si, (hs, ws) in enumerate(SOURCES):
        for n in (1, 3):
            rng = np.random.default_rng(1000 * si + 10 * n + hf)
            a, b = _logits(rng, n, hs, ws), _logits(rng, n, hs, ws)
            pa, pb = _device_probs(device, graph, *a), _device_probs(device, graph, *b)
            for flip in (0, 1):
                acc = torch.full((9, n, hf, wf), float("nan"), dtype=torch.float32, device=device)
                _accumulate(device, a[0], a[1], flip, 0.25, True, acc)
                first = acc.cpu().numpy()
                _accumulate(device, b[0], b[1], flip, 0.75, False, acc)
                got = acc.cpu().numpy()
                want1 = R.accumulate_f32(pa, hf, wf, flip, 0.25, True, perm=perm)
                want2 = R.accumulate_f32(pb, hf, wf, flip, 0.75, False, acc=want1, perm=perm)
                what = (grid, (hs, ws), n, flip)
                assert np.array_equal(_bits(first), _bits(want1)), what
                assert np.array_equal(_bits(got), _bits(want2)), what
                ref64 = R.accumulate_f64(a[0], a[1], hf, wf, flip, 0.25, True, perm=perm)
                ref64 = R.accumulate_f64(b[0], b[1], hf, wf, flip, 0.75, False, acc=ref64, perm=perm)
                bound = R.f64_bound(max(_gap(*a), _gap(*b)), hs, ws, 2)
                err = float(np.abs(got.astype(np.float64) - ref64).max())
                worst = max(worst, err / bound)
                assert err <= bound, (what, err, bound)
    with capsys.disabled():
        print("map fuse %dx%d: largest |device - float64| = %.3f of its bound" % (hf, wf, worst))


def test_flip_of_the_mirrored_logits_gives_the_identity_result(device, perm):
    rng = np.random.default_rng(33)
    px, lk = _logits(rng, 2, 7, 9)
    # the mirrored image's pass: columns reversed, and what it calls direction d is direction perm[d] of the original
    pxm = px[:, :, ::-1].copy()
    lkm = lk.reshape(2, 7, 9, 8, 2)[:, :, ::-1][:, :, :, perm].reshape(2, 7, 9, 16).copy()
    for hf, wf in ((7, 9), (5, 4), (10, 13)):
        one = torch.empty((9, 2, hf, wf), dtype=torch.float32, device=device)
        _accumulate(device, px, lk, False, 1.0, True, one)
        two = torch.empty_like(one)
        _accumulate(device, px, lk, False, 0.5, True, two)
        _accumulate(device, pxm, lkm, True, 0.5, False, two)
        assert torch.equal(one.view(torch.int32), two.view(torch.int32)), (hf, wf)      # v/2 + v/2 is v exactly


@pytest.mark.parametrize("flip", [0, 1])
def test_a_nan_logit_reaches_only_the_cells_that_sample_it(device, graph, perm, flip):
    rng = np.random.default_rng(44)
    px, lk = _logits(rng, 2, 4, 6)
    lk[1, 2, 3, 2 * 4 + 0] = np.nan                      # image 1, row 2, column 3, pair 4, its first logit
    probs = _device_probs(device, graph, px, lk)
    assert np.isnan(probs).sum() == 1 and np.isnan(probs[1 + 4, 1, 2, 3])
    for hf, wf in ((4, 6), (7, 9), (8, 12)):
        acc = torch.zeros((9, 2, hf, wf), dtype=torch.float32, device=device)
        _accumulate(device, px, lk, flip, 1.0, True, acc)
        got = acc.cpu().numpy()
        want = R.accumulate_f32(probs, hf, wf, flip, 1.0, True, perm=perm)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (hf, wf)
        plane = 1 + (perm.index(4) if flip else 4)
        where = np.argwhere(np.isnan(got))
        assert 1 <= len(where) <= 16 and set(where[:, 0]) == {plane} and set(where[:, 1]) == {1}, (hf, wf, where.tolist())
        if (hf, wf) == (4, 6):
            assert where.tolist() == [[plane, 1, 2, 2 if flip else 3]]
        assert np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)])


def test_grid_cap_the_loop_takes_the_cells_beyond_one_pass(device, graph, perm):
    rng = np.random.default_rng(55)
    px, lk = _logits(rng, 1, 300, 350)
    probs = _device_probs(device, graph, px, lk)
    acc = torch.full((9, 1, 600, 700), float("nan"), dtype=torch.float32, device=device)
    _accumulate(device, px, lk, 1, 0.5, True, acc)
    want = R.accumulate_f32(probs, 600, 700, 1, 0.5, True, perm=perm)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want))


def test_status_codes_and_nothing_written_on_error(device):
    from tensorflow_ocr_amd import _lib as L
    fn = L._fn("ocr_link_map_accumulate", ctypes.c_int)
    px = torch.zeros((2, 4, 6, 2), dtype=torch.float32, device=device)
    lk = torch.zeros((2, 4, 6, 16), dtype=torch.float32, device=device)
    acc = torch.full((9, 2, 7, 9), 1234.5, dtype=torch.float32, device=device)
    good = dict(px=L.ptr(px), lk=L.ptr(lk), n=2, hs=4, ws=6, flip=0, weight=0.5, first=1, acc=L.ptr(acc), hf=7, wf=9)

    def rc(**kw):
        a = dict(good, **kw)
        return int(fn(a["px"], a["lk"], ctypes.c_int(a["n"]), ctypes.c_int(a["hs"]), ctypes.c_int(a["ws"]), ctypes.c_int(a["flip"]),
                      ctypes.c_float(a["weight"]), ctypes.c_int(a["first"]), a["acc"], ctypes.c_int(a["hf"]), ctypes.c_int(a["wf"]),
                      L.stream_ptr()))
    invalid = [dict(px=None), dict(lk=None), dict(acc=None), dict(n=0), dict(n=-1), dict(hs=0), dict(ws=0), dict(hf=0),
               dict(wf=-3), dict(weight=0.0), dict(weight=-0.25), dict(weight=float("inf")), dict(weight=float("nan")),
               dict(lk=ctypes.c_void_p(lk.data_ptr() + 4))]
    for kw in invalid:
        assert rc(**kw) == -1, kw                                            # OCR_ERR_INVALID_ARG
    unsupported = [dict(n=65536), dict(n=2, hf=32768, wf=32768), dict(n=2, hs=32768, ws=32768), dict(n=65535, hf=256, wf=256)]
    for kw in unsupported:
        assert rc(**kw) == -2, kw                                            # OCR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((acc == 1234.5).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool((acc == 0.25).all())                                         # 0.5 * softmax(0, 0)[1]


# ------------------------------------------------------------------------------------------------ the planted words
BATCHES = [["img_a", "img_b"], ["img_c"]]        # the chains of a pass with batch_size 2, in order


def _at_scale(px, lk, side):
    """the planted logits as a network of that output size would give them: 64 = every cell repeated 2 x 2 (its 2 x 2 box
    mean is the 32 x 32 map again); 16 = the maximum text logit of every 2 x 2 block, so that a word keeps its extent"""
    if side == 32:
        return px, lk
    if side == 64:
        return np.repeat(np.repeat(px, 2, 0), 2, 1), np.repeat(np.repeat(lk, 2, 0), 2, 1)
    assert side == 16
    return px.reshape(16, 2, 16, 2, 2).max(axis=(1, 3)), lk[::2, ::2]


def _mirrored(px, lk, perm):
    n, h, w, _ = lk.shape
    return px[:, :, ::-1].copy(), lk.reshape(n, h, w, 8, 2)[:, :, ::-1][:, :, :, perm].reshape(n, h, w, 16).copy()


def _collect(device, five, max_d=None):
    """ocr_eval_collect on detect_device's five tensors with ratios (1, 1) -> (dets, det_score, nd) as NumPy"""
    from tensorflow_ocr_amd import ops
    merged, keep, n_keep, passed, _ = five
    n = merged.shape[0]
    max_d = max_d or ops.EVAL_MAX_D
    dets = torch.zeros((n, max_d, 4, 2), dtype=torch.int32, device=device)
    det_score = torch.zeros((n, max_d), dtype=torch.float32, device=device)
    nd = torch.zeros((n,), dtype=torch.int32, device=device)
    ops.eval_collect(merged, keep, n_keep, passed, torch.ones((n, 2), dtype=torch.float32, device=device), dets, det_score, nd,
                     torch.zeros_like(nd))
    return dets.cpu().numpy(), det_score.cpu().numpy(), nd.cpu().numpy()


@pytest.fixture(scope="module")
def eval_dir(device, graph, tmp_path_factory):
    """eval_support's link directory with the text logits a little stronger (P(text) in (0.95, 0.99)), so that a word's
    border survives the blend with the half-size map (see _at_scale); an image's first ground truth is its best
    single-scale detection, exactly."""
    from tensorflow_ocr_amd.tool import pixellink_fn as P

    def best_box(name, px, lk, h, w, n_regions):
        ps = P.pixel_scores(_up(device, px[None]), graph=graph)[..., 1].contiguous()
        ls = P.link_scores(_up(device, lk[None]), graph=graph)
        dets, _, nd = _collect(device, P.detect_device(ps, ls, 0.8, 0.9, 10, w / 32.0, h / 32.0, graph=graph))
        assert nd[0] == n_regions, name
        return dets[0, 0]
    return E.link_eval_dir(str(tmp_path_factory.mktemp("map_fuse_eval")), best_box, text=(3.0, 4.5))


def _stub_forward(device, maps, perm, flip=False):
    """the logits of the images a batch holds, by its size (2 = img_a, img_b; 1 = img_c), at the size the input asks for;
    with `flip` every second call of a shape is the mirrored pass and gets the mirrored logits"""
    calls, seen = [], {}

    def forward(x):
        key = tuple(x.shape)
        calls.append(key)
        k = seen[key] = seen.get(key, 0) + 1
        names = {2: ["img_a", "img_b"], 1: ["img_c"]}[x.shape[0]]
        scaled = [_at_scale(maps[nm][0], maps[nm][1], x.shape[1] // 4) for nm in names]
        px, lk = np.stack([s[0] for s in scaled]), np.stack([s[1] for s in scaled])
        if flip and k % 2 == 0:
            px, lk = _mirrored(px, lk, perm)
        return _up(device, px), _up(device, lk)
    return forward, calls


def _record(res):
    return [res["num_gt"], res["tp"], res["fp"], res["num_det"]]


def test_detect_device_multiscale_is_fusion_then_detect_device(device, graph, perm, eval_dir):
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    _, maps = eval_dir
    names = ["img_a", "img_b"]

    def passes():
        for side in (16, 32, 64):
            s = [_at_scale(maps[nm][0], maps[nm][1], side) for nm in names]
            px, lk = np.stack([v[0] for v in s]), np.stack([v[1] for v in s])
            yield _up(device, px), _up(device, lk), False
            pxm, lkm = _mirrored(px, lk, perm)
            yield _up(device, pxm), _up(device, lkm), True
    weights = [1, 1, 2, 2, 1, 1]
    ps, ls = P.fuse_score_maps(passes(), weights, (32, 32), graph=graph)
    assert tuple(ps.shape) == (2, 32, 32) and tuple(ls.shape) == (8, 2, 32, 32) and ps.is_contiguous() and ls.is_contiguous()
    assert ls.data_ptr() == ps.data_ptr() + ps.numel() * 4                    # two views of one accumulator
    want = P.detect_device(ps, ls, 0.8, 0.9, 10, 4.0, 3.0, max_comps=64, graph=graph)
    got = P.detect_device_multiscale(passes(), weights, (32, 32), 0.8, 0.9, 10, 4.0, 3.0, max_comps=64, graph=graph)
    torch.cuda.synchronize()
    assert got[2].tolist() == [2, 3]                                          # the planted words of the two images
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype == torch.float32 else a,
                                                  b.view(torch.uint8) if b.dtype == torch.float32 else b)
    # a pass is used up before the next one is asked for: a forward that reuses ONE output buffer gives the same maps
    buf = {}

    def reusing():
        for px, lk, flip in passes():
            key = tuple(px.shape)
            if key not in buf:
                buf[key] = (torch.empty_like(px), torch.empty_like(lk))
            buf[key][0].copy_(px)
            buf[key][1].copy_(lk)
            yield buf[key][0], buf[key][1], flip
    ps2, ls2 = P.fuse_score_maps(reusing(), weights, (32, 32), graph=graph)
    assert torch.equal(ps2.view(torch.int32), ps.view(torch.int32)) and torch.equal(ls2.view(torch.int32), ls.view(torch.int32))
    with pytest.raises(ValueError, match="forward passes"):
        P.fuse_score_maps(passes(), [1, 1], (32, 32), graph=graph)


def test_link_evaluator_at_the_identity_scale_returns_the_single_scale_record(device, graph, perm, eval_dir, monkeypatch):
    from tensorflow_ocr_amd import evaluate
    d, maps = eval_dir
    forward, _ = _stub_forward(device, maps, perm)
    kw = dict(batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL)
    single = evaluate.LinkEvaluator(graph, forward, d, **kw)
    assert single.map_scales is None and single.flip is False and type(single.detector) is evaluate.LinkSingleScale
    want = single.run()
    assert _record(want)[0] == 6 and want["tp"] >= 3 and want["num_det"] == 7 and want["images"] == 3
    forward, calls = _stub_forward(device, maps, perm)
    ev = evaluate.LinkEvaluator(graph, forward, d, map_scales=[1], **kw)
    assert ev.map_scales == [1.0] and ev.scale_weights == [1.0] and type(ev.detector) is evaluate.LinkFused
    reads = E.spy_reads(monkeypatch, calls)
    got = ev.run()
    monkeypatch.undo()
    assert got == want                                                        # weight 1 at the identity size: the softmaxes
    assert calls == [(2, EVAL, EVAL, 3), (1, EVAL, EVAL, 3)]
    assert ev.acc.reads == 1 and reads == [("cpu", 2)], reads                 # still one read of the device per pass
    # flip alone is scale 1 plus its mirror; the sweep rides along as before
    forward, calls = _stub_forward(device, maps, perm, flip=True)
    fl = evaluate.LinkEvaluator(graph, forward, d, flip=True, sweep=[0.5, 0.9], **kw)
    assert fl.map_scales == [1.0]
    res = fl.run()
    assert calls == [(2, EVAL, EVAL, 3)] * 2 + [(1, EVAL, EVAL, 3)] * 2
    assert _record(res) == _record(want) and len(res["sweep"]) == 2 and fl.acc.reads == 1


def test_link_evaluator_three_scales_with_flip_equals_the_calls_composed_by_hand(device, graph, perm, eval_dir):
    from tensorflow_ocr_amd import evaluate, ops
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    d, maps = eval_dir
    kw = dict(batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL)
    forward, calls = _stub_forward(device, maps, perm, flip=True)
    ev = evaluate.LinkEvaluator(graph, forward, d, map_scales=[0.5, 1, 2], flip=True, scale_weights=[1, 2, 1], max_comps=64, **kw)
    seen, match, detect = [], ev._match, ev.detector.detect

    def spy(*a):                                  # the rows the collect-and-match step is given ...
        seen[-1][:4] = [t.clone() for t in a[:4]]
        return match(*a)

    def spy_detect(*a):                           # ... and the detector's total: its overflow column is total - max_comps
        out = detect(*a)
        seen.append([None] * 4 + [out[5][:, 0] + ev.max_comps])
        return out
    ev._match, ev.detector.detect = spy, spy_detect
    res = ev.run()
    sizes = P.map_scale_sizes(EVAL, EVAL, [0.5, 1, 2])
    assert sizes == [(64, 64), (128, 128), (256, 256)]
    assert calls == [(n, s, s, 3) for n in (2, 1) for s, _ in sizes for _ in (0, 1)]      # per scale: as it is, then mirrored
    # by hand: resize from the originals, forward, accumulate with float32(w / sum w), decode once
    weights = P.pass_weights([1, 2, 1], flip=True)
    assert weights == [0.125, 0.125, 0.25, 0.25, 0.125, 0.125]
    hand_forward, _ = _stub_forward(device, maps, perm, flip=True)
    for names, got in zip(BATCHES, seen):
        h, w = SHAPES[names[0]]
        srcs = [_up(device, np.load(os.path.join(d, nm + ".npy"))) for nm in names]
        acc = torch.empty((9, len(names), EVAL // 4, EVAL // 4), dtype=torch.float32, device=device)
        k = 0
        for rh, rw in sizes:
            x = torch.empty((len(names), rh, rw, 3), dtype=torch.float32, device=device)
            for i, s in enumerate(srcs):
                ops.resize_linear_u8(s, x[i])
            for flip in (False, True):
                px, lk = hand_forward(torch.flip(x, dims=[2]) if flip else x)
                ops.link_map_accumulate(px, lk, flip, weights[k], k == 0, acc)
                k += 1
        want = P.detect_device(acc[0], acc[1:], 0.8, 0.9, 10, w / 32.0, h / 32.0, max_comps=64, graph=graph)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
            assert torch.equal(a.view(torch.uint8) if a.dtype == torch.float32 else a,
                               b.view(torch.uint8) if b.dtype == torch.float32 else b), names
    # the fused text mask is the single-scale one.  With weights 1/4, 1/2, 1/4 a fused score is 0.75 p + 0.25 q, p the
    # cell's own probability (the double-size map's 2 x 2 box mean is p again) and q the half-size map's sample.  Inside,
    # q >= 0.5625 p even at a corner that blends three outside cells (its own block of the half-size map is inside and
    # weighs 0.75 * 0.75): >= 0.89 * 0.95 > 0.8.  Outside: at most 0.75 * 0.12 + 0.25 < 0.8.  So the pass finds the planted
    # words, box for box
    single_forward, _ = _stub_forward(device, maps, perm)
    single = evaluate.LinkEvaluator(graph, single_forward, d, **kw).run()
    print("fused: %s | single scale: %s" % (evaluate.format_line(res), evaluate.format_line(single)))
    assert _record(res) == _record(single) and res["num_gt"] == 6 and res["tp"] >= 3 and res["num_det"] == 7
    assert ev.acc.reads == 1
    with pytest.raises(ValueError, match="max_comps"):                        # overflow still raises, at the end of the pass
        forward, _ = _stub_forward(device, maps, perm, flip=True)
        evaluate.LinkEvaluator(graph, forward, d, map_scales=[0.5, 1, 2], flip=True, max_comps=2, **kw).run()


def test_eval_pixellink_fast_runs_multi_scale_with_flip_on_graphed_forwards(device, tmp_path, capsys):
    """the script end to end: the flipped forward of a scale is the captured graph of the un-flipped one and returns the
    same buffers, which is why the fusion accumulates pass by pass"""
    sys.path.insert(0, ROOT)
    S = importlib.import_module("eval_pixellink_fast")
    d = str(tmp_path)
    for i in range(2):
        E.write_gt(os.path.join(d, "gt_synthetic_%d.txt" % i), [[8, 8, 40, 8, 40, 24, 8, 24], [30, 40, 60, 40, 60, 56, 30, 56]], ["text", "###"])
    S.main(["--synthetic", "2", "--gt_path", d, "--eval_image_height", "64", "--eval_image_width", "64", "--batch_size", "2",
            "--map_scales", "1,2", "--flip"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("precision ")]
    assert len(lines) == 1 and " recall " in lines[0] and " hmean " in lines[0] and "(gt 2 det " in lines[0], lines


# ------------------------------------------------------------------------------------------------ training
def test_training_with_a_fused_evaluation_records_the_same_step_and_trains_the_same_weights(device, tmp_path):
    d = str(tmp_path)
    E.write_training_eval_dir(d)
    calls0, kinds0, state0, _, _ = E.train_pixellink(device, d, None)
    calls1, kinds1, state1, results, te = E.train_pixellink(device, d, ["--eval_map_scales", "1,2", "--eval_flip"])
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    assert not [c for c in calls0 if c[1] == "ocr_link_map_accumulate"]     # ... and holds nothing of the evaluation
    for a, b in zip(state0, state1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # weights, auxiliaries, EMA: bit for bit
    assert len(results) == 4 and te.passes == 4 and te.evaluator.acc.reads == 4
    ev = te.evaluator
    assert type(ev).__name__ == "LinkEvaluator" and ev.map_scales == [1.0, 2.0] and ev.flip is True
    for r in results:
        assert r["images"] == 2 and r["num_gt"] == 2
        assert np.isfinite([r["precision"], r["recall"]]).all() and 0 <= r["precision"] <= 1 and 0 <= r["recall"] <= 1
