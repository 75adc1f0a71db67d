"""GPU: the evaluation chain around the matcher — ocr_eval_collect against the float64 / NumPy restatement of
tests/test_eval_match_host.collect_ref (integers and copied scores: bit for bit), `evaluate.Evaluator` on synthetic images
against rbox.detect -> divide -> oracle/evalboxes.py per image (counter for counter, one read of the record per pass),
and the evaluation inside a training run: the recorded step's call list and the weights are the same with it and
without it."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import test_eval_match_host as H
from oracle import evalboxes as OE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32
SENT_I, SENT_F = -123456, f32(-12345.5)
SMALL = [("block1", [(128, 64, 1), (128, 64, 2)]), ("block2", [(256, 64, 1), (256, 64, 2)]),
         ("block3", [(256, 128, 1), (256, 128, 2)]), ("block4", [(512, 128, 1)])]


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


# ------------------------------------------------------------------------------------------------ collect
def _collect_case(n, max_k, n_keep, seed, with_mask):
    rng = np.random.default_rng(seed)
    merged = rng.uniform(-500, 500, (n, max_k, 9)).astype(f32)
    merged[..., 8] = rng.choice(np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.25], f32), (n, max_k))      # ties in score
    merged[0, 3, 2], merged[0, 4, 8] = np.nan, np.nan                      # a NaN coordinate, a NaN score
    merged[1, 5, 0], merged[1, 6, 1], merged[1, 7, 7] = np.inf, -np.inf, 3e7
    keep = np.stack([rng.permutation(max_k) for _ in range(n)]).astype(i32)
    keep[0, :5] = [3, 4, 0, 1, 2]                                          # the NaN rows are kept
    keep[1, :3] = [5, 6, 7]
    keep[n - 1, 1] = max_k + 3                                             # an index outside the list: dropped
    passed = (rng.uniform(0, 1, (n, max_k)) < 0.7) if with_mask else None
    if with_mask:
        passed[0, :5] = True
    ratio = np.array([[0.75, 1.5], [1.0, 1.0], [1.5, 0.75]], f32)[np.arange(n) % 3]
    return merged, keep, np.asarray(n_keep, i32), passed, ratio


@pytest.mark.parametrize("max_k,n_keep,max_d,with_mask", [
    (40, [30, 0, 40], 16, True),                 # overflow (more than max_d pass), an empty image, a mask with holes
    (40, [12, 9, 41], 16, False),                # no mask; n_keep beyond max_k is clamped
    (600, [520, 257, 256], 1024, True),          # more than one 256-row chunk, and the chunk edges
])
def test_collect_equals_the_host_restatement(device, max_k, n_keep, max_d, with_mask):
    from tensorflow_ocr_amd import ops
    n = 3
    merged, keep, nk, passed, ratio = _collect_case(n, max_k, n_keep, 100 + max_k + max_d, with_mask)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dets = torch.full((n + 1, max_d, 4, 2), SENT_I, dtype=torch.int32, device=device)
    score = torch.full((n + 1, max_d), float(SENT_F), dtype=torch.float32, device=device)
    nd = torch.full((n + 1,), SENT_I, dtype=torch.int32, device=device)
    tot = torch.full((n + 1,), SENT_I, dtype=torch.int32, device=device)
    ops.eval_collect(up(merged), up(keep), up(nk), None if passed is None else up(passed.astype(np.uint8)), up(ratio),
                     dets[:n], score[:n], nd[:n], tot[:n])
    torch.cuda.synchronize()
    dets_h, score_h, nd_h, tot_h = dets.cpu().numpy(), score.cpu().numpy(), nd.cpu().numpy(), tot.cpu().numpy()
    overflowed = 0
    for i in range(n):
        rd, rs, rt = H.collect_ref(merged[i], keep[i], nk[i], None if passed is None else passed[i], ratio[i], max_d)
        assert tot_h[i] == rt and nd_h[i] == min(rt, max_d) == len(rd), i
        assert np.array_equal(dets_h[i, :len(rd)], rd), i
        assert np.array_equal(score_h[i, :len(rd)].view(i32), rs.view(i32)), i          # bit for bit, NaN included
        assert (dets_h[i, len(rd):] == SENT_I).all() and (score_h[i, len(rd):] == SENT_F).all()     # nothing beyond nd
        overflowed += rt > max_d
    assert (dets_h[n] == SENT_I).all() and nd_h[n] == SENT_I and tot_h[n] == SENT_I
    assert (overflowed >= 1) == (max_d == 16)                               # the small max_d cases include the overflow


def test_collect_status_codes_leave_the_outputs_alone(device):
    import ctypes
    from tensorflow_ocr_amd import _lib as L
    n, max_k, max_d = 3, 40, 16
    merged, keep, nk, _, ratio = _collect_case(n, max_k, [5, 5, 5], 9, False)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    m, k, c, r = up(merged), up(keep), up(nk), up(ratio)
    dets = torch.full((n, max_d, 4, 2), SENT_I, dtype=torch.int32, device=device)
    score = torch.full((n, max_d), float(SENT_F), dtype=torch.float32, device=device)
    nd = torch.full((2, n), SENT_I, dtype=torch.int32, device=device)
    fn, p = L._fn("ocr_eval_collect", ctypes.c_int), L.ptr

    def call(m=m, k=k, c=c, r=r, n=n, mk=max_k, md=max_d, dets=dets, score=score, nd=nd[0], tot=nd[1]):
        return fn(p(m), p(k), p(c), p(None), p(r), n, mk, md, p(dets), p(score), p(nd), p(tot), L.stream_ptr())
    for kw in (dict(m=None), dict(k=None), dict(c=None), dict(r=None), dict(dets=None), dict(score=None), dict(nd=None),
               dict(tot=None), dict(n=0), dict(mk=0), dict(md=0)):
        assert call(**kw) == -1, kw
    assert call(md=1025) == -2 and call(n=65536) == -2
    torch.cuda.synchronize()
    assert (dets == SENT_I).all() and (score == float(SENT_F)).all() and (nd == SENT_I).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert nd[0].tolist() == [5, 5, 4] and nd[1].tolist() == [5, 5, 4]      # (the last image's second index is outside the list)


# ------------------------------------------------------------------------------------------------ Evaluator
def _write_gt(path, quads, tags):
    with open(path, "w") as f:
        for q, t in zip(quads, tags):
            f.write(",".join(str(int(v)) for v in np.asarray(q).reshape(-1)) + "," + t + "\r\n")


@pytest.fixture(scope="module")
def eval_dir(device, graph, tmp_path_factory):
    """3 images (two 64 x 64, one 96 wide x 64 high) with label maps from synthetic.rbox_labels and ground truths made from
    what the detector finds on them: the best detection exactly, an ignored quad, and one nothing matches."""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.tool import rbox
    d = str(tmp_path_factory.mktemp("eval"))
    rng = np.random.default_rng(77)
    s64, g64, _ = synthetic.rbox_labels(2, 64, rng, rects=2)
    s96, g96, _ = synthetic.rbox_labels(1, 96, rng, rects=3)
    maps = {"img_a": (s64[0], g64[0]), "img_b": (s64[1], g64[1]), "img_c": (s96[0, :16], g96[0, :16])}      # [16,24] for 64 x 96
    shapes = {"img_a": (64, 64), "img_b": (64, 64), "img_c": (64, 96)}
    for name, (h, w) in shapes.items():
        np.save(os.path.join(d, name + ".npy"), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        quads = rbox.detect(maps[name][0][None], maps[name][1][None], graph=graph)[0]
        assert len(quads) >= 1, name
        best = quads[np.argsort(-quads[:, 8], kind="stable")[0], :8].astype(i32)
        _write_gt(os.path.join(d, "gt_%s.txt" % name), [best, H.rect(1, 1, 9, 6), H.rect(50, 2, 62, 9)], ["text", "###", "far"])
    return d, maps, shapes


def _stub_forward(device, maps):
    """the maps of the images a batch holds, by its shape: (2, 64, 64) = img_a, img_b in name order; (1, 64, 96) = img_c"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    calls = []

    def forward(x):
        calls.append(tuple(x.shape))
        names = {(2, 64, 64, 3): ["img_a", "img_b"], (1, 64, 96, 3): ["img_c"]}[tuple(x.shape)]
        return up(np.stack([maps[k][0] for k in names])), up(np.stack([maps[k][1] for k in names]))
    return forward, calls


def test_evaluator_counts_equal_detect_divide_oracle(device, graph, eval_dir):
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import metrics, rbox
    d, maps, shapes = eval_dir
    forward, calls = _stub_forward(device, maps)
    ev = evaluate.Evaluator(graph, forward, d, batch_size=2)
    res = ev.run()
    assert sorted(calls) == [(1, 64, 96, 3), (2, 64, 64, 3)] and ev.acc.reads == 1         # one read of the record per pass
    want = np.zeros(4, np.int64)
    for name in sorted(maps):
        quads = rbox.detect(maps[name][0][None], maps[name][1][None], graph=graph)[0]
        quads = quads[np.argsort(-quads[:, 8], kind="stable")]
        h, w = shapes[name]
        rh, rw = evaluate.resize_rule(h, w)
        boxes = quads[:, :8].reshape(-1, 4, 2).astype(f32)
        boxes[:, :, 0] /= f32(rw / float(w))
        boxes[:, :, 1] /= f32(rh / float(h))
        boxes = boxes.astype(i32)
        gts, ign = evaluate.load_ground_truth(os.path.join(d, name + ".npy"))
        n_g, tp, fp = OE.bboxes_matching(boxes.reshape(-1, 8), gts[:, :, 0], gts[:, :, 1], ign, 0.5)
        want += [n_g, int(tp.sum()), int(fp.sum()), len(boxes)]
    print("evaluator: %s, oracle record %s" % (evaluate.format_line(res), want.tolist()))
    assert [res["num_gt"], res["tp"], res["fp"], res["num_det"]] == want.tolist()
    assert want[1] >= 3 and want[0] == 6 and res["images"] == 3            # each image's best detection is a true positive
    assert (res["precision"], res["recall"]) == metrics.precision_recall(want[0], want[1], want[2])
    assert res["hmean"] == metrics.fmean(res["precision"], res["recall"])
    res2 = ev.run()                                                         # a second pass starts from zero
    assert res2 == res and ev.acc.reads == 2
    # an overflow of the detection list is an error, read at the end of the pass
    with pytest.raises(ValueError, match="max_d"):
        evaluate.Evaluator(graph, forward, d, batch_size=2, max_d=1, nms_thres=0.99).run()


# ------------------------------------------------------------------------------------------------ training
def _train(device, eval_dir_path, with_eval, steps=5):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    sys.path.insert(0, ROOT)
    T = importlib.import_module("multigpu_train")
    argv = ["--net", "east", "--geometry", "RBOX", "--input_size", "64", "--batch_size_per_gpu", "2"]
    if with_eval:
        argv += ["--eval_steps", "1", "--eval_data_path", eval_dir_path]
    FLAGS = T.parse(argv)
    rng = np.random.default_rng(51)
    images = rng.uniform(0, 255, (2, 64, 64, 3)).astype(f32)
    batch = [torch.from_numpy(a).to(device) for a in (images,) + tuple(synthetic.rbox_labels(2, 64, rng))]

    def fl(gr, im, yy, gg, mm):
        a, b = M.model_rbox(im, text_scale=FLAGS.text_scale, graph=gr, blocks=SMALL)
        return M.loss_rbox(yy, a, gg, b, mm, graph=gr)
    g = Graph(device, loss_scale=1024.0, seed=6)
    step = TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3))
    te = T.make_train_eval(FLAGS, g, step, blocks=SMALL)
    assert (te is not None) == with_eval
    results = []
    for it in range(steps):
        step(*batch)
        if te is not None and te.due(it + 1):
            T._evaluate(te, None, step.opt)
            results.append(te.last)
    torch.cuda.synchronize()
    assert step.plan is not None
    calls = [(e[0], e[3] if e[0] == "c" else (e[2] if len(e) > 2 else None)) for e in step.recorded]      # C entry names, host entry tags
    state = [t.clone() for t in (g.store.flat, g.store.flat_aux, step.opt.ema, step.opt.m, step.opt.v)]
    return calls, list(step.plan_kinds), state, results, te


def test_training_with_evaluation_records_the_same_step_and_trains_the_same_weights(device, tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(5)
    for name in ("img_1", "img_2"):
        np.save(os.path.join(d, name + ".npy"), rng.integers(0, 256, (64, 64, 3)).astype(np.uint8))
        _write_gt(os.path.join(d, "gt_%s.txt" % name), [H.rect(8, 8, 40, 24), H.rect(30, 40, 60, 56)], ["text", "###"])
    calls0, kinds0, state0, _, _ = _train(device, d, False)
    calls1, kinds1, state1, results, te = _train(device, d, True)
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    for a, b in zip(state0, state1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # weights, moving statistics, EMA, Adam slots: bit for bit
    assert len(results) == 5 and te.passes == 5 and te.evaluator.acc.reads == 5            # two eager, the recorded, two replayed steps
    for r in results:
        assert r["images"] == 2 and r["num_gt"] == 2
        assert np.isfinite([r["precision"], r["recall"]]).all() and 0 <= r["precision"] <= 1 and 0 <= r["recall"] <= 1
