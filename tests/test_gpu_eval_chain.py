"""GPU: the evaluation chain around the matcher — ocr_eval_collect against the float64 / NumPy restatement of
tests/test_eval_match_host.collect_ref (integers and copied scores: bit for bit), `evaluate.Evaluator` on synthetic images
against rbox.detect -> divide -> oracle/evalboxes.py per image (counter for counter, one read of the record per pass),
and the evaluation inside a training run: the recorded step's call list and the weights are the same with it and
without it."""
import os

import numpy as np
import pytest
import torch

import eval_support as E
import test_eval_match_host as H
from oracle import evalboxes as OE

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
SENT_I, SENT_F = -123456, f32(-12345.5)


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
@pytest.fixture(scope="module")
def eval_dir(graph, tmp_path_factory):
    return E.rbox_eval_dir(graph, str(tmp_path_factory.mktemp("eval")))


def test_evaluator_counts_equal_detect_divide_oracle(device, graph, eval_dir):
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import metrics, rbox
    d, maps, shapes = eval_dir
    forward, calls = E.rbox_stub_forward(device, maps)
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
def test_training_with_evaluation_records_the_same_step_and_trains_the_same_weights(device, tmp_path):
    d = str(tmp_path)
    E.write_training_eval_dir(d)
    calls0, kinds0, state0, _, _ = E.train_east_rbox(device, d, False)
    calls1, kinds1, state1, results, te = E.train_east_rbox(device, d, True)
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    for a, b in zip(state0, state1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # weights, moving statistics, EMA, Adam slots: bit for bit
    assert len(results) == 5 and te.passes == 5 and te.evaluator.acc.reads == 5            # two eager, the recorded, two replayed steps
    for r in results:
        assert r["images"] == 2 and r["num_gt"] == 2
        assert np.isfinite([r["precision"], r["recall"]]).all() and 0 <= r["precision"] <= 1 and 0 <= r["recall"] <= 1
