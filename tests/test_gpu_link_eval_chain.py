"""GPU: the link-geometry evaluation chain — pixellink_fn.detect_device -> ocr_eval_collect against the host path
(link_cc_decode -> min_area_rect_boxes, NumPy mean scores, stable descending sort), `evaluate.LinkEvaluator` on synthetic
images of two original shapes against the host path -> oracle/evalboxes.py (counter for counter, the device read only at
the end of the pass), the eval_pixellink_fast.py script on synthetic images, and the evaluation inside a
train_pixellink.py run: the recorded step's call list and the weights are the same with it and without it."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import eval_support as E
from eval_support import EVAL, SHAPES            # the link directory: the eval size, the originals' (h, w)
from oracle import evalboxes as OE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


def _painted(rng, regions, h=32, w=32):
    """pixel scores in (0.82, 0.99) inside the regions and below 0.5 outside: every region is one component"""
    inside = np.zeros((h, w), bool)
    for m in regions:
        inside |= m
    return np.where(inside, rng.uniform(0.82, 0.99, (h, w)), rng.uniform(0.0, 0.5, (h, w))).astype(f32)


# ------------------------------------------------------------------------------------------------ detect -> collect
def test_detect_device_and_collect_equal_the_host_path(device, graph):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    rng = np.random.default_rng(11)
    tiny = np.zeros((32, 32), bool)
    tiny[29:31, 1:3] = True                                                 # 4 pixels: dropped by min_size
    ps = np.stack([_painted(rng, [E.rot(32, 32, 8, 6, 6, 2, 0), E.rot(32, 32, 22, 12, 7, 2, 30), E.rot(32, 32, 10, 24, 4, 3, 0), tiny]),
                   _painted(rng, [E.rot(32, 32, 16, 16, 9, 3, -40)]),
                   _painted(rng, [])])
    link = np.full((8, 3, 32, 32), 0.95, f32)
    max_comps, max_d, min_size = 16, 8, 5
    for scale in ((4.0, 4.0), (5.0, 3.0)):
        want = E.host_detections(graph, torch.from_numpy(ps).to(device), torch.from_numpy(link).to(device), scale[0], scale[1],
                                min_size, max_comps)
        assert [len(b) for b, _ in want] == [3, 1, 0]
        merged, keep, n_keep, passed, total = P.detect_device(torch.from_numpy(ps).to(device), torch.from_numpy(link).to(device),
                                                              0.8, 0.9, min_size, scale[0], scale[1], max_comps=max_comps, graph=graph)
        n = 3
        dets = torch.zeros((n, max_d, 4, 2), dtype=torch.int32, device=device)
        det_score = torch.zeros((n, max_d), dtype=torch.float32, device=device)
        nd = torch.zeros((n,), dtype=torch.int32, device=device)
        nd_total = torch.zeros_like(nd)
        ops.eval_collect(merged, keep, n_keep, passed, torch.ones((n, 2), dtype=torch.float32, device=device), dets, det_score,
                         nd, nd_total)
        torch.cuda.synchronize()
        assert total.tolist() == [3, 1, 0] and n_keep.tolist() == [3, 1, 0] and nd.tolist() == [3, 1, 0] == nd_total.tolist()
        dets_h, score_h = dets.cpu().numpy(), det_score.cpu().numpy()
        for b, (bx, sc) in enumerate(want):
            assert np.array_equal(dets_h[b, :len(bx)], bx), (scale, b, dets_h[b, :len(bx)].tolist(), bx.tolist())
            assert np.array_equal(score_h[b, :len(bx)].view(i32), sc.view(i32)), (scale, b)
        assert len(set(score_h[0, :3].tolist())) == 3 and (np.diff(score_h[0, :3]) < 0).all()     # descending, no ties here


# ------------------------------------------------------------------------------------------------ LinkEvaluator
@pytest.fixture(scope="module")
def eval_dir(device, graph, tmp_path_factory):
    return E.link_eval_dir(str(tmp_path_factory.mktemp("link_eval")), E.host_best_box(graph, device))


def test_link_evaluator_counts_equal_host_path_and_oracle(device, graph, eval_dir, monkeypatch):
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import metrics
    d, maps = eval_dir
    want = np.zeros(4, np.int64)
    for name in sorted(maps):
        h, w = SHAPES[name]
        boxes, _ = E.host_image(graph, device, maps[name][0], maps[name][1], h, w)
        gts, ign = evaluate.load_ground_truth(os.path.join(d, name + ".npy"))
        n_g, tp, fp = OE.bboxes_matching(boxes.reshape(-1, 8), gts[:, :, 0], gts[:, :, 1], ign, 0.5)
        want += [n_g, int(tp.sum()), int(fp.sum()), len(boxes)]
    forward, calls = E.link_stub_forward(device, maps)
    ev = evaluate.LinkEvaluator(graph, forward, d, batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL)
    # every read of the device during the pass, with the number of chains launched before it
    reads = E.spy_reads(monkeypatch, calls)
    res = ev.run()
    monkeypatch.undo()
    assert sorted(calls) == [(1, EVAL, EVAL, 3), (2, EVAL, EVAL, 3)]       # both shapes enter at the eval size
    # one read of the device per pass — one copy holds the record and the overflow maxima — after the last chain was launched
    assert ev.acc.reads == 1 and reads == [("cpu", 2)], reads
    print("link evaluator: %s, oracle record %s" % (evaluate.format_line(res), want.tolist()))
    assert [res["num_gt"], res["tp"], res["fp"], res["num_det"]] == want.tolist()
    assert want[0] == 6 and want[1] >= 3 and want[3] == 7 and res["images"] == 3         # each image's best box is a true positive
    assert sorted(res) == sorted(["precision", "recall", "hmean", "num_gt", "tp", "fp", "num_det", "images"])
    assert (res["precision"], res["recall"]) == metrics.precision_recall(want[0], want[1], want[2])
    assert res["hmean"] == metrics.fmean(res["precision"], res["recall"])
    res2 = ev.run()                                                         # a second pass starts from zero
    assert res2 == res and ev.acc.reads == 2
    # the size filter reaches the boxes: nothing is 1000 pixels wide
    none = evaluate.LinkEvaluator(graph, forward, d, batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL, min_side=1000.0).run()
    assert none["num_det"] == 0 and none["num_gt"] == 6
    # too few component slots, too few detection slots: errors, read at the end of the pass
    with pytest.raises(ValueError, match="max_comps"):
        evaluate.LinkEvaluator(graph, forward, d, batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL, max_comps=2).run()
    with pytest.raises(ValueError, match="max_d"):
        evaluate.LinkEvaluator(graph, forward, d, batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL, max_d=1).run()


def test_eval_pixellink_fast_prints_the_line_for_synthetic_images(device, tmp_path, capsys):
    """the script end to end at the smallest size PixelLinkNet takes: two random images, ground truths under --gt_path"""
    sys.path.insert(0, ROOT)
    S = importlib.import_module("eval_pixellink_fast")
    d = str(tmp_path)
    for i in range(2):
        E.write_gt(os.path.join(d, "gt_synthetic_%d.txt" % i), [[8, 8, 40, 8, 40, 24, 8, 24], [30, 40, 60, 40, 60, 56, 30, 56]], ["text", "###"])
    S.main(["--synthetic", "2", "--gt_path", d, "--eval_image_height", "64", "--eval_image_width", "64", "--batch_size", "2"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("precision ")]
    assert len(lines) == 1 and " recall " in lines[0] and " hmean " in lines[0] and "(gt 2 det " in lines[0], lines


# ------------------------------------------------------------------------------------------------ training
def test_training_with_link_evaluation_records_the_same_step_and_trains_the_same_weights(device, tmp_path):
    d = str(tmp_path)
    E.write_training_eval_dir(d)
    calls0, kinds0, state0, _, _ = E.train_pixellink(device, d, None)
    calls1, kinds1, state1, results, te = E.train_pixellink(device, d, [])
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    for a, b in zip(state0, state1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # weights, auxiliaries, EMA: bit for bit
    assert len(results) == 4 and te.passes == 4 and te.evaluator.acc.reads == 4            # eager, recorded and replayed steps
    assert type(te.evaluator).__name__ == "LinkEvaluator"
    for r in results:
        assert r["images"] == 2 and r["num_gt"] == 2
        assert np.isfinite([r["precision"], r["recall"]]).all() and 0 <= r["precision"] <= 1 and 0 <= r["recall"] <= 1
