"""GPU: the decode-threshold grid of the link geometry end to end — pixellink_fn.detect_device_grid against detect_device
called once per point (all five tensors bit-equal per slice), `evaluate.LinkEvaluator(grid=...)` on the synthetic directory
of tests/eval_support.py against one plain `LinkEvaluator.run()` per point (every integer equal, every float ==, both
protocols), the top-level fields = row 0, the tie rule, grid_chunk, the per-point overflow, the grid behind flip fusion,
the single device read of a pass, and `TrainEval(grid=...)` inside a train_pixellink.py run: the three scalars, and the
recorded step's call list as it is without an evaluation."""
import types

import numpy as np
import pytest
import torch

import eval_support as E
from eval_support import EVAL

pytestmark = pytest.mark.gpu
f32 = np.float32
# pixel 0.5 decodes what the base pair's 0.8 decodes (P(text) is above 0.88 inside a region, below 0.12 outside): a tie;
# 0.93 and 0.97 cut into the regions; link 0.995 is above every link probability (0.993): no component survives min_size
GRID = ([0.5, 0.93, 0.97], [0.9, 0.995])
BASE = (0.8, 0.9)
POINTS = [BASE] + [(p, l) for p in GRID[0] for l in GRID[1]]
METRICS = ("precision", "recall", "hmean", "tp", "fp", "num_det", "num_gt")


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


@pytest.fixture(scope="module")
def eval_dir(device, graph, tmp_path_factory):
    return E.link_eval_dir(str(tmp_path_factory.mktemp("grid_eval")), E.host_best_box(graph, device))


def _evaluator(graph, forward, d, **kw):
    from tensorflow_ocr_amd import evaluate
    return evaluate.LinkEvaluator(graph, forward, d, batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL, **kw)


_PLAIN = {}


def plain_runs(graph, forward, d, protocol, **kw):
    """one plain pass per point, computed once per protocol and option set and shared"""
    key = (protocol,) + tuple(sorted(kw.items()))
    if key not in _PLAIN:
        _PLAIN[key] = [_evaluator(graph, forward, d, protocol=protocol, pixel_conf_threshold=p, link_conf_threshold=l, **kw).run()
                       for p, l in POINTS]
    return _PLAIN[key]


def _same_rows(res, plain):
    assert [(r["pixel_conf_threshold"], r["link_conf_threshold"]) for r in res["grid"]] == POINTS
    for row, want in zip(res["grid"], plain):
        assert "overflow" not in row
        for k in METRICS:
            assert type(row[k]) is type(want[k]) and row[k] == want[k], (row, want, k)
    assert {k: res[k] for k in plain[0]} == plain[0]                        # the top-level fields: the plain run, field for field
    assert {k: res[k] for k in METRICS} == {k: res["grid"][0][k] for k in METRICS}
    best = 0
    for k, row in enumerate(res["grid"]):
        if row["hmean"] > res["grid"][best]["hmean"]:
            best = k
    assert res["grid_best"] is res["grid"][best]


# ------------------------------------------------------------------------------------------------ detect_device_grid
def test_detect_device_grid_equals_detect_device_per_point(device, graph):
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    rng = np.random.default_rng(31)
    n, h, w, max_comps = 2, 48, 80, 128
    ps = torch.from_numpy(rng.uniform(size=(n, h, w)).astype(f32)).to(device)
    points = [(0.5, 0.5), (0.5, 0.8), (0.7, 0.3), (0.3, 0.9), (0.9, 0.1)]
    for link_shape in ((8, n, h, w), (8, n, h, w, 2)):
        lk = torch.from_numpy(rng.uniform(size=link_shape).astype(f32)).to(device)
        got = P.detect_device_grid(ps, lk, [p for p, _ in points], [l for _, l in points], 3, 4.0, 5.0, max_comps=max_comps,
                                   min_side=2.0, min_area=6.0, graph=graph)
        assert [t.shape[0] for t in got] == [len(points) * n] * 5
        totals = []
        for k, (p, l) in enumerate(points):
            want = P.detect_device(ps, lk, p, l, 3, 4.0, 5.0, max_comps=max_comps, min_side=2.0, min_area=6.0, graph=graph)
            for a, b in zip(got, want):
                s = a[k * n:(k + 1) * n]
                assert s.dtype == b.dtype and s.shape == b.shape
                assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, b.view(torch.int32) if b.dtype == torch.float32 else b), k
            totals.append(want[4].tolist())
        assert len({tuple(t) for t in totals}) == len(points) and min(min(t) for t in totals) > 0      # five different decodes
        assert max(max(t) for t in totals) > max_comps > min(min(t) for t in totals)                   # ... one beyond the table


# ------------------------------------------------------------------------------------------------ LinkEvaluator(grid=...)
@pytest.mark.parametrize("protocol", ["raster", "icdar15"])
def test_grid_rows_equal_plain_runs(device, graph, eval_dir, protocol, monkeypatch):
    d, maps = eval_dir
    forward, calls = E.link_stub_forward(device, maps)
    plain = plain_runs(graph, forward, d, protocol)
    del calls[:]
    ev = _evaluator(graph, forward, d, protocol=protocol, grid=GRID)
    reads = E.spy_reads(monkeypatch, calls)                                 # every read of the device during the pass
    res = ev.run()
    monkeypatch.undo()
    assert len(calls) == 2                                                  # one forward per batch, whatever the grid holds
    assert ev.acc.reads == 1 and reads == [("cpu", 2)], reads               # one read, after the last chain was launched
    _same_rows(res, plain)
    print("grid %s: %s" % (protocol, [(r["tp"], r["fp"], r["num_det"]) for r in res["grid"]]))
    rows = res["grid"]
    assert rows[1]["num_det"] == rows[0]["num_det"] > 0 and res["grid_best"] is rows[0]               # the tie: the lowest index
    assert rows[2]["num_det"] == rows[4]["num_det"] == rows[6]["num_det"] == 0                        # link 0.995: nothing is linked
    assert len({(r["tp"], r["fp"], r["num_det"]) for r in rows}) >= 2                                 # the grid changes the detection set
    assert ev.run() == res and ev.acc.reads == 2                            # a second pass starts from zero
    # chunking: one point per launch sequence, all points in one
    for chunk in (1, len(POINTS)):
        assert _evaluator(graph, forward, d, protocol=protocol, grid=GRID, grid_chunk=chunk).run() == res, chunk


def test_overflow_is_per_point(device, graph, eval_dir):
    """min_size = 0 and link 0.995: every pixel above 0.5 is a component of its own, far more than max_comps = 8; the two
    other rows hold the regions (2 or 3 per image).  The pass goes on; with that point as the base pair it raises."""
    d, maps = eval_dir
    forward, _ = E.link_stub_forward(device, maps)
    kw = dict(min_size=0, max_comps=8)
    grid = ([0.5], [0.9, 0.995])
    res = _evaluator(graph, forward, d, grid=grid, **kw).run()
    rows = res["grid"]
    assert [("overflow" in r) for r in rows] == [False, False, True]
    assert rows[2]["overflow"] > 20 and all(rows[2][k] is None for k in METRICS) and res["grid_best"] is rows[0]
    for row, (p, l) in zip(rows[:2], (BASE, (0.5, 0.9))):
        want = _evaluator(graph, forward, d, pixel_conf_threshold=p, link_conf_threshold=l, **kw).run()
        assert {k: row[k] for k in METRICS} == {k: want[k] for k in METRICS} and want["num_det"] == 7
    with pytest.raises(ValueError, match="components more than max_comps = 8"):
        _evaluator(graph, forward, d, grid=([0.8], [0.9]), pixel_conf_threshold=0.5, link_conf_threshold=0.995, **kw).run()


def test_grid_behind_flip_fusion_equals_the_fused_evaluator_per_point(device, graph, eval_dir):
    d, maps = eval_dir
    forward, calls = E.link_stub_forward(device, maps)
    plain = plain_runs(graph, forward, d, "raster", flip=True)
    del calls[:]
    res = _evaluator(graph, forward, d, grid=GRID, flip=True).run()
    assert len(calls) == 4                                                  # two batches, each once and once mirrored
    _same_rows(res, plain)


# ------------------------------------------------------------------------------------------------ training
def test_training_with_a_grid_records_the_same_step_and_writes_the_three_scalars(device, tmp_path):
    d = str(tmp_path)
    E.write_training_eval_dir(d)
    calls0, kinds0, _, _, _ = E.train_pixellink(device, d, None, steps=3)
    calls1, kinds1, _, results, te = E.train_pixellink(device, d, ["--eval_grid_pixel", "0.5,0.7", "--eval_grid_link", "0.5,0.9"],
                                                       steps=3)
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    assert len(results) == 3 and te.evaluator.acc.reads == 3
    for r in results:
        assert len(r["grid"]) == 5 and r["grid_best"] in r["grid"]
        assert (r["grid"][0]["pixel_conf_threshold"], r["grid"][0]["link_conf_threshold"]) == (0.8, 0.9)
    scalars = {}
    te.write(types.SimpleNamespace(add_scalar=lambda k, v: scalars.__setitem__(k, v), flush_step=lambda s: None), 3)
    best = te.last["grid_best"]
    assert sorted(scalars) == sorted(["eval/precision", "eval/recall", "eval/hmean", "eval/grid_best_hmean",
                                      "eval/grid_best_pixel_threshold", "eval/grid_best_link_threshold"])
    assert scalars["eval/grid_best_hmean"] == best["hmean"] and scalars["eval/grid_best_pixel_threshold"] == best["pixel_conf_threshold"]
    assert scalars["eval/grid_best_link_threshold"] == best["link_conf_threshold"]
