"""CPU: what one evaluation pass launches, call for call, against tests/golden/eval_pass_trace.json — recorded by
tests/golden/make_eval_pass_trace.py from THIS file on the commit from before evaluate.py was split into a pass driver and
four detectors.  Every device entry the pass reaches is replaced by a recorder on a CPU "graph" (the entries themselves
are what the GPU tests hold to their references): the resize, the forwards, the detect tools, the collect step, both
matchers, the record and the curve.  The recorder keeps every call in order — its name, tensor arguments as (shape,
dtype), the small ones (ratios, weights) by value, scalars by value, and for the read of the pass the number of values
read — and each case's result.  The overflow cases pin the order in which the limits are reported: a detector's columns
first, in its own order, then max_d.

The issue's RBOX multi-scale case (scales 0.5, 1, 2 on 96-pixel-high images) is refused by the sizing rule at scale 0.5
(48 rows -> 0); the trace keeps it as the error it is, and `rbox_ms_*_07` run the same pass at scales 0.7, 1, 2."""
import contextlib
import json
import os
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "eval_pass_trace.json")
SHAPES = {"a": (96, 128), "b": (96, 160), "c": (96, 128), "d": (96, 128), "e": (96, 160)}
QUADS = {"a": ([[4, 4, 40, 4, 40, 20, 4, 20]], ["text"]),
         "b": ([[8, 8, 60, 8, 60, 30, 8, 30], [70, 40, 150, 40, 150, 60, 70, 60]], ["text", "###"]),
         "c": ([[10, 50, 90, 50, 90, 80, 10, 80], [2, 2, 30, 2, 30, 12, 2, 12], [100, 10, 120, 10, 120, 90, 100, 90]], ["a", "b", "c"]),
         "d": ([[20, 20, 100, 20, 100, 70, 20, 70]], ["text"]),
         "e": ([[5, 5, 155, 5, 155, 90, 5, 90], [40, 30, 80, 30, 80, 50, 40, 50]], ["text", "text"])}
LINK = dict(eval_image_height=128, eval_image_width=256, max_comps=64)
CASES = {
    "rbox": ("Evaluator", {}),
    "rbox_box_thresh": ("Evaluator", dict(box_thresh=0.1)),
    "rbox_ms_nms": ("Evaluator", dict(scales=[0.5, 1, 2], fuse="nms")),
    "rbox_ms_vote": ("Evaluator", dict(scales=[0.5, 1, 2], fuse="vote")),
    "rbox_ms_nms_07": ("Evaluator", dict(scales=[0.7, 1, 2], fuse="nms", box_thresh=0.1, max_k=32, max_pool=48)),
    "rbox_ms_vote_07": ("Evaluator", dict(scales=[0.7, 1, 2], fuse="vote")),
    "link": ("LinkEvaluator", dict(LINK)),
    "link_fused": ("LinkEvaluator", dict(LINK, map_scales=[0.5, 1, 2], flip=True, scale_weights=[1, 2, 1])),
    "link_flip": ("LinkEvaluator", dict(LINK, flip=True)),
}
PROTOCOLS, SWEEPS = ("raster", "icdar15"), (None, [0.5, 0.9])
# the overflow cases: per detector, the value of each of its overflow columns (None: below the limit) and of max_d's
DETECTORS = {"rbox": 1, "rbox_ms_nms_07": 3, "link": 1, "link_fused": 1}


def overflow_cases():
    for case, m in DETECTORS.items():
        sets = [(i,) for i in range(m)] + ([(0, 1), (0, 2), (1, 2)] if m == 3 else [])
        for cols in sets:
            yield case, cols, False
        yield case, (), True
        for i in range(m):
            yield case, (i,), True


def write_dir(d):
    for name, (h, w) in SHAPES.items():
        np.save(os.path.join(d, name + ".npy"), np.zeros((h, w, 3), np.uint8))
        with open(os.path.join(d, "gt_%s.txt" % name), "w") as f:
            for q, t in zip(*QUADS[name]):
                f.write(",".join(str(v) for v in q) + "," + t + "\r\n")


def _desc(t):
    return None if t is None else [list(t.shape), str(t.dtype).replace("torch.", "")]


def _val(t):
    return _desc(t) + [t.tolist()]


class Recorder:
    """the stubs of one pass.  `over`: column index -> by how much image 0 of every chain exceeds that limit of the
    detector (7 + the index); `over_d`: the same for max_d (by 2).  Every other count lies 3 below its limit."""

    def __init__(self, geometry, over=(), over_d=False):
        self.log, self.geometry, self.over, self.over_d = [], geometry, tuple(over), over_d

    def _count(self, n, limit, column):
        t = torch.full((n,), limit - 3, dtype=torch.int32)
        if column in self.over:
            t[0] = limit + 7 + column
        return t

    def forward(self, x):
        self.log.append(["forward", _desc(x)])
        n, h, w, _ = x.shape
        a, b = (1, 5) if self.geometry == "Evaluator" else (2, 16)
        return torch.zeros((n, h // 4, w // 4, a)), torch.zeros((n, h // 4, w // 4, b))

    def resize(self, src, dst):
        self.log.append(["resize_linear_u8", _desc(src), _desc(dst)])
        dst.zero_()

    def _five(self, n, k, with_mask, column=0):
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)
        return (z(n, k, 9, dt=torch.float32), z(n, k), z(n), z(n, k, dt=torch.bool) if with_mask else None,
                self._count(n, k, column))

    def rbox_detect(self, score_map, geo_map, score_map_thresh=0.8, nms_thres=0.2, max_k=None, graph=None, box_thresh=None):
        self.log.append(["rbox.detect_device", _desc(score_map), _desc(geo_map), score_map_thresh, nms_thres, max_k, box_thresh])
        return self._five(score_map.shape[0], 16 if max_k is None else max_k, box_thresh is not None)

    def rbox_multiscale(self, maps, ratios, score_map_thresh=0.8, nms_thres=0.2, box_thresh=None, fuse="nms", fuse_thres=None,
                        max_pool=1024, max_k=None, graph=None):
        self.log.append(["rbox.detect_multiscale_device", [_val(r) for r in ratios], score_map_thresh, nms_thres, box_thresh,
                         fuse, fuse_thres, max_pool, max_k])
        n = 0
        for score_map, geo_map in maps:                     # a scale's forward runs here, when it is asked for
            self.log.append(["scale maps", _desc(score_map), _desc(geo_map)])
            n = score_map.shape[0]
        fused, keep, n_keep, _, _ = self._five(n, max_pool, False)
        return fused, keep, n_keep, torch.stack([self._count(n, 0, c) for c in range(3)], dim=1)

    def pixel_scores(self, t, graph=None):
        self.log.append(["pixellink_fn.pixel_scores", _desc(t)])
        return torch.zeros(tuple(t.shape))

    def link_scores(self, t, graph=None):
        self.log.append(["pixellink_fn.link_scores", _desc(t)])
        return torch.zeros((8,) + tuple(t.shape[:3]) + (2,))

    def link_detect(self, pixel_score, link_score, pixel_conf_threshold=0.8, link_conf_threshold=0.9, min_size=10, scale_x=4.0,
                    scale_y=4.0, max_comps=4096, min_side=0.0, min_area=0.0, graph=None):
        self.log.append(["pixellink_fn.detect_device", _desc(pixel_score), _desc(link_score), pixel_conf_threshold,
                         link_conf_threshold, min_size, scale_x, scale_y, max_comps, min_side, min_area])
        return self._five(pixel_score.shape[0], max_comps, True)

    def link_multiscale(self, passes, weights, out_hw, pixel_conf_threshold=0.8, link_conf_threshold=0.9, min_size=10,
                        scale_x=4.0, scale_y=4.0, max_comps=4096, min_side=0.0, min_area=0.0, graph=None):
        self.log.append(["pixellink_fn.detect_device_multiscale", [float(w) for w in weights], list(out_hw), pixel_conf_threshold,
                         link_conf_threshold, min_size, scale_x, scale_y, max_comps, min_side, min_area])
        n = 0
        for pixel_cls, link_cls, flip in passes:           # a pass's forward runs here, when it is asked for
            self.log.append(["pass", _desc(pixel_cls), _desc(link_cls), bool(flip)])
            n = pixel_cls.shape[0]
        return self._five(n, max_comps, True)

    def collect(self, merged, keep, n_keep, passed, inv_ratio, dets, det_score, nd, nd_total):
        self.log.append(["ops.eval_collect", _desc(merged), _desc(keep), _desc(n_keep), _desc(passed), _val(inv_ratio),
                         _desc(dets), _desc(det_score), _desc(nd), _desc(nd_total)])
        dets.zero_()
        det_score.zero_()
        nd.fill_(1)
        nd_total.copy_(torch.full_like(nd_total, dets.shape[1] - 3))
        if self.over_d:
            nd_total[0] = dets.shape[1] + 2

    def match_raster(self, dets, nd, gts, ng, gign, thr, record=None, graph=None, mask_hw=None):
        self.log.append(["bboxes.bboxes_matching_batch", _desc(dets), _desc(nd), _val(gts), _val(ng), _val(gign), thr,
                         list(mask_hw)])
        record += torch.tensor([int(ng.sum()), int(nd.sum()), 1, int(nd.sum()) + 1])
        n, max_d = dets.shape[:2]
        return torch.zeros((n, max_d), dtype=torch.uint8), torch.zeros((n, max_d), dtype=torch.uint8), None

    def match_ic15(self, dets, nd, gts, ng, gign, thr, area_thr, record=None, graph=None):
        self.log.append(["bboxes.ic15_matching_batch", _desc(dets), _desc(nd), _val(gts), _val(ng), _val(gign), thr, area_thr])
        record += torch.tensor([int(ng.sum()) - int(gign.sum()), int(nd.sum()), 1, int(nd.sum()) + 1])
        n, max_d = dets.shape[:2]
        return torch.zeros((n, max_d), dtype=torch.int32), torch.zeros((n, gts.shape[1]), dtype=torch.int32), None

    def acc_class(rec):
        class Acc:
            def __init__(self, graph=None):
                self.record, self.reads = torch.zeros(4, dtype=torch.int64), 0
                rec.log.append(["metrics.DeviceTpFp"])

            def reset(self):
                rec.log.append(["acc.reset"])
                self.record.zero_()

            def value_with(self, extra):
                self.reads += 1
                rec.log.append(["acc.value_with", 4 + extra.numel()])
                return tuple(int(v) for v in self.record.tolist()), [int(v) for v in extra.reshape(-1).tolist()]
        return Acc

    def curve_class(rec):
        class Curve:
            def __init__(self, thresholds, n_images, max_d, graph=None):
                self.thresholds_host = [float(t) for t in thresholds]
                rec.log.append(["metrics.DeviceCurve", self.thresholds_host, n_images, max_d])

            def reset(self):
                rec.log.append(["curve.reset"])

            def add_raster(self, tp, fp, det_score, nd, ng, gignored):
                rec.log.append(["curve.add_raster"] + [_desc(t) for t in (tp, fp, det_score, nd, ng, gignored)])

            def add_ic15(self, det_match, gt_match, det_score, nd, ng):
                rec.log.append(["curve.add_ic15"] + [_desc(t) for t in (det_match, gt_match, det_score, nd, ng)])

            def finish(self, record):
                rec.log.append(["curve.finish", _desc(record)])

            def value_with(self, acc, extra):
                acc.reads += 1
                T = len(self.thresholds_host)
                rec.log.append(["curve.value_with", 4 + extra.numel() + 4 * T + 2])
                record = tuple(int(v) for v in acc.record.tolist())
                rows = [[record[0], max(record[1] - t, 0), record[2], max(record[3] - t, 0)] for t in range(T)]
                return record, [int(v) for v in extra.reshape(-1).tolist()], rows, 0, 0.625
        return Curve

    @contextlib.contextmanager
    def installed(self):
        from tensorflow_ocr_amd import ops
        from tensorflow_ocr_amd.tool import bboxes, metrics, pixellink_fn, rbox
        stubs = [(ops, "resize_linear_u8", self.resize), (ops, "eval_collect", self.collect),
                 (rbox, "detect_device", self.rbox_detect), (rbox, "detect_multiscale_device", self.rbox_multiscale),
                 (pixellink_fn, "pixel_scores", self.pixel_scores), (pixellink_fn, "link_scores", self.link_scores),
                 (pixellink_fn, "detect_device", self.link_detect), (pixellink_fn, "detect_device_multiscale", self.link_multiscale),
                 (bboxes, "bboxes_matching_batch", self.match_raster), (bboxes, "ic15_matching_batch", self.match_ic15),
                 (metrics, "DeviceTpFp", self.acc_class()), (metrics, "DeviceCurve", self.curve_class())]
        saved = [(mod, name, getattr(mod, name)) for mod, name, _ in stubs]
        for mod, name, stub in stubs:
            setattr(mod, name, stub)
        try:
            yield self
        finally:
            for mod, name, orig in saved:
                setattr(mod, name, orig)


def run_case(d, case, protocol="raster", sweep=None, over=(), over_d=False):
    """one evaluator, built and run once under the recorder -> {'trace', and 'result' or 'raised'}"""
    from tensorflow_ocr_amd import evaluate
    cls, kw = CASES[case]
    rec = Recorder(cls, over, over_d)
    out = {"trace": rec.log}
    with rec.installed():
        try:
            ev = getattr(evaluate, cls)(types.SimpleNamespace(device=torch.device("cpu")), rec.forward, d, batch_size=2,
                                        protocol=protocol, sweep=sweep, **kw)
            out["result"] = ev.run()
        except ValueError as e:
            out["raised"] = str(e)
    return json.loads(json.dumps(out))                      # (tuples become lists, as the golden file holds them)


def pass_name(case, protocol, sweep):
    return "%s %s %s" % (case, protocol, "sweep" if sweep else "plain")


def overflow_name(case, cols, over_d, sweep):
    return "%s over %s%s %s" % (case, ",".join(str(c) for c in cols) or "-", " and max_d" if over_d else "",
                                "sweep" if sweep else "plain")


def record_all(d):
    passes = {pass_name(c, p, s): run_case(d, c, p, s) for c in CASES for p in PROTOCOLS for s in SWEEPS}
    overflow = {overflow_name(c, cols, od, s): run_case(d, c, "raster", s, cols, od)["raised"]
                for c, cols, od in overflow_cases() for s in SWEEPS}
    return {"passes": passes, "overflow": overflow}


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eval_pass"))
    write_dir(d)
    return d


def test_golden_holds_every_case(golden):
    assert len(golden["parent"]) == 40
    assert sorted(golden["passes"]) == sorted(pass_name(c, p, s) for c in CASES for p in PROTOCOLS for s in SWEEPS)
    assert sorted(golden["overflow"]) == sorted(overflow_name(c, cols, od, s) for c, cols, od in overflow_cases() for s in SWEEPS)
    # the cases run: only the two the sizing rule refuses end in an error, and every pass reads the device exactly once
    for name, want in golden["passes"].items():
        assert ("raised" in want) == name.startswith(("rbox_ms_nms ", "rbox_ms_vote ")), name
        if "result" in want:
            reads = [e for e in want["trace"] if e[0] in ("acc.value_with", "curve.value_with")]
            assert len(reads) == 1 and want["trace"][-1] == reads[0] and want["result"]["images"] == 5, name


@pytest.mark.parametrize("sweep", SWEEPS, ids=["plain", "sweep"])
@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_pass_launches_what_the_parent_launched(golden, data, case, protocol, sweep):
    want = golden["passes"][pass_name(case, protocol, sweep)]
    got = run_case(data, case, protocol, sweep)
    for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, (i, a, b)                            # the first call that moved, by name
    assert len(got["trace"]) == len(want["trace"])
    assert got == want                                      # ... and the result dictionary, or the error's text
    if "result" in want:
        assert list(got["result"]) == list(want["result"])  # key order included


def test_the_detector_is_chosen_once_and_a_link_evaluator_holds_no_rbox_option(data):
    from tensorflow_ocr_amd import evaluate
    g = types.SimpleNamespace(device=torch.device("cpu"))
    want = {"rbox": "RboxSingleScale", "rbox_ms_vote_07": "RboxMultiScale", "link": "LinkSingleScale", "link_fused": "LinkFused",
            "link_flip": "LinkFused"}
    for case, name in want.items():
        cls, kw = CASES[case]
        with Recorder(cls).installed():
            ev = getattr(evaluate, cls)(g, None, data, **kw)
        assert type(ev.detector).__name__ == name and issubclass(type(ev), evaluate.Evaluator)
        if cls == "LinkEvaluator":
            rbox = ("score_map_thresh", "nms_thres", "box_thresh", "max_k", "max_side_len", "ms_scales", "fuse", "max_pool")
            assert not [k for k in rbox if hasattr(ev, k)]
            assert (ev.eval_hw, ev.max_comps, ev.max_d, ev.scales(96, 128)) == ((128, 256), 64, 1024, (2.0, 3.0))


@pytest.mark.parametrize("case,cols,over_d", list(overflow_cases()),
                         ids=lambda v: v if isinstance(v, str) else ("d" if v is True else "" if v is False else "c" + "".join(map(str, v))))
def test_overflow_is_reported_in_the_parents_order_and_words(golden, data, case, cols, over_d):
    for sweep in SWEEPS:
        got = run_case(data, case, "raster", sweep, cols, over_d)
        assert got.get("raised") == golden["overflow"][overflow_name(case, cols, over_d, sweep)], (cols, over_d, sweep)
        assert got["trace"][-1][0] in ("acc.value_with", "curve.value_with")      # raised after the one read, not before
