"""CPU: host side of the decode-threshold grid of the link geometry (csrc/decode_grid.hip, include/ocr_decode_grid.h,
pixellink_fn.detect_device_grid, metrics.DeviceGrid, evaluate.LinkEvaluator's grid / grid_chunk).  The build wiring and the
kernel inventory of tests/test_gpu_link_cc_grid.py, the copy of decode.hip's direction table, the refusals decided before
anything is launched, grid validation, row order, the tie rule, format_grid, the flags of both scripts, and one grid pass on
the recorder of tests/test_eval_pass_host.py: what it launches per chunk, and that grid=None launches what it launched."""
import ast
import ctypes
import importlib
import os
import re
import sys
import types

import pytest
import torch

import mapfuse_ref as R
import test_eval_pass_host as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ocr_link_cc_grid", "ocr_link_cc_grid_workspace", "ocr_component_scores_grid",
               "ocr_component_scores_grid_workspace")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ build wiring
def test_header_is_included_declares_the_entries_and_the_makefile_knows_it():
    hip = _read("include", "ocr_hip.h")
    assert re.search(r'^#include "ocr_decode_grid\.h"$', hip, flags=re.M)
    txt = _read("include", "ocr_decode_grid.h")
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert declared == set(NEW_SYMBOLS)
    for word in ("b = g * n + i", "never replicated", "bit for bit", "HOST MEMORY", "G > 65", "Nothing is written on error"):
        assert word in txt, word
    mk = _read("tensorflow_ocr_amd", "csrc", "Makefile")
    hdrs = re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1)
    assert "ocr_decode_grid.h" in hdrs and "cc_union.h" in hdrs.split()
    from tensorflow_ocr_amd import _lib
    assert "ocr_decode_grid.h" in _read("tensorflow_ocr_amd", "_lib.py") and _lib.ABI_VERSION == 7


def test_every_kernel_and_entry_of_decode_grid_hip_is_named_in_the_gpu_test():
    src = _read("tensorflow_ocr_amd", "csrc", "decode_grid.hip")
    test = _read("tests", "test_gpu_link_cc_grid.py")
    doc = ast.get_docstring(ast.parse(test))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(", src))
    entries = set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', src))
    assert len(kernels) == 8 and entries == set(NEW_SYMBOLS), (sorted(kernels), sorted(entries))
    assert not [k for k in kernels | entries if not re.search(r"\b%s\b" % k, doc)]
    assert not [e for e in entries if '"%s"' % e not in test]
    # the helpers are shared, not copied: both files include cc_union.h and neither defines what it holds
    shared = _read("tensorflow_ocr_amd", "csrc", "cc_union.h")
    decode = _read("tensorflow_ocr_amd", "csrc", "decode.hip")
    for name in ("uf_find", "uf_unite", "lds_find", "lds_unite"):
        assert re.search(r"__device__ __forceinline__ \w+ %s\(" % name, shared)
        assert not re.search(r"__device__ __forceinline__ \w+ %s\(" % name, decode + src)
    assert "struct CcP" in shared and "struct CcP" not in decode + src and "__global__" not in shared
    assert '#include "cc_union.h"' in decode and '#include "cc_union.h"' in src


def test_direction_table_is_decode_hips():
    assert R.parse_tables("decode_grid.hip") == R.parse_tables("decode.hip")


def test_both_product_libraries_export_the_entries_and_check_their_arguments():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.c_void_p(ctypes.addressof(buf))
    tab = (ctypes.c_float * 66)()
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        size = lib.ocr_link_cc_grid_workspace
        size.restype = ctypes.c_size_t
        lib.ocr_link_cc_workspace.restype = ctypes.c_size_t
        assert size(5, 3, 33, 65) == 5 * lib.ocr_link_cc_workspace(3, 33, 65) and size(0, 3, 33, 65) == 0
        # refusals are decided before anything is launched: host memory stands in for the device pointers
        call = lambda ps=base, n=2, h=8, w=8, G=3, tp=tab, mc=4, ws=ctypes.c_size_t(1 << 30), stride=1, off=0: lib.ocr_link_cc_grid(
            ps, base, stride, off, n, h, w, G, tp, tab, 0, base, base, base, mc, base, ws, None)
        assert call(ps=None) == -1 and call(tp=None) == -1 and call(G=0) == -1 and call(n=0) == -1 and call(mc=0) == -1
        assert call(stride=0) == -1 and call(off=1) == -1
        assert call(G=66) == -2 and call(G=64, n=1024) == -2 and call(h=2) == -2 and call(w=2) == -2
        assert call(G=64, n=1023, h=200, w=200) == -2                          # G * n * h * w > INT32_MAX
        assert call(ws=ctypes.c_size_t(size(3, 2, 8, 8) - 1)) == -4
        cs = lib.ocr_component_scores_grid
        csize = lib.ocr_component_scores_grid_workspace
        csize.restype = ctypes.c_size_t
        assert csize(3, 2, 16) == 3 * 2 * 16 * 16 and csize(3, 0, 16) == 0
        ccall = lambda lab=base, G=3, n=2, h=8, w=8, mc=16, ws=ctypes.c_size_t(1 << 30): cs(lab, base, base, G, n, h, w, mc, base,
                                                                                           base, ws, None)
        assert ccall(lab=None) == -1 and ccall(G=0) == -1 and ccall(h=0) == -1
        assert ccall(G=66) == -2 and ccall(n=65536) == -2 and ccall(mc=65536) == -2 and ccall(h=32769) == -2
        assert ccall(ws=ctypes.c_size_t(csize(3, 2, 16) - 1)) == -4


def test_ops_bindings_check_shapes_before_the_library_is_reached():
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    assert callable(P.detect_device_grid) and callable(P.link_cc_decode_grid) and ops.GRID_MAX_POINTS == 65
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    i32 = torch.int32
    ok = dict(pixel_score=z(2, 4, 6), link_score=z(8, 2, 4, 6), stride=1, offset=0, pixel_thresholds=[0.5, 0.6, 0.7],
              link_thresholds=[0.5, 0.6, 0.7], min_size=0, labels=z(6, 4, 6, dt=i32), ncomp=z(6, dt=i32), comps=z(6, 5, 2, dt=i32),
              ws=None)
    for kw in (dict(link_thresholds=[0.5]), dict(pixel_thresholds=[], link_thresholds=[]), dict(pixel_thresholds=[0.5] * 66),
               dict(labels=z(4, 4, 6, dt=i32)), dict(ncomp=z(5, dt=i32)), dict(comps=z(6, 5, 3, dt=i32)), dict(labels=z(6, 4, 6)),
               dict(link_score=z(8, 2, 4, 6, 2)), dict(pixel_score=z(2, 4, 6, dt=torch.float64)),
               dict(labels=z(6, 6, 4, dt=i32).transpose(1, 2))):
        with pytest.raises(ValueError, match="link_cc_grid"):
            ops.link_cc_grid(**dict(ok, **kw))
    ok = dict(labels=z(6, 4, 6, dt=i32), pixel_score=z(2, 4, 6), ncomp=z(6, dt=i32), comp_score=z(6, 5), ws=None)
    for kw in (dict(labels=z(5, 4, 6, dt=i32), ncomp=z(5, dt=i32), comp_score=z(5, 5)), dict(pixel_score=z(2, 4, 5)),
               dict(ncomp=z(4, dt=i32)), dict(comp_score=z(6, 5, dt=torch.float64)), dict(labels=z(6, 4, 6))):
        with pytest.raises(ValueError, match="component_scores_grid"):
            ops.component_scores_grid(**dict(ok, **kw))


# ------------------------------------------------------------------------------------------------ validation
def test_check_grid_orders_pixel_major_and_refuses_what_the_issue_lists(tmp_path):
    from tensorflow_ocr_amd import evaluate
    assert evaluate.check_grid(([0.5, 0.7], [0.6, 0.8, 0.9])) == [(0.5, 0.6), (0.5, 0.8), (0.5, 0.9), (0.7, 0.6), (0.7, 0.8), (0.7, 0.9)]
    assert len(evaluate.check_grid(([0.1] * 8, [0.2] * 8))) == 64 and evaluate.check_grid(((0.5,), (1,))) == [(0.5, 1.0)]
    for bad in (([], [0.5]), ([0.5], []), ([float("nan")], [0.5]), ([0.5], [float("inf")]), ([0.1] * 13, [0.2] * 5),
                ([0.1] * 65, [0.2]), 0.5, ([0.5],), ("a", [0.5]), ([0.5], 3)):
        with pytest.raises(ValueError):
            evaluate.check_grid(bad)
    d = str(tmp_path)
    with pytest.raises(ValueError, match="link geometry"):
        evaluate.Evaluator(None, None, d, grid=([0.5], [0.5]))
    with pytest.raises(ValueError, match="grid and sweep"):
        evaluate.LinkEvaluator(None, None, d, grid=([0.5], [0.5]), sweep=[0.5])
    for kw in (dict(grid=([], [0.5])), dict(grid=([float("nan")], [0.5])), dict(grid=([0.1] * 13, [0.2] * 5)),
               dict(grid_chunk=4), dict(grid=([0.5], [0.5]), grid_chunk=0)):
        with pytest.raises(ValueError):
            evaluate.LinkEvaluator(None, None, d, **kw)
    for kw in (dict(grid=([0.5, 0.6], [0.7])), dict(grid=([0.1] * 8, [0.2] * 8), grid_chunk=3, flip=True, protocol="icdar15")):
        with pytest.raises(FileNotFoundError):                                  # good options get as far as the empty directory
            evaluate.LinkEvaluator(None, None, d, **kw)


def _record(tp, fp, num_gt=10):
    return (num_gt, tp, fp, tp + fp)


def test_rows_best_and_the_tie_rule_on_hand_made_records():
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.tool import metrics
    points = [(0.8, 0.9), (0.5, 0.5), (0.5, 0.7), (0.6, 0.5), (0.6, 0.7)]
    records = [_record(4, 4), _record(6, 2), _record(2, 0), _record(6, 2), _record(0, 0)]
    rows = evaluate.grid_rows(points, records, [0, 0, 0, 0, 0])
    assert [(r["pixel_conf_threshold"], r["link_conf_threshold"]) for r in rows] == points
    assert sorted(rows[0]) == sorted(["pixel_conf_threshold", "link_conf_threshold", "precision", "recall", "hmean", "tp", "fp",
                                      "num_det", "num_gt"])
    for row, (num_gt, tp, fp, n_det) in zip(rows, records):
        p, r = metrics.precision_recall(num_gt, tp, fp)
        assert (row["precision"], row["recall"], row["tp"], row["fp"], row["num_det"], row["num_gt"]) == (p, r, tp, fp, n_det, num_gt)
        assert row["hmean"] == (metrics.fmean(p, r) if p + r > 0 else 0.0)
    assert rows[1]["hmean"] == rows[3]["hmean"] > rows[0]["hmean"] and rows[4]["hmean"] == 0.0
    assert evaluate.grid_best(rows) is rows[1]                                  # the tie goes to the lowest index
    assert evaluate.grid_best(rows[:1]) is rows[0]
    # a row that overflowed reports it, holds no metric and cannot be the best
    rows = evaluate.grid_rows(points, records, [0, 7, 0, 0, 0])
    assert rows[1]["overflow"] == 7 and rows[1]["hmean"] is None and rows[1]["tp"] is None and rows[1]["num_gt"] is None
    assert "overflow" not in rows[0] and evaluate.grid_best(rows) is rows[3]


def test_format_grid_prints_one_line_per_row_and_marks_the_best():
    from tensorflow_ocr_amd import evaluate
    points = [(0.8, 0.9), (0.5, 0.5), (0.5, 0.7)]
    rows = evaluate.grid_rows(points, [_record(4, 4), _record(6, 2), _record(6, 2)], [0, 0, 3])
    result = {"grid": rows, "grid_best": evaluate.grid_best(rows)}
    lines = evaluate.format_grid(result).splitlines()
    assert len(lines) == 4
    assert lines[0].startswith("  pixel > 0.8") and "link > 0.9" in lines[0] and not lines[0].endswith("*")
    assert lines[1].endswith(" *") and "precision 0.7500 recall 0.6000" in lines[1] and "(tp 6 fp 2 det 8)" in lines[1]
    assert "overflow: 3" in lines[2] and "precision" not in lines[2]
    assert lines[3] == "  best hmean %.4f at pixel > 0.5, link > 0.5" % rows[1]["hmean"]
    line = evaluate.format_line(dict(rows[0], num_gt=10))                       # format_line is what it was
    assert line == "precision 0.5000 recall 0.4000 hmean 0.4444 (gt 10 det 8)"


# ------------------------------------------------------------------------------------------------ flags
def test_scripts_take_the_grid_flags(capsys):
    sys.path.insert(0, ROOT)
    ev = importlib.import_module("eval_pixellink_fast")
    from tensorflow_ocr_amd import cli
    F = ev.parse([])
    # without the flags the namespace is what it always was (tests/test_cli_host.py holds it to the recorded one)
    assert not hasattr(F, "eval_grid_pixel") and not hasattr(F, "eval_grid_link") and cli.grid_option(F) is None
    F = ev.parse(["--eval_grid_pixel", "0.5:0.9:5", "--eval_grid_link", "0.6,0.8"])
    grid = cli.grid_option(F)
    assert grid[0] == pytest.approx([0.5, 0.6, 0.7, 0.8, 0.9], abs=1e-12) and grid[1] == [0.6, 0.8]
    assert grid == (F.eval_grid_pixel, F.eval_grid_link)
    for argv in (["--eval_grid_pixel", "0.5"], ["--eval_grid_link", "0.5,0.6"], ["--eval_grid_pixel", "x", "--eval_grid_link", "0.5"],
                 ["--eval_grid_pixel", "0:1:13", "--eval_grid_link", "0:1:5"], ["--eval_grid_pixel", "", "--eval_grid_link", "0.5"],
                 ["--eval_grid_pixel", "0.5", "--eval_grid_link", "0.5", "--eval_sweep", "0.5"]):
        with pytest.raises(SystemExit):
            ev.parse(argv)
    tr = importlib.import_module("train_pixellink")
    assert cli.grid_option(tr.parse([])) is None
    on = ["--eval_data_path", "/x", "--eval_steps", "10", "--using_moving_average"]
    F = tr.parse(on + ["--eval_grid_pixel", "0.5,0.7", "--eval_grid_link", "0.9:0.9:1"])
    assert cli.grid_option(F) == ([0.5, 0.7], [0.9])
    for argv in (on + ["--eval_grid_pixel", "0.5"], on + ["--eval_grid_link", "0.5"],
                 ["--eval_grid_pixel", "0.5", "--eval_grid_link", "0.5"],          # no evaluation to put it in
                 on + ["--eval_grid_pixel", "0.5", "--eval_grid_link", "0.5", "--eval_sweep", "0.5,0.6"]):
        with pytest.raises(SystemExit):
            tr.parse(argv)
    capsys.readouterr()
    src = _read("test_pixellink_fast.py")                                       # the reference's script has no such flag
    assert "grid" not in src


def test_train_eval_passes_the_grid_on_and_writes_the_three_scalars():
    import inspect
    from tensorflow_ocr_amd import evaluate
    seen = {}

    class Probe:
        def __init__(self, graph, forward, data, **kw):
            seen.update(kw)
    te = evaluate.TrainEval(None, None, None, "/x", 5, evaluator=Probe, grid=([0.5], [0.6, 0.7]), grid_chunk=2)
    assert seen["grid"] == ([0.5], [0.6, 0.7]) and seen["grid_chunk"] == 2
    params = inspect.signature(evaluate.LinkEvaluator.__init__).parameters
    assert [params[k].default for k in ("grid", "grid_chunk")] == [None, None]
    rows = evaluate.grid_rows([(0.8, 0.9), (0.5, 0.6)], [_record(4, 4), _record(6, 2)], [0, 0])
    te.last = dict(rows[0], grid=rows, grid_best=rows[1])
    scalars, steps = {}, []
    writer = types.SimpleNamespace(add_scalar=lambda k, v: scalars.__setitem__(k, v), flush_step=steps.append)
    te.write(writer, 40)
    assert scalars == {"eval/precision": 0.5, "eval/recall": 0.4, "eval/hmean": rows[0]["hmean"],
                       "eval/grid_best_hmean": rows[1]["hmean"], "eval/grid_best_pixel_threshold": 0.5,
                       "eval/grid_best_link_threshold": 0.6} and steps == [40]


# ------------------------------------------------------------------------------------------------ one grid pass, recorded
class GridRecorder(T.Recorder):
    """the recorder of test_eval_pass_host.py plus the grid's entries: detect_device_grid (its thresholds by value;
    `over`: point -> by how much image 0 of every chain exceeds max_comps at it), fuse_score_maps and DeviceGrid"""

    def __init__(self, over=None):
        super().__init__("LinkEvaluator")
        self.over_at = over or {}

    def link_detect_grid(self, pixel_score, link_score, pixel_thresholds, link_thresholds, min_size=10, scale_x=4.0, scale_y=4.0,
                         max_comps=4096, min_side=0.0, min_area=0.0, graph=None):
        self.log.append(["pixellink_fn.detect_device_grid", T._desc(pixel_score), T._desc(link_score), list(pixel_thresholds),
                         list(link_thresholds), min_size, scale_x, scale_y, max_comps])
        n, G = pixel_score.shape[0], len(pixel_thresholds)
        merged, keep, n_keep, passed, total = self._five(G * n, max_comps, True)
        for k, point in enumerate(zip(pixel_thresholds, link_thresholds)):
            if point in self.over_at:
                total[k * n] = max_comps + self.over_at[point]
        return merged, keep, n_keep, passed, total

    def fuse(self, passes, weights, out_hw, graph=None):
        n = 0
        for pixel_cls, link_cls, flip in passes:
            self.log.append(["pass", T._desc(pixel_cls), bool(flip)])
            n = pixel_cls.shape[0]
        self.log.append(["pixellink_fn.fuse_score_maps", [float(w) for w in weights], list(out_hw)])
        acc = torch.zeros((9, n) + tuple(out_hw))
        return acc[0], acc[1:]

    def grid_class(rec):
        class Grid:
            def __init__(self, points, graph=None):
                self.records, self.reads = torch.zeros((points, 4), dtype=torch.int64), 0
                self.record = self.records[0]
                rec.log.append(["metrics.DeviceGrid", points])

            def reset(self):
                rec.log.append(["grid.reset"])
                self.records.zero_()

            def value_with(self, extra):
                self.reads += 1
                rec.log.append(["grid.value_with", self.records.numel() + extra.numel()])
                return [tuple(r) for r in self.records.tolist()], [int(v) for v in extra.reshape(-1).tolist()]
        return Grid

    def installed(self):
        import contextlib
        from tensorflow_ocr_amd.tool import metrics, pixellink_fn

        @contextlib.contextmanager
        def both():
            saved = (getattr(pixellink_fn, "detect_device_grid"), pixellink_fn.fuse_score_maps, metrics.DeviceGrid)
            with T.Recorder.installed(self):
                pixellink_fn.detect_device_grid, pixellink_fn.fuse_score_maps = self.link_detect_grid, self.fuse
                metrics.DeviceGrid = self.grid_class()
                try:
                    yield self
                finally:
                    pixellink_fn.detect_device_grid, pixellink_fn.fuse_score_maps, metrics.DeviceGrid = saved
        return both()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("grid_pass"))
    T.write_dir(d)
    return d


def _run(d, rec, **kw):
    from tensorflow_ocr_amd import evaluate
    with rec.installed():
        ev = evaluate.LinkEvaluator(types.SimpleNamespace(device=torch.device("cpu")), rec.forward, d, batch_size=2,
                                    **dict(T.LINK, **kw))
        return ev, ev.run()


GRID = ([0.5, 0.7], [0.6, 0.9])
POINTS = [(0.8, 0.9), (0.5, 0.6), (0.5, 0.9), (0.7, 0.6), (0.7, 0.9)]


@pytest.mark.parametrize("protocol", T.PROTOCOLS)
def test_a_grid_pass_forwards_once_decodes_per_chunk_and_matches_per_point(data, protocol):
    rec = GridRecorder()
    ev, res = _run(data, rec, grid=GRID, protocol=protocol)
    names = [e[0] for e in rec.log]
    chains = names.count("forward")
    assert chains == 3                                                          # 5 images of two shapes, batches of 2
    assert names.count("pixellink_fn.detect_device_grid") == chains == names.count("ops.eval_collect")
    matcher = "bboxes.bboxes_matching_batch" if protocol == "raster" else "bboxes.ic15_matching_batch"
    assert names.count(matcher) == 5 * chains and "pixellink_fn.detect_device" not in names
    assert names[0] == "metrics.DeviceGrid" and "metrics.DeviceTpFp" not in names
    assert names[-1] == "grid.value_with" and names.count("grid.value_with") == 1 and ev.acc.reads == 1
    assert rec.log[-1][1] == 5 * 4 + 5 * 2                                      # one copy: five records, five pairs of maxima
    for e in rec.log:
        if e[0] == "pixellink_fn.detect_device_grid":
            assert list(zip(e[3], e[4])) == POINTS and e[1][0][0] in (1, 2)     # the maps of the batch, not G copies
        if e[0] == "ops.eval_collect":
            assert e[1][0][0] in (5, 10)                                        # points x images
        if e[0] == matcher:
            assert e[1][0][0] in (1, 2)                                         # ... and each point's own slices
    assert [(r["pixel_conf_threshold"], r["link_conf_threshold"]) for r in res["grid"]] == POINTS
    top = {k: res["grid"][0][k] for k in ("precision", "recall", "hmean", "tp", "fp", "num_det", "num_gt")}
    assert {k: res[k] for k in top} == top and res["images"] == 5
    assert res["grid_best"] is res["grid"][0]                                   # every stub record is the same: the tie rule
    # the plain run of the same pair gives the same top-level fields, key for key
    plain = T.run_case(data, "link", protocol)["result"]
    assert {k: res[k] for k in plain} == plain and list(res)[:len(plain)] == list(plain)


def test_the_result_does_not_depend_on_grid_chunk_and_the_chunks_are_what_was_asked(data):
    results = []
    for chunk, per_chain in ((None, 1), (1, 5), (2, 3), (5, 1)):
        rec = GridRecorder()
        _, res = _run(data, rec, grid=GRID, grid_chunk=chunk)
        results.append(res)
        calls = [e for e in rec.log if e[0] == "pixellink_fn.detect_device_grid"]
        assert len(calls) == 3 * per_chain and max(len(e[3]) for e in calls) == (chunk or 5)
        assert [p for e in calls[:per_chain] for p in zip(e[3], e[4])] == POINTS
        assert [e[0] for e in rec.log].count("forward") == 3
    assert all(r == results[0] for r in results)
    from tensorflow_ocr_amd import evaluate
    assert evaluate.GRID_MAX_SLICES == 512


def test_overflow_is_per_point(data):
    rec = GridRecorder(over={(0.5, 0.9): 7})
    _, res = _run(data, rec, grid=GRID)
    rows = res["grid"]
    assert rows[2]["overflow"] == 7 and rows[2]["hmean"] is None and [("overflow" in r) for r in rows] == [False, False, True, False, False]
    clean = _run(data, GridRecorder(), grid=GRID)[1]
    assert [r for k, r in enumerate(rows) if k != 2] == [r for k, r in enumerate(clean["grid"]) if k != 2]
    assert res["grid_best"] is rows[0] and "overflow" not in res
    # the same point as the base pair raises what the plain pass raises
    rec = GridRecorder(over={(0.5, 0.9): 7})
    with pytest.raises(ValueError, match="an image holds 7 components more than max_comps = 64"):
        _run(data, rec, grid=GRID, pixel_conf_threshold=0.5, link_conf_threshold=0.9)
    assert rec.log[-1][0] == "grid.value_with"                                  # raised after the one read, not before


def test_the_grid_runs_behind_fused_maps(data):
    rec = GridRecorder()
    _, res = _run(data, rec, grid=GRID, flip=True)
    names = [e[0] for e in rec.log]
    assert names.count("forward") == 6 and names.count("pixellink_fn.fuse_score_maps") == 3
    assert names.count("pixellink_fn.detect_device_grid") == 3 and "pixellink_fn.detect_device_multiscale" not in names
    assert len(res["grid"]) == 5


def test_without_a_grid_the_pass_is_the_recorded_one(data):
    """(tests/test_eval_pass_host.py holds every case to the golden trace; this is its link case through this file's recorder,
    whose extra stubs must stay unused)"""
    import json
    with open(T.GOLDEN) as f:
        want = json.load(f)["passes"][T.pass_name("link_flip", "raster", None)]
    rec = GridRecorder()
    _, res = _run(data, rec, flip=True)
    assert json.loads(json.dumps(rec.log)) == want["trace"] and json.loads(json.dumps(res)) == want["result"]
