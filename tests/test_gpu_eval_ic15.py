"""GPU: ocr_eval_ic15_match_batch (csrc/eval_ic15.hip, tool/bboxes.ic15_matching_batch, evaluate.py protocol='icdar15')
against the exact reference tests/ic15_ref.py.  Matches and the record are integers and must be equal; the exported
intersection areas must lie within 2^-40 (area_d + area_g) of the exact ones (about 10^3 x the deviation a float64
restatement of the clipper showed; the room is for another valid operation order).  tests/test_ic15_host.py checks on the
CPU that every decision of every fixture is further than 1e-6 from the thresholds, or an exact lattice tie.
Shapes n = 3, max_d = 16, max_g = 8; one case with max_d = 96 for the 64-wide scan."""
import ctypes
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import eval_support as E
import ic15_ref as R
from eval_support import EVAL

pytestmark = pytest.mark.gpu
MAX_D, MAX_G, N = R.MAX_D, R.MAX_G, R.N
SENT = -77
FIXTURES = {name: images for name, (images, _) in R.directed_cases().items()}
FIXTURES.update({"jittered_%d" % s: R.jittered_cases(s) for s in R.JITTER_SEEDS})
TOL = Fr(1, 2 ** 40)


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


@pytest.fixture(scope="module")
def rbox_eval_dir(graph, tmp_path_factory):
    return E.rbox_eval_dir(graph, str(tmp_path_factory.mktemp("eval")))


@pytest.fixture(scope="module")
def link_eval_dir(device, graph, tmp_path_factory):
    return E.link_eval_dir(str(tmp_path_factory.mktemp("link_eval")), E.host_best_box(graph, device))


@pytest.fixture(scope="module")
def expected():
    """the exact reference, computed once"""
    return {name: [R.match_image(*im) for im in images] for name, images in FIXTURES.items()}


def _pack(images, device, max_d=MAX_D, max_g=MAX_G):
    """images -> device tensors; rows beyond a count hold a quad that would match everything there"""
    n = len(images)
    dets = np.zeros((n, max_d, 4, 2), np.int32)
    gts = np.zeros((n, max_g, 4, 2), np.int32)
    nd, ng = np.zeros(n, np.int32), np.zeros(n, np.int32)
    dc = np.zeros((n, max_g), np.uint8)
    for i, (d, g, c) in enumerate(images):
        fill = d[0] if len(d) else g[0] if len(g) else np.asarray(R.A)
        dets[i], gts[i] = fill, fill
        dets[i, :len(d)], gts[i, :len(g)], dc[i, :len(g)] = d, g, c
        nd[i], ng[i] = len(d), len(g)
    up = lambda a: torch.from_numpy(a).to(device)
    return up(dets), up(nd), up(gts), up(ng), up(dc)


def _want(refs, max_d=MAX_D, max_g=MAX_G):
    dm, gm = np.full((len(refs), max_d), -1, np.int32), np.full((len(refs), max_g), -1, np.int32)
    rec = np.zeros(4, np.int64)
    for i, r in enumerate(refs):
        dm[i, :len(r["det_match"])], gm[i, :len(r["gt_match"])] = r["det_match"], r["gt_match"]
        rec += r["record"]
    return dm, gm, rec


def _run_abi(device, packed, max_d=MAX_D, max_g=MAX_G, export=True):
    """through ops (the C ABI): sentinel-filled outputs with a tail behind them"""
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.graph import Graph
    n = packed[0].shape[0]
    dm = torch.full((n * max_d + 32,), SENT, dtype=torch.int32, device=device)
    gm = torch.full((n * max_g + 32,), SENT, dtype=torch.int32, device=device)
    inter = torch.full((n, max_g, max_d), float(SENT), dtype=torch.float64, device=device) if export else None
    rec = torch.full((6,), -99, dtype=torch.int64, device=device)
    ops.eval_record_init(rec[:4])
    ops.eval_ic15_match_batch(*packed, 0.5, 0.5, dm[:n * max_d].view(n, max_d), gm[:n * max_g].view(n, max_g), rec[:4],
                              Graph(device).workspace(), inter=inter)
    torch.cuda.synchronize()
    assert (dm[n * max_d:] == SENT).all() and (gm[n * max_g:] == SENT).all() and rec[4:].tolist() == [-99, -99]
    return (dm[:n * max_d].view(n, max_d).cpu().numpy(), gm[:n * max_g].view(n, max_g).cpu().numpy(), rec[:4].cpu().numpy(),
            None if inter is None else inter.cpu().numpy())


def _check_inter(inter, refs, tag):
    worst = Fr(0)
    for i, r in enumerate(refs):
        n_g, k = len(r["gt_match"]), len(r["det_match"])
        for g in range(n_g):
            for d in range(k):
                err, room = abs(Fr(float(inter[i, g, d])) - r["inter"][g][d]), TOL * (r["area_d"][d] + r["area_g"][g])
                if room > 0:
                    worst = max(worst, err / room)
                assert err <= room, (tag, i, g, d, float(err), float(room))
        assert (inter[i, n_g:] == SENT).all() and (inter[i, :, k:] == SENT).all()          # dead pairs are not written
    print("ic15 %s: worst |inter - exact| / (2^-40 (area_d + area_g)) = %.3g" % (tag, float(worst)))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_match_batch_equals_the_exact_reference(device, graph, expected, name):
    from tensorflow_ocr_amd.tool import bboxes
    refs = expected[name]
    wdm, wgm, wrec = _want(refs)
    packed = _pack(FIXTURES[name], device)
    dm, gm, rec, inter = _run_abi(device, packed)
    print("ic15 %s: record %s, reference %s" % (name, rec.tolist(), wrec.tolist()))
    assert np.array_equal(dm, wdm) and np.array_equal(gm, wgm) and rec.tolist() == wrec.tolist()
    _check_inter(inter, refs, name)
    # the tool wrapper: device tensors, a record of its own, bool flags
    tdm, tgm, trec = bboxes.ic15_matching_batch(*packed[:4], packed[4].bool(), graph=graph)
    assert tdm.is_cuda and tdm.dtype == torch.int32 and trec.dtype == torch.int64
    assert np.array_equal(tdm.cpu().numpy(), wdm) and np.array_equal(tgm.cpu().numpy(), wgm) and trec.tolist() == wrec.tolist()
    # the containment ties are decided as the exact rule decides them (pinned by hand in test_ic15_host)
    if name == "half_iou_is_no_match":
        assert dm[0, 0] == -1 and gm[0, 0] == -1 and dm[1, 0] == 0 and inter[0, 0, 0] == 100.0
    if name == "dontcare_half_precision":
        assert dm[0, 0] == -1 and dm[1, 0] == -2 and inter[0, 0, 0] == 100.0 and inter[1, 0, 0] == 110.0


def test_the_64_wide_scan_takes_the_first_free_detection(device, graph):
    """one image, max_d = 96, nd = 70, ng = 8: the only free detection that matches gt 0 sits at index 65, in the second
    64-block; index 3 overlaps gt 0 above the threshold too (480 / 800) but is a don't-care detection: the don't-care gt 1,
    the top 8 rows of gt 0, holds 320 / 480 of it and only 280 / 760 of detection 65; index 64 overlaps gt 0 by 1/8; the
    last gt is matched too; the rows beyond nd / ng hold quads that would match and must never be read."""
    g0, top, g7 = R.rect(10, 10, 50, 30), R.rect(10, 10, 50, 18), R.rect(200, 200, 240, 230)
    far = [R.rect(300 + 12 * k, 0, 310 + 12 * k, 8) for k in range(70)]
    dets = list(far)
    dets[3], dets[65], dets[64], dets[69] = R.rect(10, 10, 50, 22), R.rect(10, 11, 50, 30), R.rect(10, 20, 20, 30), g7
    gts = [g0, top] + [R.rect(0, 100 + 12 * k, 30, 110 + 12 * k) for k in range(5)] + [g7]
    image = R._image(dets, gts, [0, 1, 0, 0, 0, 0, 0, 0])
    ref = R.match_image(*image)
    assert ref["det_match"][3] == -2 and ref["det_match"][65] == 0 and ref["det_match"][69] == 7 and ref["det_match"][64] == -1
    assert ref["gt_match"] == [65, -2, -1, -1, -1, -1, -1, 69]
    assert ref["iou"][0][3] == Fr(3, 5) and ref["prec"][1][3] == Fr(2, 3) and ref["prec"][1][65] == Fr(7, 19)
    assert ref["iou"][0][64] == Fr(1, 8)
    wdm, wgm, wrec = _want([ref], 96, MAX_G)
    packed = _pack([image], device, 96, MAX_G)
    dm, gm, rec, inter = _run_abi(device, packed, 96, MAX_G)
    assert np.array_equal(dm, wdm) and np.array_equal(gm, wgm) and rec.tolist() == wrec.tolist()
    _check_inter(inter, [ref], "scan")
    # ng below max_g: the rows beyond it hold a copy of detection 0 and stay -1
    few = R._image(dets, gts[:3], [0, 1, 0])
    ref3 = R.match_image(*few)
    dm3, gm3, rec3, _ = _run_abi(device, _pack([few], device, 96, MAX_G), 96, MAX_G, export=False)
    w3 = _want([ref3], 96, MAX_G)
    assert np.array_equal(dm3, w3[0]) and np.array_equal(gm3, w3[1]) and rec3.tolist() == w3[2].tolist()
    assert gm3[0, 3:].tolist() == [-1] * 5 and (dm3[0, 70:] == -1).all()


def test_record_accumulates_and_runs_are_bit_identical(device, graph, expected):
    from tensorflow_ocr_amd.tool import bboxes, metrics
    acc = metrics.DeviceTpFp(graph)
    total = np.zeros(4, np.int64)
    for name in ("jittered_1", "chevron"):
        bboxes.ic15_matching_batch(*_pack(FIXTURES[name], device), record=acc.record, graph=graph)
        total += _want(expected[name])[2]
    assert acc.reads == 0 and acc.value() == tuple(int(v) for v in total) and acc.reads == 1
    p, r = metrics.precision_recall(*acc.value()[:3])
    assert p == total[1] / (total[1] + total[2]) and r == total[1] / total[0]
    acc.reset()                                                             # ocr_eval_record_init zeroes it
    assert acc.value() == (0, 0, 0, 0)
    packed = _pack(FIXTURES["jittered_2"], device)
    a, b = _run_abi(device, packed), _run_abi(device, packed)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()                                   # every output, the areas included, bit for bit


def test_every_status_code_leaves_the_outputs_alone(device, expected):
    from tensorflow_ocr_amd import _lib as L
    dets, nd, gts, ng, dc = _pack(FIXTURES["jittered_1"], device)
    nbytes = L.call_size("ocr_eval_ic15_workspace", ctypes.c_int(N), ctypes.c_int(MAX_D), ctypes.c_int(MAX_G))
    dm = torch.full((N, MAX_D), SENT, dtype=torch.int32, device=device)
    gm = torch.full((N, MAX_G), SENT, dtype=torch.int32, device=device)
    inter = torch.full((N, MAX_G, MAX_D), float(SENT), dtype=torch.float64, device=device)
    rec = torch.full((4,), -99, dtype=torch.int64, device=device)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=device)
    fn = L._fn("ocr_eval_ic15_match_batch", ctypes.c_int)
    D, SZ, p = ctypes.c_double, ctypes.c_size_t, L.ptr

    def call(dets=dets, nd=nd, gts=gts, ng=ng, dc=dc, n=N, d=MAX_D, g=MAX_G, dm=dm, gm=gm, inter=inter, rec=rec, ws=ws, wsb=nbytes):
        return fn(p(dets), p(nd), p(gts), p(ng), p(dc), n, d, g, D(0.5), D(0.5), p(dm), p(gm), p(inter), p(rec), p(ws), SZ(wsb),
                  L.stream_ptr())
    for kw in (dict(dets=None), dict(nd=None), dict(gts=None), dict(ng=None), dict(dc=None), dict(dm=None), dict(gm=None),
               dict(rec=None), dict(ws=None), dict(n=0), dict(d=0), dict(g=-1)):
        assert call(**kw) == -1, kw
    for kw in (dict(d=1025), dict(g=255), dict(n=65536)):
        assert call(**kw) == -2, kw
    assert call(wsb=nbytes - 1) == -4 and call(wsb=0) == -4
    torch.cuda.synchronize()
    assert (dm == SENT).all() and (gm == SENT).all() and (inter == SENT).all() and (ws == 0xA5).all() and rec.tolist() == [-99] * 4
    assert call(inter=None) == 0                                            # the export is optional; the same arguments run
    torch.cuda.synchronize()
    wdm, wgm, wrec = _want(expected["jittered_1"])
    assert np.array_equal(dm.cpu().numpy(), wdm) and np.array_equal(gm.cpu().numpy(), wgm) and (inter == SENT).all()
    assert rec.tolist() == (np.array([-99] * 4) + wrec).tolist()            # added to, not overwritten


# ------------------------------------------------------------------------------------------------ the chain
def _chain_case(ev, calls, monkeypatch):
    """one icdar15 pass with every chain's `last` kept (device tensors, no read) -> (result, reads, reference record)"""
    chains = E.keep_lasts(ev)
    reads = E.spy_reads(monkeypatch, calls)
    res = ev.run()
    monkeypatch.undo()
    want = np.zeros(4, np.int64)
    for last in chains:
        host = {k: last[k].cpu().numpy() for k in ("dets", "nd", "gts", "ng", "gdontcare", "det_match", "gt_match")}
        for i in range(len(host["nd"])):
            k, n_g = int(host["nd"][i]), int(host["ng"][i])
            r = R.match_image(host["dets"][i, :k], host["gts"][i, :n_g], host["gdontcare"][i, :n_g].astype(bool))
            assert host["det_match"][i, :k].tolist() == r["det_match"] and host["gt_match"][i, :n_g].tolist() == r["gt_match"]
            want += r["record"]
    return res, reads, want


def _check_chain(evaluate, res, reads, want, n_chains):
    from tensorflow_ocr_amd.tool import metrics
    print("icdar15 chain: %s, reference record %s" % (evaluate.format_line(res), want.tolist()))
    assert reads == [("cpu", n_chains)], reads                              # exactly one device-to-host read, after the last chain
    assert [res["num_gt"], res["tp"], res["fp"], res["num_det"]] == want.tolist()
    assert res["protocol"] == "icdar15" and res["invalid_gt"] == 0 and res["images"] == 3
    assert want[1] >= 3 and want[0] == 6                                    # each image's best detection is its own ground truth
    assert (res["precision"], res["recall"]) == metrics.precision_recall(want[0], want[1], want[2])
    assert evaluate.format_line(res).endswith(" [icdar15]")


def _same_last(a, b):
    """every tensor of `last` bit for bit; of dets / det_score the rows below nd (ocr_eval_collect writes nothing beyond)"""
    assert sorted(a) == sorted(b) == sorted(["dets", "det_score", "nd", "nd_total", "tp", "fp", "gts", "ng"])
    assert torch.equal(a["nd"], b["nd"])
    live = torch.arange(a["dets"].shape[1], device=a["nd"].device)[None, :] < a["nd"][:, None]
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        x, y = (a[k][live], b[k][live]) if k in ("dets", "det_score") else (a[k], b[k])
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), k


def test_evaluator_icdar15_equals_the_reference_and_raster_is_untouched(device, graph, rbox_eval_dir, monkeypatch):
    from tensorflow_ocr_amd import evaluate
    d, maps, _ = rbox_eval_dir
    forward, calls = E.rbox_stub_forward(device, maps)
    ev = evaluate.Evaluator(graph, forward, d, batch_size=2, protocol="icdar15")
    res, reads, want = _chain_case(ev, calls, monkeypatch)
    assert ev.acc.reads == 1
    _check_chain(evaluate, res, reads, want, 2)
    plain, raster = evaluate.Evaluator(graph, forward, d, batch_size=2), evaluate.Evaluator(graph, forward, d, batch_size=2, protocol="raster")
    ra, rb = plain.run(), raster.run()
    assert ra == rb and "protocol" not in rb and "invalid_gt" not in rb
    _same_last(plain.last, raster.last)


def test_link_evaluator_icdar15_equals_the_reference_and_raster_is_untouched(device, graph, link_eval_dir, monkeypatch):
    from tensorflow_ocr_amd import evaluate
    d, maps = link_eval_dir
    forward, calls = E.link_stub_forward(device, maps)
    kw = dict(batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL)
    ev = evaluate.LinkEvaluator(graph, forward, d, protocol="icdar15", **kw)
    res, reads, want = _chain_case(ev, calls, monkeypatch)
    assert ev.acc.reads == 1
    _check_chain(evaluate, res, reads, want, 2)
    plain, raster = evaluate.LinkEvaluator(graph, forward, d, **kw), evaluate.LinkEvaluator(graph, forward, d, protocol="raster", **kw)
    ra, rb = plain.run(), raster.run()
    assert ra == rb and "protocol" not in rb
    _same_last(plain.last, raster.last)
