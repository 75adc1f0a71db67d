"""GPU: ocr_eval_match_batch / ocr_eval_record_init (csrc/eval_match.hip, tool/bboxes.bboxes_matching_batch,
tool/metrics.DeviceTpFp) against oracle/evalboxes.py per image.  tp, fp and the record are integers: everything is exact.
Shapes n = 3, max_d = 16, max_g = 8, coordinates inside 64 x 64; the thresholds (0.25, 0.5, 0.75) are f32 numbers, so
the kernel's f32 comparison and the oracle's agree.  The cases are tests/test_eval_match_host.directed_cases, which the
CPU tests pin against the oracle and against answers worked out by hand."""
import ctypes

import numpy as np
import pytest
import torch

import test_eval_match_host as H

pytestmark = pytest.mark.gpu
MAX_D, MAX_G, N = H.MAX_D, H.MAX_G, 3
SENT = 0xA5
CASES = H.directed_cases()


def _pack(images, device, pad_rows=2):
    """3 images -> device tensors; rows beyond a count hold junk that must not be read as data"""
    dets = np.full((N, MAX_D, 4, 2), 7777, np.int32)
    gts = np.full((N, MAX_G, 4, 2), -7777, np.int32)
    nd, ng = np.zeros(N, np.int32), np.zeros(N, np.int32)
    ign = np.full((N, MAX_G), 1, np.uint8)
    for i, (d, g, ig) in enumerate(images):
        dets[i, :len(d)], gts[i, :len(g)], ign[i, :len(g)] = d, g, ig
        nd[i], ng[i] = len(d), len(g)
    up = lambda a: torch.from_numpy(a).to(device)
    return up(dets), up(nd), up(gts), up(ng), up(ign)


def _expected(images, thr):
    tp, fp = np.zeros((N, MAX_D), np.uint8), np.zeros((N, MAX_D), np.uint8)
    rec = np.zeros(4, np.int64)
    for i, (d, g, ig) in enumerate(images):
        n_g, t, f = H.oracle_image(d, g, ig, thr)
        tp[i, :len(d)], fp[i, :len(d)] = t, f
        rec += [n_g, int(t.sum()), int(f.sum()), len(d)]
    return tp, fp, rec


def _outputs(device):
    """tp / fp with a sentinel tail behind [n][max_d]"""
    buf = torch.full((2, N * MAX_D + 64), SENT, dtype=torch.uint8, device=device)
    return buf, buf[0, :N * MAX_D].view(N, MAX_D), buf[1, :N * MAX_D].view(N, MAX_D)


@pytest.fixture(scope="module")
def expected():
    return {name: _expected(images, thr) for name, (thr, images, _) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_match_batch_equals_the_oracle(device, expected, name):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.graph import Graph
    thr, images, by_hand = CASES[name]
    g = Graph(device)
    dets, nd, gts, ng, ign = _pack(images, device)
    buf, tp, fp = _outputs(device)
    rec = torch.full((6,), -99, dtype=torch.int64, device=device)
    ops.eval_record_init(rec[:4])
    ops.eval_match_batch(dets, nd, gts, ng, ign, thr, 74, 74, tp, fp, rec[:4], g.workspace())
    torch.cuda.synchronize()
    etp, efp, erec = expected[name]
    print("eval match %s: record %s" % (name, rec[:4].tolist()))
    assert np.array_equal(tp.cpu().numpy(), etp) and np.array_equal(fp.cpu().numpy(), efp)
    assert rec[:4].tolist() == erec.tolist() and rec[4:].tolist() == [-99, -99]
    assert (buf[:, N * MAX_D:] == SENT).all()                               # nothing beyond [n][max_d]
    if by_hand is not None:
        for i, (t, f) in enumerate(by_hand):
            assert tp[i, :len(t)].tolist() == t and fp[i, :len(f)].tolist() == f


def test_tool_wrapper_and_device_record_add_up_over_calls(device, expected):
    """bboxes_matching_batch + DeviceTpFp: two successive calls on the same record give the sum of both; the mask only has
    to hold every vertex (the default, 32768 x 32768, gives the same counts); one read."""
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import bboxes, metrics
    g = Graph(device)
    acc = metrics.DeviceTpFp(g)
    total = np.zeros(4, np.int64)
    for name, mask_hw in (("random", None), ("full_empty_no_gt", (64, 64)), ("nan_pair", (200, 90))):
        thr, images, _ = CASES[name]
        dets, nd, gts, ng, ign = _pack(images, device)
        tp, fp, rec = bboxes.bboxes_matching_batch(dets, nd, gts, ng, ign.bool(), thr, record=acc.record, graph=g, mask_hw=mask_hw)
        assert rec is acc.record
        etp, efp, erec = expected[name]
        assert np.array_equal(tp.cpu().numpy(), etp) and np.array_equal(fp.cpu().numpy(), efp), name
        total += erec
    assert acc.reads == 0
    assert acc.value() == tuple(int(v) for v in total) and acc.reads == 1
    p, r = metrics.precision_recall(*acc.value()[:3])
    assert p == total[1] / (total[1] + total[2]) and r == total[1] / total[0]
    acc.reset()
    assert acc.value() == (0, 0, 0, 0)
    # without a record the call makes a zeroed one of its own
    thr, images, _ = CASES["random"]
    _, _, rec = bboxes.bboxes_matching_batch(*_pack(images, device), thr, graph=g)
    assert rec.tolist() == expected["random"][2].tolist()


def test_every_status_code_leaves_the_outputs_alone(device):
    from tensorflow_ocr_amd import _lib as L
    thr, images, _ = CASES["random"]
    dets, nd, gts, ng, ign = _pack(images, device)
    buf, tp, fp = _outputs(device)
    rec = torch.full((4,), -99, dtype=torch.int64, device=device)
    nbytes = L.call_size("ocr_eval_match_workspace", ctypes.c_int(N), ctypes.c_int(MAX_D), ctypes.c_int(MAX_G))
    assert nbytes == N * MAX_D * MAX_G * 8
    ws = torch.full((nbytes,), SENT, dtype=torch.uint8, device=device)
    fn = L._fn("ocr_eval_match_batch", ctypes.c_int)
    F, SZ, p = ctypes.c_float, ctypes.c_size_t, L.ptr

    def call(dets=dets, nd=nd, gts=gts, ng=ng, ign=ign, n=N, d=MAX_D, gg=MAX_G, mh=74, mw=74, tp=tp, fp=fp, rec=rec, ws=ws, wsb=nbytes):
        return fn(p(dets), p(nd), p(gts), p(ng), p(ign), n, d, gg, F(thr), mh, mw, p(tp), p(fp), p(rec), p(ws), SZ(wsb), L.stream_ptr())
    for kw in (dict(dets=None), dict(nd=None), dict(gts=None), dict(ng=None), dict(ign=None), dict(tp=None), dict(fp=None),
               dict(rec=None), dict(ws=None), dict(n=0), dict(d=0), dict(gg=-1), dict(mh=0), dict(mw=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(d=1025), dict(gg=255), dict(n=65536), dict(mh=32769), dict(mw=32769)):
        assert call(**kw) == -2, kw
    assert call(wsb=nbytes - 1) == -4 and call(wsb=0) == -4
    assert L._fn("ocr_eval_record_init", ctypes.c_int)(None, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (ws == SENT).all() and rec.tolist() == [-99] * 4
    assert call() == 0                                                      # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert rec.tolist() == (np.array([-99] * 4) + _expected(images, thr)[2]).tolist()      # added to, not overwritten
