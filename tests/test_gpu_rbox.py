"""GPU: the EAST RBOX geometry (csrc/rbox.hip, tool/rbox.py, model_vgg_16.model_rbox / loss_rbox, test.py --geometry RBOX)
against float64 restatements written here from the formulas of include/ocr_hip.h (NumPy, torch autograd in float64); the
decode restatement is tests/test_rbox_host.decode_ref, which the CPU tests hold to answers worked out by hand.

Bounds (all from the number formats, none from what the kernels give):
  head forward   rtol 2e-6 = 16 f32 ulp (one expf / tanhf, one divide, one scale)
  head backward  rtol 1e-4: 1 - sigma >= 0.018 on z in [-4, 4], so sigma recovered from the stored output carries its
                 6e-8 rounding as at most 3e-6 of sigma (1 - sigma); the rest is margin
  decode         counts, total, order and the score column exact; coordinates 4e-3 px (magnitudes < 4096: ulp 2.4e-4,
                 a sin / cos and about five multiply-adds: 16 ulp)
  decode->LANMS  bit for bit against oracle/lanms on the downloaded quads of the same decode
  loss           out[0..3] 1e-5 relative; gradients rtol 1e-4, atol 1e-7 (A_u >= max(A_g, A_p): no cancellation)
  graph          head-variable gradients against float64 computed from the downloaded merge-branch feature (z = x W + b,
                 head, loss, autograd): the bar of tests/test_gpu_heads_matrix.py for the two kernels head_conv_bias runs,
                 |dev - ref| <= g(m) S and nothing else — m the sequential f32 roundings of the route (narrow weight
                 gradient, column sum), S the float64 sum of |terms|.  The same for the per-head path
                 (OCR_RESNET_MERGE_HEADS=0) and for the 4- and 6-column narrow weight-gradient instances called directly.
  f32 precision  forward only: outputs within the activation's largest slope times g(2 cin + 1) (|x| |W| + |b|), plus the
                 head's 2e-6

Measured on the MI355X, largest |err| / bound (f16 library): head score 0.058, geo 0.077, dz 0.044; decode coordinates
0.015 (6.0e-5 px); loss out 0.003, d_cls < 0.001, d_geo 0.001; graph loss < 0.001, dW 0.048, db 0.031; per-head dW 0.021 /
0.048 / 0.021, db 0.004 / 0.040 / < 0.001; f32 heads 0.028; narrow weight gradient called directly 0.006 to 0.009.
"""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_rbox_host as H
from matrix_support import _cdiv, _g as _gm, _h as _h16
from oracle import lanms as OL
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
SENT = f32(-12345.5)
SMALL = [("block1", [(128, 64, 1), (128, 64, 2)]), ("block2", [(256, 64, 1), (256, 64, 2)]),
         ("block3", [(256, 128, 1), (256, 128, 2)]), ("block4", [(512, 128, 1)])]


def _d(a, device, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _within(got, ref, rtol, atol=0.0, what=""):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = np.abs(got - ref), rtol * np.abs(ref) + atol
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("rbox %s: largest |err| / bound = %.3f (max |err| %.3e)" % (what, worst, float(err.max()) if err.size else 0.0))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, worst)


# ------------------------------------------------------------------------------------------------ head
def _head_ref(z, ts):
    """torch float64: (score [P], geo [P,5]) of z [P,6]"""
    s = torch.sigmoid(z)
    return s[:, 0], torch.cat([s[:, 1:5] * ts, (s[:, 5:6] - 0.5) * (math.pi / 2)], dim=1)


def test_head_forward_backward(device):
    from tensorflow_ocr_amd import ops
    P, ts = 1000, 512.0                                   # 3 full workgroups + a tail of 232
    rng = np.random.default_rng(11)
    z = rng.uniform(-4, 4, (P, 6)).astype(f32)
    dscore, dgeo = rng.standard_normal(P).astype(f32), rng.standard_normal((P, 5)).astype(f32)
    zd = _d(z, device)
    score = torch.full((P + 64,), float(SENT), device=device)
    geo = torch.full((P + 64, 5), float(SENT), device=device)
    ops.rbox_head_fwd(zd, ts, score[:P], geo[:P])
    z64 = torch.from_numpy(z.astype(f64)).requires_grad_(True)
    rs, rg = _head_ref(z64, ts)
    _within(score[:P].cpu().numpy(), rs.detach().numpy(), 2e-6, what="head score")
    _within(geo[:P].cpu().numpy(), rg.detach().numpy(), 2e-6, what="head geo")
    assert (score[P:] == float(SENT)).all() and (geo[P:] == float(SENT)).all()          # nothing beyond P
    g = geo[:P].cpu().numpy()
    assert (g[:, :4] > 0).all() and (g[:, :4] < ts).all() and (np.abs(g[:, 4]) < math.pi / 4).all()
    ((rs * torch.from_numpy(dscore.astype(f64))).sum() + (rg * torch.from_numpy(dgeo.astype(f64))).sum()).backward()
    ref = z64.grad.numpy()
    s_in, g_in = score[:P].contiguous(), geo[:P].contiguous()
    pad = torch.full((P + 64, 6), float(SENT), device=device)
    dz = pad[:P]
    ops.rbox_head_bwd(s_in, _d(dscore, device), g_in, _d(dgeo, device), ts, dz)
    _within(dz.cpu().numpy(), ref, 1e-4, what="head dz")
    assert (pad[P:] == float(SENT)).all()
    ops.rbox_head_bwd(s_in, _d(dscore, device), g_in, None, ts, dz)                     # NULL dgeo: zeros
    got = dz.cpu().numpy()
    assert (got[:, 1:] == 0).all()
    _within(got[:, 0], ref[:, 0], 1e-4, what="head dz0, dgeo NULL")
    ops.rbox_head_bwd(s_in, None, g_in, _d(dgeo, device), ts, dz)                       # NULL dscore
    got = dz.cpu().numpy()
    assert (got[:, 0] == 0).all()
    _within(got[:, 1:], ref[:, 1:], 1e-4, what="head dz1..5, dscore NULL")


# ------------------------------------------------------------------------------------------------ decode
N, HH, WW, THR = 2, 37, 53, 0.7


@pytest.fixture(scope="module")
def decode_case():
    """maps, and the float64 rows of image 0 (computed once, read by every decode test)"""
    rng = np.random.default_rng(21)
    score = rng.uniform(0, 1, (N, HH, WW)).astype(f32)
    thr = f32(THR)
    ys, xs = rng.integers(0, HH, 24), rng.integers(0, WW, 24)
    score[0, ys, xs] = thr                                               # exactly the threshold: not selected
    score[1] = np.minimum(score[1], thr) * f32(0.99)                     # image 1: nothing above
    score[1, 5, 7] = thr
    geo = np.zeros((N, HH, WW, 5), f32)
    geo[..., :4] = rng.uniform(1, 200, (N, HH, WW, 4))
    geo[..., 4] = rng.uniform(-0.78, 0.78, (N, HH, WW))
    geo[..., 4][rng.uniform(size=(N, HH, WW)) < 0.1] = 0.0               # angles of both signs, some exactly 0
    ref = H.decode_ref(score[0], geo[0], thr)
    sel = score[0] > thr
    assert 0.25 < sel.mean() < 0.35 and len(ref) == sel.sum() and not (score[1] > thr).any()
    a = geo[0][sel][:, 4]
    assert (a > 0).any() and (a < 0).any() and (a == 0).any()
    assert np.abs(ref[:, :8]).max() < 4096
    return score, geo, ref


def _decode(device, score, geo, max_k):
    from tensorflow_ocr_amd import ops
    pad = torch.full((N * max_k * 9 + 64,), float(SENT), device=device)                 # rows + a guard band behind them
    boxes = pad[:N * max_k * 9].view(N, max_k, 9)
    counts = torch.full((N,), -7, dtype=torch.int32, device=device)
    total = torch.full((N,), -7, dtype=torch.int32, device=device)
    ops.rbox_decode(_d(score, device), _d(geo, device), N, HH, WW, THR, 4.0, boxes, counts, total,
                    ops.Workspace(device, 1 << 16))
    torch.cuda.synchronize()
    assert (pad[N * max_k * 9:] == float(SENT)).all()
    return boxes.cpu().numpy(), counts.cpu().numpy(), total.cpu().numpy()


def test_decode_raster_order_counts_and_coordinates(device, decode_case):
    score, geo, ref = decode_case
    k = len(ref)
    boxes, counts, total = _decode(device, score, geo, HH * WW)
    assert counts.tolist() == [k, 0] and total.tolist() == [k, 0]
    got = boxes[0, :k]
    assert np.array_equal(got[:, 8].view(np.int32), score[0][score[0] > f32(THR)].view(np.int32))   # raster order, bitwise
    _within(got[:, :8], ref[:, :8], 0.0, 4e-3, what="decode coordinates")
    assert (boxes[0, k:].view(np.int32) == SENT.view(np.int32)).all() and (boxes[1].view(np.int32) == SENT.view(np.int32)).all()


def test_decode_overflow_keeps_the_first_rows_and_the_true_total(device, decode_case):
    score, geo, ref = decode_case
    k = len(ref)
    full, _, _ = _decode(device, score, geo, HH * WW)
    max_k = k // 2
    boxes, counts, total = _decode(device, score, geo, max_k)
    assert counts.tolist() == [max_k, 0] and total.tolist() == [k, 0]
    assert np.array_equal(boxes[0].view(np.int32), full[0, :max_k].view(np.int32))
    assert (boxes[1].view(np.int32) == SENT.view(np.int32)).all()


def test_decode_status_codes(device, decode_case):
    from tensorflow_ocr_amd import _lib as L
    score, geo, _ = decode_case
    fn = L._fn("ocr_rbox_decode", ctypes.c_int)
    sd, gd = _d(score, device), _d(geo, device)
    boxes = torch.full((N, 16, 9), float(SENT), device=device)
    cnt = torch.full((2 * N,), -7, dtype=torch.int32, device=device)
    ws = torch.full((64,), -7, dtype=torch.int32, device=device)
    need = L.call_size("ocr_rbox_decode_workspace", ctypes.c_int(N), ctypes.c_int(HH), ctypes.c_int(WW))
    assert need == N * 8 * 4
    p, F, SZ = L.ptr, ctypes.c_float, ctypes.c_size_t

    def rc(score_p, h, nbytes):
        return fn(score_p, p(gd), N, h, WW, F(THR), F(4.0), 16, p(boxes), p(cnt[:N]), p(cnt[N:]), p(ws), SZ(nbytes), L.stream_ptr())
    assert rc(p(None), HH, need) == -1
    assert rc(p(sd), 0, need) == -1
    assert rc(p(sd), HH, need - 1) == -4
    torch.cuda.synchronize()
    assert (boxes == float(SENT)).all() and (cnt == -7).all() and (ws == -7).all()      # nothing written on error
    assert rc(p(sd), HH, need) == 0
    torch.cuda.synchronize()
    assert cnt[:N].tolist() == [16, 0]


# ------------------------------------------------------------------------------------------------ decode -> LANMS
def test_detect_equals_lanms_oracle_on_the_decoded_quads(device):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import rbox
    g = Graph(device)
    rng = np.random.default_rng(31)
    label, geo, _ = synthetic.rbox_labels(2, 256, rng)                   # 64 x 64 maps
    score = (label[..., 0] * rng.uniform(0.85, 1.0, label.shape[:3])).astype(f32)
    geo = geo.copy()
    geo[..., :4] += (label * rng.uniform(-1.5, 1.5, geo[..., :4].shape)).astype(f32)     # per-pixel regression noise
    geo[..., 4] += (label[..., 0] * rng.uniform(-0.02, 0.02, label.shape[:3])).astype(f32)
    boxes, counts, total = rbox.decode(score, geo, graph=g)
    boxes, counts, total = boxes.cpu().numpy(), counts.cpu().numpy(), total.cpu().numpy()
    assert boxes.shape == (2, 4096, 9) and counts.tolist() == total.tolist() == (score > f32(0.8)).sum(axis=(1, 2)).tolist()
    assert counts[0] != counts[1] and counts.min() > 100
    kept = rbox.detect(score, geo, graph=g)
    assert len(kept) == 2
    for i in range(2):
        om, ok = OL.lanms(boxes[i, :counts[i]], 0.2)
        assert 0 < len(ok) < counts[i]
        assert kept[i].shape == (len(ok), 9) and np.array_equal(kept[i].view(np.int32), om[ok].view(np.int32))
    with pytest.raises(ValueError, match="max_k"):
        rbox.detect(score, geo, max_k=int(counts.max()) - 1, graph=g)


# ------------------------------------------------------------------------------------------------ loss
def _loss_ref(y, p, gt, gp, m):
    """torch float64, the formulas of include/ocr_hip.h; maps flattened to [P] / [P,5]"""
    P = y.numel()
    l_cls = 0.01 * (1 - 2 * (y * p * m).sum() / ((y * m).sum() + (p * m).sum() + 1e-5))
    a_g, a_p = (gt[:, 0] + gt[:, 2]) * (gt[:, 1] + gt[:, 3]), (gp[:, 0] + gp[:, 2]) * (gp[:, 1] + gp[:, 3])
    w = torch.minimum(gt[:, 1], gp[:, 1]) + torch.minimum(gt[:, 3], gp[:, 3])
    h = torch.minimum(gt[:, 0], gp[:, 0]) + torch.minimum(gt[:, 2], gp[:, 2])
    a_i = w * h
    a_u = a_g + a_p - a_i
    aabb = (-torch.log((a_i + 1) / (a_u + 1)) * y * m).sum() / P
    theta = ((1 - torch.cos(gp[:, 4] - gt[:, 4])) * y * m).sum() / P
    return aabb + 20 * theta + l_cls, l_cls, aabb, theta


@pytest.fixture(scope="module")
def loss_case():
    from tensorflow_ocr_amd import synthetic
    rng = np.random.default_rng(41)
    y, gt, _ = synthetic.rbox_labels(2, 92, rng)                          # 23 x 23 maps: P = 1058, two workgroups
    y, gt = y.reshape(-1), gt.reshape(-1, 5)
    P = y.size
    assert P == 1058 and 50 < y.sum() < P - 50
    p = rng.uniform(0.05, 0.95, P).astype(f32)
    gp = np.empty((P, 5), f32)
    gp[:, :4] = gt[:, :4] * rng.uniform(0.6, 1.4, (P, 4)) + rng.uniform(0.5, 3.0, (P, 4))
    gp[:, 4] = gt[:, 4] + rng.uniform(-0.3, 0.3, P)
    assert not (gp[:, :4] == gt[:, :4]).any()                              # no ties of the minimum
    m = (rng.uniform(size=P) < 0.8).astype(f32)
    t = [torch.from_numpy(a.astype(f64)) for a in (y, p, gt, gp, m)]
    t[1].requires_grad_(True)
    t[3].requires_grad_(True)
    out = _loss_ref(*t)
    out[0].backward()
    ref = dict(out=np.array([v.item() for v in out]), d_cls=t[1].grad.numpy().copy(), d_geo=t[3].grad.numpy().copy())
    return y, p, gt, gp, m, ref


def _loss_run(device, y, p, gt, gp, m, grad_scale=1.0, dyn=None):
    from tensorflow_ocr_amd import ops
    yd, pd, gtd, gpd, md = (_d(a, device) for a in (y, p, gt, gp, m))
    sums, out = torch.full((5,), float(SENT), device=device), torch.full((4,), float(SENT), device=device)
    ops.rbox_loss_fwd(yd, pd, gtd, gpd, md, sums, out, ops.Workspace(device, 1 << 16))
    d_cls, d_geo = torch.full_like(pd, float(SENT)), torch.full_like(gpd, float(SENT))
    if dyn is None:
        ops.rbox_loss_bwd(yd, gtd, gpd, md, sums, grad_scale, d_cls, d_geo)
    else:
        ops.rbox_loss_bwd_dyn(yd, gtd, gpd, md, sums, grad_scale, dyn, d_cls, d_geo)
    return out.cpu().numpy(), d_cls.cpu().numpy(), d_geo.cpu().numpy()


def test_loss_forward_backward(device, loss_case):
    y, p, gt, gp, m, ref = loss_case
    out, d_cls, d_geo = _loss_run(device, y, p, gt, gp, m)
    _within(out, ref["out"], 1e-5, what="loss out")
    assert ref["out"][2] > 1e-3 and ref["out"][3] > 1e-5                  # both geometry terms are live
    _within(d_cls, ref["d_cls"], 1e-4, 1e-7, what="loss d_cls")
    _within(d_geo, ref["d_geo"], 1e-4, 1e-7, what="loss d_geo")
    off = (y * m) == 0
    assert off.any() and (d_geo[off] == 0).all() and (d_geo[~off] != 0).any()


def test_loss_without_positives_is_the_dice_constant(device, loss_case):
    y, p, gt, gp, m, _ = loss_case
    out, d_cls, d_geo = _loss_run(device, np.zeros_like(y), p, gt, gp, m)
    _within(out, [0.01, 0.01, 0.0, 0.0], 1e-5, what="loss, y = 0")
    assert np.isfinite(d_cls).all() and np.isfinite(d_geo).all() and (d_geo == 0).all()


def test_loss_dynamic_seed_equals_the_static_product(device, loss_case):
    y, p, gt, gp, m, _ = loss_case
    scale = torch.tensor([1024.0], device=device)
    a = _loss_run(device, y, p, gt, gp, m, grad_scale=0.5 * 1024.0)
    b = _loss_run(device, y, p, gt, gp, m, grad_scale=0.5, dyn=scale)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32), v.view(np.int32))


# ------------------------------------------------------------------------------------------------ graph
HEAD = "feature_fusion/Conv_7+Conv_8+Conv_9/"
MERGED = [(HEAD, 0, 6)]
PER_HEAD = [("feature_fusion/Conv_7/", 0, 1), ("feature_fusion/Conv_8/", 1, 4), ("feature_fusion/Conv_9/", 5, 1)]
LOSS_SCALE, TEXT_SCALE = 1024.0, 512.0


@pytest.fixture(scope="module")
def graph_case():
    from tensorflow_ocr_amd import synthetic
    rng = np.random.default_rng(51)
    images = rng.uniform(0, 255, (2, 64, 64, 3)).astype(f32)
    y, gt, m = synthetic.rbox_labels(2, 64, rng)
    return images, y, gt, m


def _forward(device, case, heads, **graph_kw):
    """model_rbox + loss_rbox on the reduced net; asserts shapes, ranges and the head variables' names"""
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    batch = [_d(a, device) for a in case]
    g = Graph(device, loss_scale=LOSS_SCALE, seed=6, **graph_kw)
    fs, fg = M.model_rbox(batch[0], graph=g, blocks=SMALL)
    assert fs.data.shape == (2, 16, 16, 1) and fg.data.shape == (2, 16, 16, 5)
    L = M.loss_rbox(batch[1], fs, batch[2], fg, batch[3], graph=g)
    assert g.collections["losses"][-1] is L
    names = [k for k in g.store.order if "Conv_7" in k or "Conv_8" in k or "Conv_9" in k]
    assert names == [h + v for h, _, _ in heads for v in ("weights", "biases")]
    return g, fs, fg, L


def _ranges(fs, fg):
    s_h, g_h = fs.data.cpu().numpy(), fg.data.cpu().numpy()
    assert (s_h > 0).all() and (s_h < 1).all() and (g_h[..., :4] > 0).all() and (g_h[..., :4] < TEXT_SCALE).all()
    assert (np.abs(g_h[..., 4]) < math.pi / 4).all()
    return s_h, g_h


def _reference(g, heads, case, round_w):
    """float64 from the DOWNLOADED merge-branch feature: z = x W + b (W as the convolution reads it: rounded to the
    16-bit storage type on the f16 path), the head, the loss, and dz by autograd.  Returns x, W, b, (score, geo), out, dz."""
    _, y, gt, m = case
    x = g.end_points["feature_fusion"].data.float().cpu().numpy().reshape(-1, 32).astype(f64)
    P = x.shape[0]
    w = np.concatenate([g.store.vars[h + "weights"].data.cpu().numpy() for h, _, _ in heads], axis=1)
    b = np.concatenate([g.store.vars[h + "biases"].data.cpu().numpy() for h, _, _ in heads])
    assert w.shape == (32, 6) and b.shape == (6,)
    w = (_h16(w) if round_w else w).astype(f64)
    z = (torch.from_numpy(x) @ torch.from_numpy(w) + torch.from_numpy(b.astype(f64))).requires_grad_(True)
    rs, rg = _head_ref(z, TEXT_SCALE)
    t = [torch.from_numpy(a.reshape(P, -1).astype(f64)) for a in (y, gt, m)]
    out = _loss_ref(t[0][:, 0], rs, t[1], rg, t[2][:, 0])
    out[0].backward()
    return x, w, b.astype(f64), (rs.detach().numpy(), rg.detach().numpy()), [v.item() for v in out], z.grad.numpy()


def _narrow_m(P, cin):
    """sequential f32 roundings of conv1x1_small_wgrad_narrow_kernel + ocr_sum_rows_kernel (tests/test_gpu_heads_matrix.py)"""
    S_, lanes = _cdiv(P, 1024), 256 // (cin // 8)
    return 2 * _cdiv(_cdiv(P, S_), lanes) + lanes + _cdiv(S_, 64) + 6


def _colsum_m(P, C):
    """the same for ocr_sc_colsum"""
    lanes = 256 // C
    T = max(min(_cdiv(P, lanes * 8), 1024), 1)
    return _cdiv(P, T * lanes) + lanes + _cdiv(T, 64) + 6


def _bar(tag, got, ref, m, S):
    """the heads-matrix bar for an f32 output: |dev - ref| <= g(m) S (+ 2^-149)"""
    err, bound = np.abs(np.asarray(got, f64) - ref), _gm(m) * S + 2.0 ** -149
    print("rbox %s: largest |err| / bound = %.3f" % (tag, float((err / bound).max())))
    assert got.shape == ref.shape and (S > 0).all() and (err <= bound).all(), tag


def _check_head_gradients(g, heads, x, dz, tag):
    P = x.shape[0]
    for h, c0, c in heads:
        d = dz[:, c0:c0 + c]
        wv, bv = g.store.vars[h + "weights"], g.store.vars[h + "biases"]
        _bar("%s dW %s" % (tag, h), wv.grad.cpu().numpy().astype(f64) / LOSS_SCALE, x.T @ d, _narrow_m(P, 32), np.abs(x).T @ np.abs(d))
        _bar("%s db %s" % (tag, h), bv.grad.cpu().numpy().astype(f64) / LOSS_SCALE, d.sum(0), _colsum_m(P, c), np.abs(d).sum(0))


def test_model_rbox_graph_trains_and_its_head_gradients_match_float64(device, graph_case):
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    # eager: one forward / backward, the head variables' gradients against float64 from the downloaded feature
    g, fs, fg, L = _forward(device, graph_case, MERGED)
    g.backward()
    torch.cuda.synchronize()
    _ranges(fs, fg)
    x, _, _, _, out, dz = _reference(g, MERGED, graph_case, round_w=True)
    _within(L.data.cpu().numpy(), out, 1e-4, 1e-7, what="graph loss")
    _check_head_gradients(g, MERGED, x, dz, "graph")
    # recorded: two eager steps, the third is recorded, the fourth replays the plan
    batch = [_d(a, device) for a in graph_case]

    def fl(gr, im, yy, gg, mm):
        a, b = M.model_rbox(im, graph=gr, blocks=SMALL)
        return M.loss_rbox(yy, a, gg, b, mm, graph=gr)
    g2 = Graph(device, loss_scale=LOSS_SCALE, seed=6)
    step = TrainStep(g2, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3))
    losses = [step(*batch).item() for _ in range(4)]
    assert step.plan is not None and np.isfinite(losses).all()
    assert abs(losses[0] - L.item()) <= 1e-6 * abs(L.item())                    # the same graph from the same seed


def test_per_head_convolutions_give_the_same_gradients_bar(device, graph_case, monkeypatch):
    """OCR_RESNET_MERGE_HEADS=0: three convolutions (variables Conv_7, Conv_8, Conv_9), the activation kernel on their
    concatenation, the backward scattered into the three — against the same float64 reference and the same bar; the
    path refuses a recorded step."""
    from tensorflow_ocr_amd import head_layers as R
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    monkeypatch.setattr(R, "MERGE_HEADS", False)
    g, fs, fg, L = _forward(device, graph_case, PER_HEAD)
    g.backward()
    torch.cuda.synchronize()
    _ranges(fs, fg)
    x, _, _, _, out, dz = _reference(g, PER_HEAD, graph_case, round_w=True)
    _within(L.data.cpu().numpy(), out, 1e-4, 1e-7, what="per-head loss")
    _check_head_gradients(g, PER_HEAD, x, dz, "per-head")
    batch = [_d(a, device) for a in graph_case]

    def fl(gr, im, yy, gg, mm):
        a, b = M.model_rbox(im, graph=gr, blocks=SMALL)
        return M.loss_rbox(yy, a, gg, b, mm, graph=gr)
    step = TrainStep(Graph(device, loss_scale=LOSS_SCALE, seed=6), fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3))
    assert np.isfinite([step(*batch).item() for _ in range(2)]).all()           # eager steps run
    with pytest.raises(NotImplementedError, match="recorded step"):
        step(*batch)                                                            # the third call records


def test_f32_precision_forward_matches_float64(device, graph_case):
    """Graph(precision="f32") (forward only) takes the per-head path with f32 convolutions.  z = x W + b against
    float64 of the downloaded f32 feature within g(2 cin + 1) (|x| |W| + |b|): cin products and additions, not
    necessarily fused, and the bias; the outputs within that times the activation's largest slope (1/4 for the sigmoid:
    text_scale / 4 for a distance, pi / 8 for the angle) plus the head's own 2e-6."""
    g, fs, fg, L = _forward(device, graph_case, PER_HEAD, precision="f32")
    torch.cuda.synchronize()
    s_h, g_h = _ranges(fs, fg)
    x, w, b, (rs, rg), out, _ = _reference(g, PER_HEAD, graph_case, round_w=False)
    zb = _gm(2 * 32 + 1) * (np.abs(x) @ np.abs(w) + np.abs(b))                  # [P, 6]
    slope = np.array([0.25] + [TEXT_SCALE / 4] * 4 + [math.pi / 8])
    got = np.concatenate([s_h.reshape(-1, 1), g_h.reshape(-1, 5)], axis=1).astype(f64)
    ref = np.concatenate([rs.reshape(-1, 1), rg], axis=1)
    err, bound = np.abs(got - ref), slope * zb + 2e-6 * np.abs(ref)
    print("rbox f32 heads: largest |err| / bound = %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    _within(L.data.cpu().numpy(), out, 1e-4, 1e-7, what="f32 loss")
    with pytest.raises(NotImplementedError):
        g.backward()


@pytest.mark.parametrize("P,cout", [(1025, 6), (1025, 4), (512, 4)])
def test_narrow_weight_gradient_instances_for_the_rbox_heads(device, P, cout):
    """ocr_conv1x1_small_wgrad_f16 at cin = 32 with the 4- and 6-column instances the RBOX heads added (one and two
    strips), against float64 with the bar of tests/test_gpu_heads_matrix.py; the strip route still has neither."""
    from tensorflow_ocr_amd import _lib as L
    rng = np.random.default_rng(1000 * cout + P)
    x = _h16(rng.standard_normal((P, 32)))
    dz = rng.standard_normal((P, cout)).astype(f32)
    xd, dzd = _d(x, device, O.STORAGE), _d(dz, device)
    ci, SZ = ctypes.c_int, ctypes.c_size_t
    nbytes = L.call_size("ocr_conv1x1_small_wgrad_workspace", ci(P), ci(32), ci(cout))
    assert nbytes == _cdiv(P, 1024) * 32 * cout * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    pad = torch.full((32 * cout + 64,), float(SENT), device=device)
    fn = L._fn("ocr_conv1x1_small_wgrad_f16", ctypes.c_int)
    assert fn(L.ptr(xd), L.ptr(dzd), P, 32, cout, L.ptr(pad), L.ptr(ws), SZ(nbytes), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (pad[32 * cout:] == float(SENT)).all()
    x64, d64 = x.astype(f64), dz.astype(f64)
    _bar("narrow wgrad P%d cout%d" % (P, cout), pad[:32 * cout].view(32, cout).cpu().numpy().astype(f64), x64.T @ d64,
         _narrow_m(P, 32), np.abs(x64).T @ np.abs(d64))
    x40 = torch.zeros((P, 40), dtype=O.STORAGE, device=device)                  # cin = 40: the strip route
    ws40 = torch.empty(1 << 20, dtype=torch.uint8, device=device)
    assert fn(L.ptr(x40), L.ptr(dzd), P, 40, cout, L.ptr(pad), L.ptr(ws40), SZ(1 << 20), L.stream_ptr()) == -2


def test_model_is_unchanged_by_model_rbox(device):
    """`model` (1 + 8 sigmoid heads) before and after `model_rbox` was built in this process: same variables in the same
    order, same outputs bit for bit; the two nets share every variable but the heads'."""
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    images = np.random.default_rng(61).uniform(0, 255, (2, 64, 64, 3)).astype(f32)

    def build(fn):
        g = Graph(device, seed=9)
        a, b = fn(images, graph=g, blocks=SMALL)
        torch.cuda.synchronize()
        return list(g.store.order), a.data.cpu().numpy(), b.data.cpu().numpy()
    o1, s1, g1 = build(M.model)
    orb, _, grb = build(M.model_rbox)
    o2, s2, g2 = build(M.model)
    assert o1 == o2 and np.array_equal(s1.view(np.int32), s2.view(np.int32)) and np.array_equal(g1.view(np.int32), g2.view(np.int32))
    assert g1.shape == (2, 16, 16, 8) and grb.shape == (2, 16, 16, 5)
    heads = [k for k in o1 if "+" in k]
    assert heads == ["feature_fusion/Conv_7+Conv_8/weights", "feature_fusion/Conv_7+Conv_8/biases"]
    assert [k for k in o1 if "+" not in k] == [k for k in orb if "+" not in k]
    assert [k for k in orb if "+" in k] == [HEAD + "weights", HEAD + "biases"]


# ------------------------------------------------------------------------------------------------ driver
@pytest.mark.parametrize("precision", ["f16", "f32", "f16x2"])
def test_east_test_script_rbox_end_to_end(device, tmp_path, precision):
    """test.py --geometry RBOX in a fresh child process: network -> per-pixel quads -> LANMS -> res file."""
    from tensorflow_ocr_amd import checkpoint
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    os.makedirs(os.path.join(tmp_path, "in"))
    rng = np.random.default_rng(71)
    np.save(os.path.join(tmp_path, "in", "photo_0.npy"), rng.integers(0, 256, size=(96, 128, 3)).astype(np.uint8))
    g0 = Graph(device, seed=3)
    M.model_rbox(np.zeros((1, 64, 64, 3), f32), is_training=False, graph=g0)
    sd = checkpoint.internal_to_tf(g0.store.state_dict())
    assert sd["feature_fusion/Conv_8/weights"].shape == (1, 1, 32, 4) and sd["feature_fusion/Conv_9/biases"].shape == (1,)
    # random weights under inference-mode BN (moving stats 0 / 1) overflow f16 through 50 layers: switch the trunk off
    # (gamma = 0) and let the biases say "text everywhere, 24 x 12 px boxes at +-0.1 rad"
    for k in sd:
        if k.endswith("BatchNorm/gamma"):
            sd[k] = np.zeros_like(sd[k])
    sd["feature_fusion/Conv_7/biases"] = np.array([3.0], f32)                       # sigmoid 0.95 > 0.8
    sd["feature_fusion/Conv_8/biases"] = np.array([-4.4, -3.7, -4.4, -3.7], f32)    # 512 sigmoid: ~6, ~12 px
    sd["feature_fusion/Conv_9/biases"] = np.array([0.25], f32)
    ck = os.path.join(tmp_path, "ckpt")
    checkpoint.save_tf_checkpoint(ck, 7, sd, {k: v for k, v in sd.items() if "moving_" not in k})
    out_dir = os.path.join(tmp_path, "res")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--geometry", "RBOX", "--precision", precision, "--test_data_path",
                        os.path.join(tmp_path, "in"), "--output_dir", out_dir, "--checkpoint_path", ck],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Find 1 images" in r.stdout and "Restore from" in r.stdout
    lines = open(os.path.join(out_dir, "res_photo_0.txt"), newline="").read().split("\r\n")[:-1]
    assert len(lines) >= 4
    # every pixel predicts the same box shape, so a merged quad (a weighted mean of translates) keeps it: W = 512
    # (sigmoid(-3.7) * 2), H = 512 (sigmoid(-4.4) * 2), turned by (sigmoid(0.25) - 0.5) pi/2 > 0.  Every coordinate is truncated
    # towards zero (moves by less than 1), so each projection of a side moves by less than 2 and its length by < 2 sqrt(2)
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    W, Hh = 1024 * sig(-3.7), 1024 * sig(-4.4)
    for line in lines:
        assert re.fullmatch(r"-?\d+(,-?\d+){7}", line), line
        q = np.array([int(v) for v in line.split(",")], f64).reshape(4, 2)
        assert abs(math.hypot(*(q[1] - q[0])) - W) < 2.83 and abs(math.hypot(*(q[2] - q[1])) - Hh) < 2.83, line
        assert q[1, 1] <= q[0, 1] and q[1, 0] > q[0, 0], line                   # the top side runs right and (y down) upwards
