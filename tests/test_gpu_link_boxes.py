"""GPU: the two link-geometry entries of csrc/link_boxes.hip against the NumPy restatements of
tests/test_link_eval_host.py, bit for bit — ocr_component_scores (exact integer sums: scheduling cannot show) on a map
whose runs cross wave and workgroup edges, ocr_link_boxes on what ocr_min_area_rects produces for rotated rectangles,
lines, two- and one-point components, with and without the size filters — and their status codes."""
import ctypes

import numpy as np
import pytest
import torch

import test_link_eval_host as H

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
SENT_I, SENT_F = -123456, f32(-12345.5)


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


# ------------------------------------------------------------------------------------------------ scores
N, HH, WW, MAX_COMPS = 3, 20, 300, 8


def _score_case():
    rng = np.random.default_rng(314)
    lab = np.zeros((N, HH, WW), i32)
    a = lab[0]
    a[0, :] = 1                                  # a full-width row: 300 pixels, four wave edges and a workgroup edge
    a[2, 5] = 2                                  # one pixel
    a.reshape(-1)[703:705] = 3                   # two pixels on either side of a wave edge (704 = 11 * 64)
    a[4:10, 10:201] = 4                          # a block: six runs of 191
    a[4:10, 201:300] = 5                         # touching it: the label changes inside a wave
    a[10, 60:91] = 6                             # a run across a workgroup edge (3072 = 12 * 256 is row 10, column 72)
    a[12, 0:130:2] = 7                           # interleaved pixel by pixel: 130 one-pixel runs
    a[12, 1:130:2] = 8
    a[14, 0:51] = 9                              # two ids beyond max_comps: ignored
    a[15, 100:121] = 10
    a[17, 3], a[17, 4] = -3, 1000                # labels outside 1..max_comps: ignored
    lab[2] = 1                                   # one component of all 6000 pixels
    ncomp = np.array([10, 0, 1], i32)
    score = rng.uniform(0, 1, (N, HH, WW)).astype(f32)
    special = np.array([0.0, 1.0, np.nan, -0.5, 1.5, 0.125, f32(0.125) + f32(2.0 ** -26), f32(0.125) + f32(2.0 ** -25),
                        np.nextafter(f32(0.5), f32(1)), 0.5, np.inf, -np.inf, f32(2.0 ** -25), f32(1e-30)], f32)
    flat = score[0].reshape(-1)
    where = rng.choice(flat.size, 600, replace=False)
    flat[where] = special[np.arange(600) % len(special)]
    score[0, 2, 5] = np.nan                      # the one-pixel component scores NaN -> 0
    score[0].reshape(-1)[703:705] = [0.125, f32(0.125) + f32(2.0 ** -26)]
    score[2] = 1.0                               # 6000 * 2^24 does not fit 32 bits
    return lab, ncomp, score


def test_component_scores_equal_the_integer_restatement(device, graph):
    from tensorflow_ocr_amd import ops
    lab, ncomp, score = _score_case()
    assert len(set(np.unique(lab[0])) & set(range(1, 11))) == 10
    want = H.component_scores_ref(lab, score, ncomp, MAX_COMPS)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    l_d, s_d, n_d = up(lab), up(score), up(ncomp)
    runs = []
    for _ in range(2):
        out = torch.full((N + 1, MAX_COMPS), float(SENT_F), dtype=torch.float32, device=device)
        ops.component_scores(l_d, s_d, n_d, out[:N], graph.workspace())
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    got = runs[0]
    print("component scores, image 0: %s" % got[0].tolist())
    assert np.array_equal(got[:N].view(i32), want.view(i32))                # bit for bit
    assert (got[N] == SENT_F).all()                                         # nothing beyond [n]
    assert np.array_equal(runs[0].view(i32), runs[1].view(i32))             # two runs, the same bits
    assert got[0, 1] == 0.0 and got[0, 2] == f32(0.125)                     # NaN -> 0; below the quantum -> the same integer
    assert (got[1] == 0).all() and got[2].tolist() == [1.0] + [0.0] * 7     # no component; rows beyond ncomp are 0
    assert 0 < got[0, 3] < 1 and got[0, 3] != got[0, 4]


def test_component_scores_status_codes_leave_the_output_alone(device, graph):
    from tensorflow_ocr_amd import _lib as L
    lab, ncomp, score = _score_case()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    l_d, s_d, n_d = up(lab), up(score), up(ncomp)
    out = torch.full((N, MAX_COMPS), float(SENT_F), dtype=torch.float32, device=device)
    nbytes = L.call_size("ocr_component_scores_workspace", ctypes.c_int(N), ctypes.c_int(MAX_COMPS))
    assert nbytes == N * MAX_COMPS * 16
    ws = graph.workspace().get(nbytes)
    fn, p = L._fn("ocr_component_scores", ctypes.c_int), L.ptr

    def call(lab=l_d, ps=s_d, nc=n_d, n=N, h=HH, w=WW, mc=MAX_COMPS, out=out, ws=ws, wsb=nbytes):
        return fn(p(lab), p(ps), p(nc), n, h, w, mc, p(out), p(ws), ctypes.c_size_t(wsb), L.stream_ptr())
    for kw in (dict(lab=None), dict(ps=None), dict(nc=None), dict(out=None), dict(ws=None), dict(n=0), dict(h=0), dict(w=0),
               dict(mc=0), dict(n=-1)):
        assert call(**kw) == -1, kw
    assert call(n=65536) == -2 and call(mc=65536) == -2 and call(h=32769) == -2 and call(w=32769) == -2
    assert call(wsb=nbytes - 1) == -4
    torch.cuda.synchronize()
    assert (out == float(SENT_F)).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out[2].tolist() == [1.0] + [0.0] * 7


# ------------------------------------------------------------------------------------------------ boxes
BH = BW = 48
BOX_COMPS = 10


def _box_label_maps():
    """image 0: ten ids inside max_comps — rotated rectangles at 0, 45, 88 and 20 degrees, a horizontal, a vertical and a
    diagonal line, a two-point and a one-point component, an id without pixels — and two more beyond it; image 1: none."""
    lab = np.zeros((2, BH, BW), i32)
    ys, xs = np.mgrid[0:BH, 0:BW]

    def rot(cx, cy, a, b, deg):
        th = np.deg2rad(deg)
        u = (xs - cx) * np.cos(th) + (ys - cy) * np.sin(th)
        v = -(xs - cx) * np.sin(th) + (ys - cy) * np.cos(th)
        return (np.abs(u) <= a) & (np.abs(v) <= b)
    masks = [rot(8, 6, 6, 2, 0), rot(24, 7, 6, 2, 45), rot(40, 8, 6, 2, 88), rot(8, 20, 6, 2, 20),
             (ys == 18) & (xs >= 18) & (xs <= 30),                          # horizontal line
             (xs == 40) & (ys >= 18) & (ys <= 28),                          # vertical line
             (xs - 4 == ys - 30) & (xs >= 4) & (xs <= 12),                  # diagonal line
             (ys == 34) & ((xs == 20) | (xs == 21)),                        # two points
             (ys == 36) & (xs == 30),                                       # one point
             np.zeros((BH, BW), bool),                                      # id 10: no pixels
             rot(40, 40, 4, 2, 0), rot(24, 44, 4, 1, 0)]                    # ids 11, 12: beyond max_comps
    for k, m in enumerate(masks):
        assert not (m & (lab[0] != 0)).any(), k
        lab[0][m] = k + 1
    return lab, np.array([12, 0], i32)


@pytest.fixture(scope="module")
def rects(device, graph):
    """scale -> (hull_n, hull_head, calipers) of ocr_min_area_rects on the label maps: device tensors and host copies"""
    from tensorflow_ocr_amd import ops
    lab, ncomp = _box_label_maps()
    out = {}
    for scale in ((4.0, 4.0), (1280.0 / 320, 720.0 / 192)):
        hn = torch.zeros((2, BOX_COMPS), dtype=torch.int32, device=device)
        hd = torch.zeros((2, BOX_COMPS, 4), dtype=torch.int32, device=device)
        cal = torch.zeros((2, BOX_COMPS, 6), dtype=torch.float32, device=device)
        ops.min_area_rects(torch.from_numpy(lab).to(device), torch.from_numpy(ncomp).to(device), BOX_COMPS, scale[0], scale[1],
                           hn, hd, cal, graph.workspace())
        torch.cuda.synchronize()
        out[scale] = (hn, hd, cal, hn.cpu().numpy(), hd.cpu().numpy(), cal.cpu().numpy())
    return ncomp, out


@pytest.mark.parametrize("min_side,min_area", [(0.0, 0.0), (12.0, 0.0), (0.0, 700.0)])
@pytest.mark.parametrize("scale", [(4.0, 4.0), (1280.0 / 320, 720.0 / 192)])
def test_link_boxes_equal_the_host_formatting(device, rects, scale, min_side, min_area):
    from tensorflow_ocr_amd import ops
    ncomp, by_scale = rects
    hn, hd, cal, hn_h, hd_h, cal_h = by_scale[scale]
    n = 2
    kinds = hn_h[0]
    assert (kinds[:4] > 2).all() and kinds[7] == 2 and kinds[8] == 1 and kinds[9] == 0, kinds     # the shapes are what they are named
    comp_score = np.random.default_rng(5).uniform(0, 1, (n, BOX_COMPS)).astype(f32)
    want = H.link_boxes_ref(hn_h, hd_h, cal_h, comp_score, ncomp, min_side, min_area)
    merged = torch.full((n + 1, BOX_COMPS, 9), float(SENT_F), dtype=torch.float32, device=device)
    keep = torch.full((n + 1, BOX_COMPS), SENT_I, dtype=torch.int32, device=device)
    n_keep = torch.full((n + 1,), SENT_I, dtype=torch.int32, device=device)
    passed = torch.full((n + 1, BOX_COMPS), 77, dtype=torch.uint8, device=device)
    total = torch.full((n + 1,), SENT_I, dtype=torch.int32, device=device)
    ops.link_boxes(hn, hd, cal, torch.from_numpy(comp_score).to(device), torch.from_numpy(ncomp).to(device), min_side, min_area,
                   merged[:n], keep[:n], n_keep[:n], passed[:n], total[:n])
    torch.cuda.synchronize()
    m, k, nk, p, t = (x.cpu().numpy() for x in (merged, keep, n_keep, passed, total))
    print("scale %s filters (%g, %g): boxes %s passed %s" % (scale, min_side, min_area,
                                                             m[0, :, :8].astype(int).tolist(), p[0].tolist()))
    bad = [c for c in range(BOX_COMPS) if not np.array_equal(m[0, c, :8], want[0][0, c, :8])]
    assert not bad, (bad, m[0, bad, :8].tolist(), want[0][0, bad, :8].tolist())
    assert np.array_equal(m[:n, :, 8].view(i32), want[0][:, :, 8].view(i32))       # the scores: copied bits
    assert (m[:n, :, :8] == np.trunc(m[:n, :, :8])).all()                          # integers, stored as f32
    assert np.array_equal(k[:n], want[1]) and (k[0] == np.arange(BOX_COMPS)).all()  # the identity
    assert nk[:n].tolist() == [BOX_COMPS, 0] and t[:n].tolist() == [12, 0]         # min(ncomp, max_comps); ncomp itself
    assert np.array_equal(p[:n], want[3])
    assert (m[1] == 0).all() and (p[1] == 0).all()                                 # rows at or beyond n_keep: zeros, not passed
    assert (m[n] == SENT_F).all() and (k[n] == SENT_I).all() and nk[n] == SENT_I and (p[n] == 77).all() and t[n] == SENT_I
    n_pass = int(p[0].sum())
    if min_side == 0.0 and min_area == 0.0:
        assert n_pass == BOX_COMPS - 1                                      # only the id without pixels fails
    else:
        # the 0-degree rectangle covers x 2..14, y 4..8: 48 x 16 (scale 4) or 48 x 15 (scale 3.75) pixels passes both
        # filters; lines and points have no second side (the diagonal's is a pixel or two at the uneven scale)
        assert p[0, 0] == 1 and not p[0, 4:].any() and n_pass <= 4


def test_link_boxes_status_codes_leave_the_outputs_alone(device, rects):
    from tensorflow_ocr_amd import _lib as L
    ncomp, by_scale = rects
    hn, hd, cal = by_scale[(4.0, 4.0)][:3]
    n = 2
    sc = torch.zeros((n, BOX_COMPS), dtype=torch.float32, device=device)
    nc = torch.from_numpy(ncomp).to(device)
    merged = torch.full((n, BOX_COMPS, 9), float(SENT_F), dtype=torch.float32, device=device)
    ints = torch.full((3, n, BOX_COMPS), SENT_I, dtype=torch.int32, device=device)
    passed = torch.full((n, BOX_COMPS), 77, dtype=torch.uint8, device=device)
    fn, p = L._fn("ocr_link_boxes", ctypes.c_int), L.ptr
    F = ctypes.c_float

    def call(hn=hn, hd=hd, cal=cal, sc=sc, nc=nc, n=n, mc=BOX_COMPS, m=merged, k=ints[0], nk=ints[1], ps=passed, t=ints[2]):
        return fn(p(hn), p(hd), p(cal), p(sc), p(nc), n, mc, F(0), F(0), p(m), p(k), p(nk), p(ps), p(t), L.stream_ptr())
    for kw in (dict(hn=None), dict(hd=None), dict(cal=None), dict(sc=None), dict(nc=None), dict(m=None), dict(k=None),
               dict(nk=None), dict(ps=None), dict(t=None), dict(n=0), dict(mc=0), dict(mc=-1)):
        assert call(**kw) == -1, kw
    assert call(n=65536) == -2 and call(mc=65536) == -2
    torch.cuda.synchronize()
    assert (merged == float(SENT_F)).all() and (ints == SENT_I).all() and (passed == 77).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert ints[1].reshape(-1)[:2].tolist() == [BOX_COMPS, 0] and ints[2].reshape(-1)[:2].tolist() == [12, 0]
    assert ints[0, 0].tolist() == list(range(BOX_COMPS))
