"""GPU: PixelLink's instance-balanced loss (csrc/pixellink_balance.hip) — the instance weight map from cover rasters
(ocr_pixellink_instance_weights), the loss with weighted mining (ocr_balanced_loss_fwd / _selected / _bwd / _bwd_dyn),
every status code, and the path from `pixellink_fn.generate_rbox_batch(weights=True)` through
`PixelLinkNet.build_loss(pixel_weights=...)` into a recorded TrainStep — against the float64 / NumPy restatement of the
header's definition in tests/balanced_ref.py.  The loss is build-defined (the reference keeps only the remains of it,
nets/pixellink.py:138-168); nothing here is compared with an upstream TensorFlow run.  Entries are called through ctypes
on the library tensorflow_ocr_amd.ops binds; every output sits NaN-filled between guard bands.

Index work is bit-exact: area and weight (integer counts, then one rounding from double), the threshold and the selected
mask (the mining score restated in float32 with O.neg_score_f32, the sequence the kernels share).

Bounds (u = 2^-24; g(m) = m u / (1 - m u); no relative tolerance), in the form of tests/test_gpu_loss_matrix.py, whose
ELOG = 3.064 and EPOW = 2.322 (logf / powf measured on the MI355X, plus one ulp) are taken over:
  A reduction of terms v_i formed within d_i: |dev - ref| <= g(m_sum) sum(|v_i| + d_i) + sum d_i + 2^-149,
      m_sum = ceil(total / (T 256)) [per-thread trips] + 6 [shuffles] + 3 [cross-wave additions] + 1 [f64 -> f32].
  CE term: d_ce = g(2 ELOG + 2) (1 + |log s| + |m| + |l_t|); focal term: the first-order propagation of that file.
  Weighted term v w with the f32 weight w exact: the product adds one u: d = (d_v + u (|v| + d_v)) w.
  Weight sums (sums34[1], [3 + 4d], [5 + 4d]): the terms are exact, only the tree rounds: g(m_sum) sum w.  (They are no
      longer counts, so they are bounded, not bit-compared.)
  loss10: a quotient a / b of sums known within da, db: (da + |q| db) / (b - db) + 2 u |q|; a link term adds u for its
      addition, the total 9 u of the magnitudes for its nine.
  gradients, referred to the sums the device wrote: CE g(13) (|p1| + 1) W |c_pix| (p1 7, subtraction 1, weight product 1,
      coefficient 3, final product 1); links (d_dz1 + g(5) |dz1|) |coef|, d_dz1 = g(8) (q1 + 1) for CE (coefficient:
      division, seed product, weight product; final product).  A cell with W = 0 / outside P must hold exact zeros.
  `_dyn` with scale s: the seed is the f32 product grad_scale * s, so it must equal the plain form seeded with that
      product bit for bit.
  Every row prints `balanced <entry> <row> ratio=<|err| / bound>`.

MEASURED (largest |err| / bound over the rows, f16 library, MI355X; 0.000 = bit-exact index work)
  instance_weights area / weight 0.000      threshold, selected mask       0.000
  balanced_loss_fwd_sums         0.192      balanced_loss_fwd              0.068
  balanced_loss_bwd_pixel        0.160      balanced_loss_bwd_link         0.220
  balanced_loss_bwd_dyn_pixel    0.154      balanced_loss_bwd_dyn_link     0.231
  _dyn against the plain form seeded grad_scale * s: bit-identical.  No row was over its bound.
  Time on the MI355X: the file's 30 tests 2.8 s.
"""
import ctypes
import math
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import balanced_ref as B
import matrix_support
from matrix_support import FL, INVALID_ARG, OK, SZ, UNSUPPORTED, WORKSPACE, Guard, _d32, _lib, _ratio, _rc, _rng, f32, f64

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "balanced")


def _cmp(entry, row, got, ref, bound):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    bound = np.broadcast_to(np.asarray(bound, f64), ref.shape)
    assert got.shape == ref.shape and np.isfinite(got).all(), (entry, row)
    _note(entry, row, _ratio(np.abs(got - ref), bound + 2.0 ** -149))


# ------------------------------------------------------------------------------------------------ weight map
def _quads(rects, P):
    polys = np.zeros((P, 4, 2), np.int32)
    for j, (x0, y0, x1, y1) in enumerate(rects):
        polys[j] = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return polys


GRID254 = [(4 * (k % 16), 4 * (k // 16), 4 * (k % 16) + 3, 4 * (k // 16) + 3) for k in range(254)]
# (row, h, w, new_h, new_w, per image (rects, ignored indices))
WEIGHT_ROWS = [
    ("overlap", 64, 64, 16, 16, [([(4, 4, 40, 30), (20, 16, 59, 50)], [])]),
    ("hidden", 64, 64, 16, 16, [([(4, 4, 30, 30), (44, 50, 50, 58), (42, 48, 56, 60)], [])]),
    ("ignored", 64, 64, 16, 16, [([(4, 4, 30, 30), (34, 8, 60, 28), (8, 40, 50, 60)], [1])]),
    ("sub_cell", 64, 64, 16, 16, [([(4, 4, 30, 30), (8, 40, 9, 41), (41, 41, 43, 43)], [])]),   # owns one cell | none
    ("empty", 64, 64, 16, 16, [([], []), ([(4, 4, 30, 30), (20, 20, 50, 50)], []), ([], [])]),
    ("all_ignored", 64, 64, 16, 16, [([(4, 4, 30, 30)], [0])]),
    ("same_size", 32, 32, 32, 32, [([(1, 1, 9, 12), (5, 6, 30, 20), (25, 25, 25, 25)], [])]),
    ("h_ne_w", 48, 80, 12, 20, [([(2, 2, 40, 20), (30, 10, 79, 47), (50, 30, 60, 40)], [2]), ([(0, 0, 79, 47)], [])]),
    ("grid254", 64, 64, 16, 16, [(GRID254, [7, 253])]),
]


@pytest.mark.parametrize("row", WEIGHT_ROWS, ids=[r[0] for r in WEIGHT_ROWS])
def test_instance_weights(device, row):
    L, ops = _lib()
    name, h, w, nh, nw, images = row
    n = len(images)
    P = max([len(r) for r, _ in images] + [1])
    polys = np.stack([_quads(r, P) for r, _ in images])
    counts = np.array([len(r) for r, _ in images], np.int32)
    ignore = np.zeros((n, P), np.uint8)
    for b, (_, ig) in enumerate(images):
        ignore[b, ig] = 1
    cover = torch.empty((n, h, w), dtype=torch.int32, device=device)
    # the cover is made with a zero ignore table, as generate_rbox_batch makes it: the flags go to the weights only
    ops.poly_cover(torch.from_numpy(polys).to(device), torch.from_numpy(counts).to(device),
                   torch.zeros((n, P), dtype=torch.uint8, device=device), h, w, cover)
    area, weight = Guard((n, P), torch.int32, device), Guard((n, nh, nw), torch.float32, device)
    ig = torch.from_numpy(ignore).to(device)
    assert _rc(L, "ocr_pixellink_instance_weights", cover, ig, n, P, h, w, nh, nw, area, weight) == OK
    torch.cuda.synchronize()
    cv = cover.cpu().numpy()
    ra, rw, live = B.instance_weights(cv, ignore, nh, nw)
    assert np.array_equal(area.raw(), ra), (area.raw(), ra)
    got = weight.np()
    assert np.array_equal(got.view(np.int32), rw.view(np.int32)), "%d weights differ" % int((got != rw).sum())
    # the weights line up with ocr_pixellink_labels' score map: text cells are the owned cells
    score = torch.empty((n, nh, nw), dtype=torch.float32, device=device)
    link = torch.empty((n, nh, nw, 8), dtype=torch.float32, device=device)
    ops.pixellink_labels(cover, nh, nw, score, link)
    own = B.owner_map(cv, nh, nw, P)
    assert np.array_equal(score.cpu().numpy() > 0, own > 0) and not (got[own == 0] != 0).any()
    for b in range(n):
        S = int(ra[b][live[b]].sum())
        assert abs(got[b].astype(f64).sum() - S) <= 2.0 ** -24 * S
    if name == "overlap":
        assert live[0].all() and (cv[0, 20, 24] & 255, (cv[0, 20, 24] >> 8) & 255) == (1, 2)     # the later one on top
    if name == "hidden":
        assert ra[0, 1] == 0 and live[0].tolist() == [True, False, True]
        assert got[0, 1, 1] == f32(f64(ra[0, 0] + ra[0, 2]) / (2.0 * f64(ra[0, 0])))             # N = 2, not 3
    if name == "ignored":
        assert ra[0, 1] > 0 and not live[0, 1] and (got[0][own[0] == 2] == 0).all()
    if name == "sub_cell":
        assert ra[0].tolist()[1:] == [1, 0] and got[0, 10, 2] == f32(f64(ra[0, 0] + 1) / 2.0)
    if name == "empty":
        assert (got[0] == 0).all() and (got[2] == 0).all() and (got[1] != 0).any() and (ra[0] == 0).all()
    if name == "all_ignored":
        assert ra[0, 0] > 0 and (got == 0).all()
    if name == "grid254":
        assert (ra[0] == 1).all() and own.max() == 254 and got[0, 15, 13] == 0 and got[0, 0, 0] == 1


def test_instance_weights_status_codes(device):
    L, _ = _lib()
    n, P, h, w, nh, nw = 1, 2, 16, 16, 4, 4
    cover = torch.zeros((n, h, w), dtype=torch.int32, device=device)
    ig = torch.zeros((n, P), dtype=torch.uint8, device=device)
    area, weight = Guard((n, P), torch.int32, device), Guard((n, nh, nw), torch.float32, device)
    good = [cover, ig, n, P, h, w, nh, nw, area, weight]
    for k in (0, 1, 8, 9):
        a = list(good)
        a[k] = None
        assert _rc(L, "ocr_pixellink_instance_weights", *a) == INVALID_ARG, k
    for k, v in ((2, 0), (2, 65536), (3, 0), (3, 255), (4, 0), (4, 16385), (5, 0), (5, 16385), (6, 0), (7, 0), (6, -1)):
        a = list(good)
        a[k] = v
        assert _rc(L, "ocr_pixellink_instance_weights", *a) == UNSUPPORTED, (k, v)
    torch.cuda.synchronize()
    assert area.untouched() and weight.untouched()
    assert _rc(L, "ocr_pixellink_instance_weights", *good) == OK
    torch.cuda.synchronize()
    assert (area.raw() == 0).all() and (weight.np() == 0).all()


# ------------------------------------------------------------------------------------------------ the loss
def _case(n, hw, focal, key=0, neg_ratio=3.0, alpha=0.25, gamma=2.0):
    rng = _rng("balanced", n, hw, key)
    c = NS(n=n, hw=hw, focal=focal, neg_ratio=neg_ratio, alpha=alpha, gamma=gamma)
    c.pl = (2 * rng.standard_normal((n, hw, 2))).astype(f32)
    c.ll = (2 * rng.standard_normal((n, hw, 16))).astype(f32)
    vals = np.array([1, 0, 0.5, -1, 2], f32)
    c.plab = rng.choice(vals, (n, hw), p=[0.1, 0.8, 0.03, 0.04, 0.03])       # ~ 14 % weighted text: k is about half of n_neg
    c.llab = rng.choice(vals, (n, hw, 8), p=[0.4, 0.45, 0.05, 0.05, 0.05])
    # text cells weigh like instances of 1 / 8 to 8 times the mean area; 15 % of them are ignored text (weight 0)
    wv = np.where(rng.random((n, hw)) < 0.15, 0.0, 2.0 ** rng.uniform(-3, 3, (n, hw)))
    c.w = np.where(c.plab > 0, wv, 0.0).astype(f32)
    c.row = "n%d_hw%d_f%d" % (n, hw, focal)
    return c


def _desc(L, c, **over):
    v = dict(n=c.n, hw=c.hw, focal=c.focal, neg_ratio=c.neg_ratio, alpha=c.alpha, gamma=c.gamma)
    v.update(over)
    return L.BalancedLossDesc(v["n"], v["hw"], v["focal"], float(v["neg_ratio"]), float(v["alpha"]), float(v["gamma"]))


def _run(device, c):
    """fwd, selected, bwd and bwd_dyn on one case, everything checked against balanced_ref"""
    L, _ = _lib()
    d = _desc(L, c)
    dr = ctypes.byref(d)
    total = c.n * c.hw
    nb = int(L._fn("ocr_balanced_loss_workspace", SZ)(dr))
    assert nb == B.blocks(total) * 34 * 4
    pl, ll, plab, llab, w = (_d32(a, device) for a in (c.pl, c.ll, c.plab, c.llab, c.w))
    thr, sums, loss, ws = (Guard(s, torch.float32, device) for s in ((c.n,), (34,), (10,), (nb // 4,)))
    assert _rc(L, "ocr_balanced_loss_fwd", dr, pl, ll, plab, llab, w, thr, sums, loss, ws, SZ(nb)) == OK
    mask = Guard((c.n, c.hw), torch.uint8, device)
    assert _rc(L, "ocr_balanced_loss_selected", dr, pl, plab, w, thr, mask) == OK
    torch.cuda.synchronize()
    r = B.loss_ref(c)
    out = NS(r=r, thr=thr.np(), sums=sums.np(), loss=loss.np(), mask=mask.raw())
    assert ws.ok()
    assert np.array_equal(out.thr.view(np.int32), r.thr.view(np.int32)), (out.thr, r.thr)
    assert np.array_equal(out.mask, (r.W != 0).astype(np.uint8)), "mask: %d cells differ" % int((out.mask != (r.W != 0)).sum())
    _cmp("balanced_loss_fwd_sums", c.row, out.sums, r.sums, r.sums_bound)
    _cmp("balanced_loss_fwd", c.row, out.loss, r.loss, r.loss_bound)
    scale = _d32(np.array([3.0], f32), device)
    runs = {}
    for name, gs, extra in (("ocr_balanced_loss_bwd", f32(1.7), ()), ("ocr_balanced_loss_bwd_dyn", f32(0.85), (scale,)),
                            ("ocr_balanced_loss_bwd", f32(0.85) * f32(3.0), ())):
        dpl, dll = Guard((c.n, c.hw, 2), torch.float32, device), Guard((c.n, c.hw, 16), torch.float32, device)
        assert _rc(L, name, dr, pl, ll, plab, llab, w, thr, sums, FL(gs), *extra, dpl, dll) == OK
        torch.cuda.synchronize()
        gp, gl = dpl.np(), dll.np()                      # every element written
        seed = f64(gs * f32(3.0)) if extra else f64(gs)
        rp, bp, rl, bl = B.grad_ref(c, r, out.sums, seed)
        entry = name[4:] + ("_seeded" if gs == f32(0.85) * f32(3.0) else "")
        _cmp(entry + "_pixel", c.row, gp, rp, bp)
        _cmp(entry + "_link", c.row, gl, rl, bl)
        assert (gp[r.W == 0] == 0).all(), "a pixel gradient on a cell of weight 0 (ignored text among them)"
        assert (gl[~r.P] == 0).all(), "a link gradient outside P"
        runs[entry] = (gp, gl)
    for a, b in zip(runs["balanced_loss_bwd_dyn"], runs["balanced_loss_bwd_seeded"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "_dyn differs from the plain form seeded grad_scale * s"
    out.dpl, out.dll = runs["balanced_loss_bwd"]
    for t, a in ((pl, c.pl), (ll, c.ll), (plab, c.plab), (llab, c.llab), (w, c.w)):
        assert np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32)), "an input was written"
    return out


@pytest.mark.parametrize("focal", [0, 1])
@pytest.mark.parametrize("hw", [64, 256, 1000])
@pytest.mark.parametrize("n", [1, 3])
def test_balanced_loss(device, n, hw, focal):
    """hw = 1000 at n = 1: one block, four trips per thread and a ragged last one; n = 3: three blocks"""
    assert B.blocks(1000) == 1 and B.m_sum(1000) == 4 + 10 and B.blocks(3000) == 3
    c = _case(n, hw, focal)
    out = _run(device, c)
    ignored = (c.plab > 0) & (c.w == 0)
    assert ignored.any() and not out.mask[ignored].any()           # ignored text is in neither set
    assert out.r.mined.any() and (out.loss[0] > 0)


def test_image_without_positives_and_image_of_ignored_text(device):
    c = _case(3, 256, 0, key=1)
    c.plab[0] = np.where(c.plab[0] > 0, 0, c.plab[0])              # no text at all
    c.w[0] = 0
    c.w[1] = 0                                                     # text, all of it ignored
    c.row = "no_pos"
    out = _run(device, c)
    assert out.thr[0] == -1 and out.thr[1] == -1 and out.thr[2] >= 0
    assert not out.mask[:2].any() and (out.dpl[:2] == 0).all() and (out.dll[:2] == 0).all()
    # and a batch with nothing to train on at all: every sum, loss and gradient is an exact zero
    c.w[2] = 0
    c.row = "nothing"
    out = _run(device, c)
    assert (out.sums == 0).all() and (out.loss == 0).all() and (out.dpl == 0).all() and (out.dll == 0).all()


@pytest.mark.parametrize("focal", [0, 1])
def test_direction_without_positive_or_negative_links(device, focal):
    c = _case(2, 256, focal, key=2)
    c.llab[..., 3] = 0
    c.llab[..., 5] = 1
    c.row = "zero_guard_f%d" % focal
    out = _run(device, c)
    assert out.sums[2 + 4 * 3] == 0 and out.sums[3 + 4 * 3] == 0 and out.sums[4 + 4 * 5] == 0 and out.sums[5 + 4 * 5] == 0
    assert np.isfinite(out.loss).all() and out.loss[2 + 3] > 0 and out.loss[2 + 5] > 0


def _mining_image(rng, hw, n_pos, d_neg):
    """n_pos weighted text cells, the rest negatives whose logit difference l1 - l0 comes from d_neg; shuffled"""
    y = np.zeros(hw, f32)
    y[:n_pos] = 1
    w = np.where(y > 0, f32(1.5), f32(0))
    l = np.zeros((hw, 2), f32)
    l[:, 0] = (rng.integers(-8, 9, hw) / 4).astype(f32)
    l[:, 1] = l[:, 0] + np.concatenate([rng.standard_normal(n_pos).astype(f32), np.asarray(d_neg, f32)])
    perm = rng.permutation(hw)
    return y[perm], w[perm], l[perm]


def test_directed_mining(device):
    hw = 64
    rng = _rng("balanced", "mining")
    c = _case(3, hw, 0, key=3)
    # image 0: 5 positives, k = 15, negatives in three groups of equal score (10 | 20 | 29, hardest first): the 15th
    #          lies inside the second group, which is mined whole
    # image 1: 30 positives, 34 negatives, k = min(90, 34) = n_neg: every negative is mined
    # image 2: all different scores, mined exactly k
    specs = [(5, np.repeat([2.0, 0.5, -1.0], [10, 20, 29])), (30, rng.standard_normal(34)), (7, np.arange(57) / 8.0)]
    for i, (n_pos, d) in enumerate(specs):
        c.plab[i], c.w[i], c.pl[i] = _mining_image(rng, hw, n_pos, d)
    c.row = "ties_kmax"
    out = _run(device, c)
    mined = out.mask.astype(bool) & ~(c.w > 0)
    assert out.r.ks == [15, 34, 21] and mined.sum(1).tolist() == [30, 34, 21]      # tie-inclusive: both groups whole
    # (n_pos, ratio) = (10, 0.7f): the product in double is 6.9999998, 6 negatives — 10 * 0.7f in f32 rounds up to 7
    c = _case(1, hw, 0, key=4, neg_ratio=0.7)
    c.plab[0], c.w[0], c.pl[0] = _mining_image(rng, hw, 10, np.arange(54) / 8.0)
    c.row = "ratio0.7"
    assert f32(10) * f32(0.7) == f32(7)
    out = _run(device, c)
    assert out.r.ks == [6] and int((out.mask.astype(bool) & ~(c.w > 0)).sum()) == 6
    # ratio 0: k = 0, nothing is mined, the positives still count
    c.neg_ratio, c.row = 0.0, "ratio0"
    out = _run(device, c)
    assert out.thr[0] == -1 and int(out.mask.sum()) == 10


def test_mining_agrees_with_the_reference_rule_loss(device):
    """with w = [label > 0] the threshold and the selected mask are those of ocr_softmax_loss_fwd / _selected at
    pixel_rule 0, label_rule 1, bit for bit: one radix select, one score"""
    L, _ = _lib()
    for n, hw in ((3, 1000), (2, 64)):
        c = _case(n, hw, 0, key=5)
        c.w = (c.plab > 0).astype(f32)
        pl, ll, plab, llab, w = (_d32(a, device) for a in (c.pl, c.ll, c.plab, c.llab, c.w))
        res = []
        for kind in ("balanced", "softmax"):
            d = _desc(L, c) if kind == "balanced" else L.SoftmaxLossDesc(n, hw, 0, 1, 1, 0, 3.0, 0.25, 2.0)
            dr = ctypes.byref(d)
            nb = int(L._fn("ocr_%s_loss_workspace" % kind, SZ)(dr))
            thr, sums, loss, ws = (Guard(s, torch.float32, device) for s in ((n,), (34,), (10,), (nb // 4,)))
            mask = Guard((n, hw), torch.uint8, device)
            wt = (w,) if kind == "balanced" else ()
            assert _rc(L, "ocr_%s_loss_fwd" % kind, dr, pl, ll, plab, llab, *wt, thr, sums, loss, ws, SZ(nb)) == OK
            assert _rc(L, "ocr_%s_loss_selected" % kind, dr, pl, plab, *wt, thr, mask) == OK
            torch.cuda.synchronize()
            res.append((thr.np(), mask.raw(), sums.np()))
        (ta, ma, sa), (tb, mb, sb) = res
        assert np.array_equal(ta.view(np.int32), tb.view(np.int32)) and np.array_equal(ma, mb) and ma.any()
        assert sa[0] == sb[0]                     # the same CE over the same cells in the same order


def test_loss_status_codes(device):
    L, _ = _lib()
    c = _case(2, 64, 0, key=6)
    d = _desc(L, c)
    dr = ctypes.byref(d)
    nb = int(L._fn("ocr_balanced_loss_workspace", SZ)(dr))
    pl, ll, plab, llab, w = (_d32(a, device) for a in (c.pl, c.ll, c.plab, c.llab, c.w))
    thr, sums, loss, ws = (Guard(s, torch.float32, device) for s in ((c.n,), (34,), (10,), (nb // 4,)))
    mask = Guard((c.n, c.hw), torch.uint8, device)
    dpl, dll = Guard((c.n, c.hw, 2), torch.float32, device), Guard((c.n, c.hw, 16), torch.float32, device)
    scale = _d32(np.array([2.0], f32), device)
    outs = (thr, sums, loss, ws, mask, dpl, dll)

    def calls(dref):
        return {"fwd": ["ocr_balanced_loss_fwd", dref, pl, ll, plab, llab, w, thr, sums, loss, ws, SZ(nb)],
                "selected": ["ocr_balanced_loss_selected", dref, pl, plab, w, thr, mask],
                "bwd": ["ocr_balanced_loss_bwd", dref, pl, ll, plab, llab, w, thr, sums, FL(1.0), dpl, dll],
                "bwd_dyn": ["ocr_balanced_loss_bwd_dyn", dref, pl, ll, plab, llab, w, thr, sums, FL(1.0), scale, dpl, dll]}

    query = L._fn("ocr_balanced_loss_workspace", SZ)
    assert query(None) == 0
    bad = [(dict(n=0), INVALID_ARG), (dict(n=-1), INVALID_ARG), (dict(hw=0), INVALID_ARG), (dict(focal=2), INVALID_ARG),
           (dict(focal=-1), INVALID_ARG), (dict(neg_ratio=-0.5), INVALID_ARG), (dict(neg_ratio=float("nan")), INVALID_ARG),
           (dict(n=2, hw=2 ** 30), UNSUPPORTED)]
    for over, want in bad:
        db = _desc(L, c, **over)
        if "n" in over and over["n"] <= 0 or over.get("hw") == 0:
            assert query(ctypes.byref(db)) == 0
        for key, a in calls(ctypes.byref(db)).items():
            assert _rc(L, *a) == want, (over, key)
    assert _rc(L, *calls(None)["fwd"]) == INVALID_ARG and _rc(L, *calls(None)["bwd"]) == INVALID_ARG
    for key, a in calls(dr).items():                       # every pointer NULL in turn
        for k in range(2, len(a)):
            if isinstance(a[k], (torch.Tensor, Guard)):
                b = list(a)
                b[k] = None
                assert _rc(L, *b) == INVALID_ARG, (key, k)
    short = calls(dr)["fwd"]
    short[-1] = SZ(nb - 1)
    assert _rc(L, *short) == WORKSPACE
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused call wrote"
    for key in ("fwd", "selected", "bwd", "bwd_dyn"):
        assert _rc(L, *calls(dr)[key]) == OK, key
    torch.cuda.synchronize()
    assert all(o.ok() for o in outs)


# ------------------------------------------------------------------------------------------------ end to end
def _boxes():
    """two images of normalised quads: xs, ys [k, 4], bboxes, ignored"""
    out = []
    for rects, ign in (([(0.1, 0.1, 0.6, 0.4), (0.3, 0.5, 0.9, 0.8), (0.05, 0.7, 0.25, 0.95)], [0, 0, 1]),
                       ([(0.2, 0.2, 0.8, 0.6)], [0])):
        r = np.array(rects, f32)
        xs = np.stack([r[:, 0], r[:, 2], r[:, 2], r[:, 0]], 1)
        ys = np.stack([r[:, 1], r[:, 1], r[:, 3], r[:, 3]], 1)
        out.append((xs, ys, np.stack([r[:, 1], r[:, 0], r[:, 3], r[:, 2]], 1), np.array(ign, np.int32)))
    return [list(v) for v in zip(*out)]


def test_generate_rbox_batch_weights(device):
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import pixellink_fn
    g = Graph(device)
    xs, ys, bb, ig = _boxes()
    s0, l0, sb0 = pixellink_fn.generate_rbox_batch(64, 64, xs, ys, bb, ig, graph=g)
    s1, l1, sb1, wt = pixellink_fn.generate_rbox_batch(64, 64, xs, ys, bb, ig, graph=g, weights=True)
    assert torch.equal(s0, s1) and torch.equal(l0, l1) and np.array_equal(sb0, sb1)      # the flags reach the weights only
    assert wt.shape == (2, 16, 16) and wt.dtype == torch.float32
    s, wv = s1.cpu().numpy(), wt.cpu().numpy()
    assert not (wv[s == 0] != 0).any() and (wv >= 0).all()
    assert s[0, 13, 2] == 1 and wv[0, 13, 2] == 0                  # inside the ignored quad: text in the score map, weight 0
    live0 = wv[0] > 0
    assert abs(wv[0].astype(f64).sum() - live0.sum()) <= 2.0 ** -24 * live0.sum() and len(np.unique(wv[0][live0])) == 2
    assert (wv[1][s[1] > 0] == 1).all()                            # one instance: S / (1 * S)


def test_train_step_with_pixel_weights(device):
    """PixelLinkNet at 64 x 64, batch 2, `build_loss(pixel_weights=...)` inside a TrainStep: two eager steps, the
    recorded one and a replay"""
    from tensorflow_ocr_amd import losses
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.tool import pixellink_fn
    from tensorflow_ocr_amd.train import MomentumOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=1)
    xs, ys, bb, ig = _boxes()
    score, link, _, wt = pixellink_fn.generate_rbox_batch(64, 64, xs, ys, bb, ig, graph=g, weights=True)
    images = torch.from_numpy(np.random.default_rng(4).uniform(0, 255, (2, 64, 64, 3)).astype(f32)).to(device)
    nets = []

    def forward_loss(gr, im, pixel_labels, link_labels, pixel_weights):
        net = pixellink.PixelLinkNet(im, graph=gr, input_norm=(120.0, 60.0))
        nets.append(net)
        return net.build_loss(pixel_labels, link_labels, pixel_weights=pixel_weights, neg_ratio=3.0)

    step = TrainStep(g, forward_loss, lambda gr: MomentumOptimizer(gr, base_lr=0.01, momentum=0.9, weight_decay=5e-4))
    first = step(images, score, link, wt).data.clone()
    px, lk = nets[-1].pixel_cls.data.clone(), nets[-1].link_cls.data.clone()
    assert len(g.collections["losses"]) == 2                       # the two reference entries (train_pixellink.py:263)
    g2 = Graph(device)
    alone = losses.balanced_loss(g2, NS(data=px, grad=None), NS(data=lk, grad=None), score, link, wt, neg_ratio=3.0)
    assert torch.equal(alone.data, first), (alone.data, first)
    assert int(alone.selected_mask().sum()) > int((wt > 0).sum())  # negatives were mined on top of the weighted cells
    mean = losses.softmax_loss(g2, NS(data=px, grad=None), NS(data=lk, grad=None), score, link, pixel_rule=2, label_rule=1,
                               link_gate=False)
    assert float(mean.data[0]) != float(first[0])                  # not the default path
    vals = [float(first[0])]
    for _ in range(3):
        vals.append(step(images, score, link, wt).item())
    assert step.plan is not None                                   # step 3 was recorded, step 4 replayed it
    assert all(math.isfinite(v) for v in vals) and vals[1] != vals[0] and vals[3] != vals[2]
    assert any("ocr_balanced_loss_fwd" == e[3] for e in step.plan if e[0] == "c")
    assert any("ocr_balanced_loss_bwd" == e[3] for e in step.plan if e[0] == "c")
