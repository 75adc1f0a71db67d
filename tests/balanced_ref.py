"""float64 / NumPy restatement of PixelLink's instance-balanced loss as include/ocr_hip.h defines it
(ocr_pixellink_instance_weights, ocr_balanced_loss_*): the weight map from a cover raster, the mining (index work, in
float32 with O.neg_score_f32, the sequence the kernels share), sums34, loss10 and the gradients, each with the bound its
f32 evaluation on the device is held to.  A plain module: no fixtures, no device code.  The derivation of the bounds is in
the docstring of tests/test_gpu_balanced_loss.py."""
from types import SimpleNamespace as NS

import numpy as np

from oracle import ocr_oracle as O

f32, f64 = np.float32, np.float64
U32 = 2.0 ** -24
ELOG = 3.064        # ulps of logf on [1, 2] plus one, EPOW of powf plus one: measured for tests/test_gpu_loss_matrix.py
EPOW = 2.322
M_GRAD = 13


def _g(m):
    m = np.asarray(m, f64)
    return m * U32 / (1.0 - m * U32)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ weight map
def paint_cover(h, w, rects, ignore=()):
    """The cover words ocr_poly_cover gives for axis-aligned rectangles (x0, y0, x1, y1), corners inclusive, drawn in
    order: bits 0-7 smallest covering index + 1, bits 8-15 the largest, bit 16 covered by an ignored one."""
    mn, mx, ig = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
    for j, (x0, y0, x1, y1) in enumerate(rects):
        sl = (slice(max(y0, 0), y1 + 1), slice(max(x0, 0), x1 + 1))
        mn[sl] = np.where(mn[sl] == 0, j + 1, mn[sl])
        mx[sl] = j + 1
        if j < len(ignore) and ignore[j]:
            ig[sl] = 1
    return mn | (mx << 8) | (ig << 16)


def owner_map(cover, new_h, new_w, max_polys):
    """owner (1 + polygon index, 0: none) of every label cell: bits 8-15 of the cover word at the cv2.resize
    INTER_NEAREST source index, min(floor(o * (1 / (new / old))), old - 1) in double"""
    cover = np.asarray(cover).astype(np.int64) & 0xFFFFFFFF
    n, h, w = cover.shape
    ifx, ify = 1.0 / (f64(new_w) / f64(w)), 1.0 / (f64(new_h) / f64(h))
    sx = np.minimum(np.floor(np.arange(new_w) * ifx).astype(np.int64), w - 1)
    sy = np.minimum(np.floor(np.arange(new_h) * ify).astype(np.int64), h - 1)
    own = (cover[:, sy][:, :, sx] >> 8) & 255
    own[own > max_polys] = 0
    return own


def instance_weights(cover, ignore, new_h, new_w):
    """-> (area int32 [n, P], weight f32 [n, new_h, new_w], live bool [n, P])"""
    ignore = np.asarray(ignore)
    n, P = ignore.shape
    own = owner_map(cover, new_h, new_w, P)
    area = np.zeros((n, P), np.int32)
    weight = np.zeros((n, new_h, new_w), f32)
    live = np.zeros((n, P), bool)
    for b in range(n):
        area[b] = np.bincount(own[b].ravel(), minlength=P + 1)[1:P + 1]
        live[b] = (ignore[b] == 0) & (area[b] >= 1)
        N, S = int(live[b].sum()), int(area[b][live[b]].sum())
        for j in np.flatnonzero(live[b]):
            weight[b][own[b] == j + 1] = f32(f64(S) / (f64(N) * f64(area[b, j])))      # one rounding, from double
    return area, weight, live


# ------------------------------------------------------------------------------------------------ the loss
def blocks(total):
    return min(max(_cdiv(total, 1024), 1), 1024)


def m_sum(total):
    """additions behind one f32 sum: per-thread trips, 6 shuffles, 3 cross-wave additions, the f64 -> f32 rounding"""
    return _cdiv(total, blocks(total) * 256) + 6 + 3 + 1


def count(n_pos, ratio, n_neg):
    """the mining count: the product in double"""
    return int(min(f64(n_pos) * f64(f32(ratio)), f64(n_neg)))


def ce64(l0, l1, t):
    """(ce, d_ce, p1, log s, m, l_t) of the 2-class CE in float64"""
    l0, l1 = l0.astype(f64), l1.astype(f64)
    m = np.maximum(l0, l1)
    s = np.exp(l0 - m) + np.exp(l1 - m)
    lt = np.where(t, l1, l0)
    ce = np.log(s) + m - lt
    return ce, _g(2 * ELOG + 2) * (1 + np.log(s) + np.abs(m) + np.abs(lt)), np.exp(l1 - m) / s, np.log(s), m, lt


def focal64(l0, l1, t, alpha, gamma):
    """(L, d_L, dz1, d_dz1) of the focal term in float64 with first-order bounds"""
    alpha, gamma = f64(f32(alpha)), f64(f32(gamma))
    _, _, p1, logs, m, lt = ce64(l0, l1, t)
    p = np.where(t, p1, 1 - p1)
    logp = lt - m - logs
    a = np.where(t, alpha, f64(f32(1) - f32(alpha)))
    om = np.maximum(1 - p, 1e-30)
    rel_om = (7 * p + om) * U32 / om
    assert (rel_om < 0.5).all()
    omg = om ** gamma
    rel_omg = np.maximum(np.expm1(gamma * rel_om), gamma * rel_om / (1 - rel_om)) + 2 * EPOW * U32     # |(1 +- r)^g - 1|
    so = 1.01 * (1 + rel_omg)                                                                        # the second order
    dlogp = U32 * (np.abs(lt - m) + 4 + 2 * ELOG * logs + np.abs(logp))
    L = -a * omg * logp
    dL = so * (a * (np.abs(logp) * omg * rel_omg + omg * dlogp) + 4 * U32 * np.abs(L))
    T1, T2 = gamma * omg * p * logp, omg * om
    dT1 = np.abs(T1) * (rel_omg + 7 * U32 + 3 * U32) + np.abs(gamma * omg * p) * dlogp
    dT2 = np.abs(T2) * (rel_omg + rel_om + U32)
    dzt = a * (T1 - T2)
    ddzt = so * (a * (dT1 + dT2) + 3 * U32 * a * (np.abs(T1) + np.abs(T2)))
    return L, dL, np.where(t, dzt, -dzt), ddzt


def mine(c):
    """index work in float32 -> (threshold f32 [n], pixel weight W f32 [n, hw], P, mined, counts)"""
    with np.errstate(invalid="ignore"):
        P = c.w > 0
        neg = ~(c.plab > 0)
    score = O.neg_score_f32(c.pl[..., 0], c.pl[..., 1])
    thr, ks = np.full(c.n, -1, f32), []
    for i in range(c.n):
        k = count(P[i].sum(), c.neg_ratio, neg[i].sum())
        ks.append(k)
        if P[i].any() and k > 0:
            thr[i] = np.sort(score[i][neg[i]])[k - 1]
    mined = neg & (score <= thr[:, None]) & ~P
    return thr, np.where(P, c.w, np.where(mined, f32(1), f32(0))).astype(f32), P, mined, ks


def _reduced(v, d, total, axis=0):
    """float64 sum of the terms v and the bound of its f32 tree: g(m_sum) sum(|v| + d) + sum d"""
    return v.sum(axis), _g(m_sum(total)) * (np.abs(v) + d).sum(axis) + d.sum(axis)


def _weighted(v, d, w):
    """the terms v (formed within d) times the exact f32 weights w: the product adds one u"""
    return v * w, (d + U32 * (np.abs(v) + d)) * w


def _quot(a, da, b, db):
    """a / b in f32 from a, b known within da, db (b > db >= 0): propagated, plus the division's u twice over"""
    q = a / b
    return q, (da + abs(q) * db) / (b - db) + 2 * U32 * abs(q)


def loss_ref(c):
    """sums34 and loss10 in float64 with their bounds.  c: n, hw, focal, neg_ratio, alpha, gamma, pl [n,hw,2],
    ll [n,hw,16], plab [n,hw], llab [n,hw,8], w [n,hw] (all f32)"""
    r = NS()
    r.thr, r.W, r.P, r.mined, r.ks = mine(c)
    total = c.n * c.hw
    W = r.W.astype(f64)
    with np.errstate(invalid="ignore"):
        r.pos = c.plab > 0
        r.lp = c.llab > 0
    ce, dce, r.p1, *_ = ce64(c.pl[..., 0], c.pl[..., 1], r.pos)
    sums, bnd = np.zeros(34), np.zeros(34)
    sums[0], bnd[0] = _reduced(*(a.ravel() for a in _weighted(ce, dce, W)), total)
    sums[1], bnd[1] = _reduced(W.ravel(), np.zeros(total), total)
    a0, a1 = c.ll[..., 0::2], c.ll[..., 1::2]
    if c.focal:
        L, dL, r.dz1, r.ddz1 = focal64(a0, a1, r.lp, c.alpha, c.gamma)
    else:
        L, dL, q1, *_ = ce64(a0, a1, r.lp)
        r.dz1, r.ddz1 = q1 - r.lp, _g(8) * (q1 + 1)
    wP = np.where(r.P, c.w, f32(0)).astype(f64)                    # links count on P only
    for k, sel in ((2, r.lp), (4, ~r.lp)):
        w = (sel * wP[..., None]).reshape(total, 8)
        v, d = _weighted(L.reshape(total, 8), dL.reshape(total, 8), w)
        sums[k::4], bnd[k::4] = _reduced(v, d, total)
        sums[k + 1::4], bnd[k + 1::4] = _reduced(w, np.zeros_like(w), total)
    r.sums, r.sums_bound = sums, bnd
    loss, lb = np.zeros(10), np.zeros(10)
    if sums[1] > 0:
        loss[1], lb[1] = _quot(sums[0], bnd[0], sums[1], bnd[1])
    for d in range(8):
        lp, wp, ln, wn = sums[2 + 4 * d:6 + 4 * d]
        bp, bwp, bn, bwn = bnd[2 + 4 * d:6 + 4 * d]
        qp, dp = (0.0, 0.0) if wp == 0 else _quot(lp, bp, wp, bwp)
        qn, dn = (0.0, 0.0) if wn == 0 else _quot(ln, bn, wn, bwn)
        loss[2 + d] = qp + qn
        lb[2 + d] = dp + dn + U32 * abs(qp + qn)
    loss[0] = 2 * loss[1] + loss[2:].sum()
    lb[0] = 2 * lb[1] + lb[2:].sum() + 9 * U32 * (2 * abs(loss[1]) + np.abs(loss[2:]).sum())
    r.loss, r.loss_bound = loss, lb
    return r


def grad_ref(c, r, sums_dev, seed):
    """gradients in float64 from the sums the device wrote; seed = the f64 value of the f32 seed"""
    s = np.asarray(sums_dev).astype(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cpix = 2 * seed / s[1] if s[1] > 0 else 0.0
        wp, wn = s[3::4], s[5::4]
        cpos = np.where(wp == 0, 0.0, seed / wp)
        cneg = np.where(wn == 0, 0.0, seed / wn)
    W = r.W.astype(f64)
    g1 = (r.p1 - r.pos) * W * cpix
    b1 = _g(M_GRAD) * (r.p1 + 1) * W * abs(cpix)
    wP = np.where(r.P, c.w, f32(0)).astype(f64)[..., None]
    coef = wP * np.where(r.lp, cpos, cneg)
    gl = r.dz1 * coef
    bl = np.where(coef == 0, 0.0, (r.ddz1 + _g(5) * np.abs(r.dz1)) * np.abs(coef))
    dpl = np.stack([-g1, g1], -1)
    dll = np.stack([-gl, gl], -1).reshape(c.n, c.hw, 16)
    return dpl, np.stack([b1, b1], -1), dll, np.stack([bl, bl], -1).reshape(c.n, c.hw, 16)
