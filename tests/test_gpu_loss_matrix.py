"""GPU: every entry of csrc/loss_softmax.hip and csrc/loss_dice.hip — the fused softmax / OHNM / focal loss, its mined
mask and gradients, the mining helpers (ocr_label_masks, ocr_ohnm_select), the one-direction link CE and the dice loss,
the `_dyn` forms included — against a float64 restatement in NumPy of the formulas in the two file headers (no autograd,
no oracle loss routine, no device route compared with another).  Every entry is called through ctypes on the library
tensorflow_ocr_amd.ops binds and the status of each call is asserted.  Every output sits in a NaN-filled buffer between
guard bands, every strided output inside sentinel columns; both must be bit-identical after the call.
The one exception to float64 is index work: the mining score is restated in float32 with O.det_exp_f32 /
O.neg_score_f32, the sequence the kernel documents as shared; the threshold, the mined mask, the label masks and the
ocr_ohnm_select outputs must be bit-exact, and the float64 sums then use that mask as W.
The losses read no 16-bit operand and the bf16 library compiles the same code, so this file is not run a second time on
the bf16 library (tests/test_gpu_bf16.py).

Kernels and the rows that reach them
  ohnm_threshold_kernel     test_softmax (pixel_rule 0: SHAPES hw 1 | 63 | 1023 | 1024 | 1025 around the 1024-thread
                            stride), test_softmax_modes, test_directed_mining (ties, clamps, each radix pass, k clipped /
                            = n_neg / 1 / 0, images without positives / negatives / labels, non-integer ratios),
                            test_softmax_cap (262 272 negatives per image)
  sl_reduce_kernel, sl_finalize_kernel   test_softmax (1 to 5 partial rows: (5, 1000) and (2, 2100) give 5, one row
                            group of the finalisation adds two), test_softmax_modes (all 24 combinations pixel_rule x
                            label_rule x link_gate x focal at (3, 577) and (1, 1025)), test_focal, test_degenerate,
                            test_nonfinite, test_softmax_cap ((4, 262 272): 1024 blocks, second grid-stride pass)
  sl_selected_kernel        every softmax row (ocr_softmax_loss_selected: bit-exact against the reference mask)
  sl_bwd_kernel<SeedStatic|SeedDevice>   every softmax row (ocr_softmax_loss_bwd, ocr_softmax_loss_bwd_dyn)
  label_masks_kernel        test_label_masks: both rules x count 1 | 1023 | 1025 | 5000, labels 0, -0.0, 1, 0.5, -1, 2, NaN
  ohnm_select_kernel        test_ohnm_select: n 1..4 x hw 1 | 1023 | 1024 | 1025 | 5000 x negative / mixed / zeros
                            scores, n_pos_i32 with and without pos_mask, each output NULL; test_directed_mining (the
                            non-integer ratios, same k and same mask as the fused loss)
  link_ce_reduce_kernel, link_ce_finalize_kernel, link_ce_bwd_kernel<SeedStatic|SeedDevice>
                            test_link_ce: strides (1, 2, 2) | (8, 16, 16) at direction 3 | (3, 5, 7) x count 1 | 255 | 257 |
                            1025 | 5121, weights in [0, 2] with exact zeros; the row whose positives all weigh 0;
                            test_link_ce_cap (1 048 653: 1024 blocks, second pass)
  dice_reduce_kernel, dice_bwd_kernel<SeedStatic|SeedDevice>   test_dice (pc, G) = (2, 1) | (1, 2) | (3, 2) | (1, 3), and
                            (2, 2) | (1, 1) with every tensor offset by one float (test_dice_unaligned)
  dice_reduce22_kernel, dice_bwd22_kernel<...>   test_dice (2, 2), test_dice_cap (P = 1 049 605)
  dice_reduce11_kernel, dice_bwd11_kernel<...>   test_dice (1, 1)
  dice_finalize_kernel      test_dice: P 1 | 255 | 257 | 1023 | 1025 (1, 2 rows), 31 749 (32 rows), 33 792 (33), 263 171
                            (258 rows: second trip of the eight-in-flight loop), the cap (1024 rows)
  every OCR_CHECK_ARG / OCR_CHECK_SHAPE and both workspace checks of the two files: test_status_codes (nothing written)

Exact rows (dice, kind "exact"): labels, predictions and masks k / 8 in [0, 1]: every f32 partial sum is exact, the
finalisation adds in double, and sums27 must be the float64 sums rounded once, bit for bit.

Bounds (u = 2^-24; g(m) = m u / (1 - m u); no relative tolerance anywhere)
  A reduction of terms v_i that the kernel forms with |v^_i - v_i| <= d_i:
      |dev - ref| <= g(m_sum) * sum(|v_i| + d_i) + sum d_i + 2^-149,
      m_sum = ceil(total / (T * 256)) [per-thread trips] + 6 [shuffles] + 3 [cross-wave additions] + 1 [f64 -> f32].
  Library calls: expf 1 ulp (= 2 u, as the heads matrix takes it).  logf and powf: ROCm's accuracy table is not in
  the tree's reach, so each was measured alone (the device-library function against double, 2^24 arguments per range:
  logf on [1, 2] — the argument is e0 + e1 with the larger exponent 0 —, powf(x, g) for x in [1e-6, 1] and e^[-25, 0], g in
  {0, 0.7, 1.5, 2, 3.3}); one ulp is added: ELOG, EPOW below, figures in MEASURED.
  CE term  ce = logf(e0 + e1) + m - l_t:  d_ce = g(2 ELOG + 2) * (1 + |log s| + |m| + |l_t|).  The "1" carries the
      error of s (s >= 1: subtraction 0.37, two expf 2, addition 1: <= 4 u on log s), |log s| its 2 ELOG u and two
      later additions, |m| two, |l_t| one.
  focal term  L = -a (1 - p)^g log p: first-order propagation, one u per f32 operation: rel(p) <= 7 u (two expf, two
      subtractions, the sum, the division), d(om) = 7 u p + u om, rel(omg) = g rel(om) + 2 EPOW u, d(logp) = u (|l_t - m|
      + 4 + 2 ELOG |log s| + |logp|), d(L) = a (|logp| d(omg) + omg d(logp)) + 4 u |L|.  Where p is near 1, rel(om) =
      7 u p / om is no longer small (0.07 at om = 6e-6), so rel(omg) is taken exactly, max |(1 +- r)^g - 1| with
      r = rel(om) < 0.5 (asserted), and the other terms carry the factor 1.01 (1 + rel(omg)) for the second order.
  loss10: the sums' bounds propagated through the quotients to first order plus one u per f32 operation.
  gradients: referred to the sums the device wrote (each checked on its own).  CE: |dev - ref| <= g(13) (|p1| + 1) |coef|
      (p1 7, the subtraction 1 — its cancellation is what S = |p1| + 1 covers —, weight product 1, coefficient up to 3
      (n hw product, division, seed product), final product 1).  Focal: the same propagation as the loss term.
  dice sums: I = y ps m: d = g(pc + 1) |y| sum|p_j| |m| (pc - 1 additions, two products); A: g(1); B: g(pc).
  dice loss10: computed in double on the device from the double totals; the sums' bounds propagated, plus u per output.
  dice gradients: g(11) |m| (|y cU| + |cI|), cU and cI formed in float64 from the device's own sums27 with f32(1e-5)
      (U two additions, cU division + seed, cI four more, then multiply-add and the mask product).
  Every test prints `loss <entry> <row> ratio=<|err| / bound>`.

Findings
  * The mining count disagreed between the fused loss and the helper: ohnm_threshold_kernel took
    (int)fminf((float)n_pos * neg_ratio, (float)n_neg), ohnm_select_kernel the product in double.  (10, 0.7f),
    (20, 0.35f) and (10, 0.9f) round up in f32: 7 | 7 | 9 mined negatives against 6 | 6 | 8.  Both kernels now use the
    double form (test_directed_mining rows ratio0.7 | ratio0.35 | ratio0.9; the fused half fails with the f32 product).
  * dice_reduce22 / reduce11 / bwd22 / bwd11 read and write 8- and 16-byte vectors and the launchers never looked at the
    pointers.  ocr_dice_loss_fwd and the backward launcher now pick a vector kernel only when the pointers it vectorises
    are aligned, the generic kernel otherwise; test_dice_unaligned offsets every tensor by one float and gets the bits of
    the aligned run.
  * fill() validated neither label_rule, link_gate nor focal (any non-zero value meant 1, a label_rule of 2 meant 1),
    nor neg_ratio (negative or NaN: k <= 0 silently), nor n * hw against the int the mining kernels count pixels in.
    Now OCR_ERR_INVALID_ARG for the first four, OCR_ERR_UNSUPPORTED for n * hw > INT32_MAX; ocr_softmax_loss_workspace
    answers 0 for a non-positive n or hw instead of sizing from the product.
  * pixel_rule 1 without positives gives a NaN pixel term AND an all-NaN pixel gradient (0 * inf: W = 0 times
    c_pix = 2 g / 0); pinned as the header documents it (test_degenerate).
  * The threshold buffer is written under pixel_rule 0 only; under rules 1 and 2 it is neither read nor written
    (asserted: it keeps its fill).

MEASURED (largest |err| / bound over the rows, f16 library; 0.000 = bit-exact index work)
  softmax_loss_fwd_sums          0.113      link_ce_fwd_sums               0.146
  softmax_loss_fwd               0.113      link_ce_fwd                    0.029
  softmax_loss_bwd_pixel         0.158      link_ce_bwd                    0.207
  softmax_loss_bwd_link          0.253      link_ce_bwd_dyn                0.207
  softmax_loss_bwd_dyn_pixel     0.164      dice_loss_fwd_sums             0.170
  softmax_loss_bwd_dyn_link      0.259      dice_loss_fwd                  0.181
  label_masks                    0.000      dice_loss_bwd_pixel / _link    0.464 / 0.499
  ohnm_select                    0.000      dice_loss_bwd_dyn_pixel / _link  0.365 / 0.449
  dice_unaligned                 0.000 (bit-identical to the aligned run)
  Library functions alone on the MI355X (device-library function against double, 2^24 arguments per range, ulps of the
  result): logf on [1, 2] 2.064 (on [1, 1.001] 1.938: the result goes to 0 at 1); powf(x, g), x in [1e-6, 1] and
  e^[-25, 0]: g = 2 1.322, 1.5 1.302, 0.7 1.307, 3.3 1.311, 0 exact; expf on [-90, 0] 0.851 (taken as 1).  Hence
  ELOG = 3.064, EPOW = 2.322.
  No row was over its bound.  With the mining count of ohnm_threshold_kernel put back to the f32 product, the rows
  test_directed_mining[ratio0.7 | ratio0.35 | ratio0.9] fail on the threshold (7 | 7 | 9 negatives mined), the others pass.
  Time on the MI355X: the file's 161 tests 8.0 s; slowest test_softmax_cap 1.5 s and test_dice_cap 1.2 s (the float64
  references over 1 M pixels on the host), every other test under 0.6 s.
"""
import ctypes
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (FL, I64, INVALID_ARG, OK, SZ, U32, UNSUPPORTED, WORKSPACE, Guard, Strided, _bits_equal, _cdiv, _d32,
                            _g, _lib, _ratio, _rc, _rng, f32, f64)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "loss")
ELOG = 3.064        # ulps: logf measured 2.064 ulp on [1, 2] (the result goes to 0 at 1), plus one (MEASURED)
EPOW = 2.322        # ulps: powf measured 1.322 ulp over the rows' range, plus one (MEASURED)
M_GRAD = 13


def _blocks(total):
    return min(max(_cdiv(total, 1024), 1), 1024)


def _m_sum(total):
    return _cdiv(total, _blocks(total) * 256) + 6 + 3 + 1


def _cmp(entry, row, got, ref, bound):
    """NaN where the reference is NaN and nowhere else; |err| <= bound elsewhere"""
    got, ref, bound = np.asarray(got, f64), np.asarray(ref, f64), np.broadcast_to(np.asarray(bound, f64), np.shape(ref))
    assert got.shape == ref.shape, (entry, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s %s: NaN pattern differs (%d vs %d)" % (entry, row, np.isnan(got).sum(), nan.sum())
    inf = np.isinf(ref) & ~nan
    assert np.array_equal(got[inf], ref[inf])
    ok = ~(nan | inf)
    _note(entry, row, _ratio(np.abs(got[ok] - ref[ok]), bound[ok] + 2.0 ** -149))


def _reduced(v, d, total, axis=0):
    """float64 sum of the terms v and the bound of its f32 tree: g(m_sum) sum(|v| + d) + sum d"""
    return v.sum(axis), _g(_m_sum(total)) * (np.abs(v) + d).sum(axis) + d.sum(axis)


# ------------------------------------------------------------------------------------------------ float64 restatement
def _ce64(l0, l1, t):
    """(ce, d_ce, p1, log s, m, l_t) of the 2-class CE in float64"""
    l0, l1 = l0.astype(f64), l1.astype(f64)
    m = np.maximum(l0, l1)
    s = np.exp(l0 - m) + np.exp(l1 - m)
    lt = np.where(t, l1, l0)
    ce = np.log(s) + m - lt
    return ce, _g(2 * ELOG + 2) * (1 + np.log(s) + np.abs(m) + np.abs(lt)), np.exp(l1 - m) / s, np.log(s), m, lt


def _focal64(l0, l1, t, alpha, gamma):
    """(L, d_L, dz1, d_dz1) of focal2 in float64 with first-order bounds (docstring)"""
    alpha, gamma = f64(f32(alpha)), f64(f32(gamma))
    _, _, p1, logs, m, lt = _ce64(l0, l1, t)
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


def _labels(y, rule):
    with np.errstate(invalid="ignore"):
        pos = (y > 0) if rule else (y == 1)
        neg = ~(y > 0) if rule else (y == 0)
    return pos, neg


def _count(n_pos, ratio, n_neg):
    """the mining count, one definition: the product in double"""
    return int(min(f64(n_pos) * f64(f32(ratio)), f64(n_neg)))


def _mine(c):
    """index work in float32: per-image threshold and the pixel weight map W (bool)"""
    pos, neg = _labels(c.plab, c.label_rule)
    if c.pixel_rule == 2:
        return None, np.ones_like(pos), pos, []
    if c.pixel_rule == 1:
        return None, pos.copy(), pos, []
    score = O.neg_score_f32(c.pl[..., 0], c.pl[..., 1])
    thr, ks = np.full(c.n, -1, f32), []
    for i in range(c.n):
        k = _count(pos[i].sum(), c.neg_ratio, neg[i].sum())
        ks.append(k)
        if pos[i].any() and k > 0:
            thr[i] = np.sort(score[i][neg[i]])[k - 1]
    return thr, pos | (neg & (score <= thr[:, None])), pos, ks


def _softmax_ref(c):
    """sums34 and loss10 in float64 with their bounds, from the mined mask W"""
    r = NS()
    r.thr, r.W, r.pos, r.ks = _mine(c)
    total = c.n * c.hw
    W = r.W.astype(f64)
    ce, dce, r.p1, *_ = _ce64(c.pl[..., 0], c.pl[..., 1], r.pos)
    sums, bnd = np.zeros(34), np.zeros(34)
    sums[0], bnd[0] = _reduced((ce * W).ravel(), (dce * W).ravel(), total)
    sums[1] = r.pos.sum()
    G = W if c.link_gate else np.ones_like(W)
    r.lp, r.ln = _labels(c.llab, c.label_rule)
    a0, a1 = c.ll[..., 0::2], c.ll[..., 1::2]
    if c.focal:
        L, dL, r.dz1, r.ddz1 = _focal64(a0, a1, r.lp, c.alpha, c.gamma)
    else:
        L, dL, q1, *_ = _ce64(a0, a1, r.lp)
        r.dz1, r.ddz1 = q1 - r.lp, _g(8) * (q1 + 1)
    r.G = G
    for k, sel in ((2, r.lp), (4, r.ln)):
        w = (sel * G[..., None]).reshape(total, 8)
        sums[k::4], bnd[k::4] = _reduced(L.reshape(total, 8) * w, dL.reshape(total, 8) * w, total)
        sums[k + 1::4] = w.sum(0)
    r.sums, r.sums_bound = sums, bnd
    loss, lb = np.zeros(10), np.zeros(10)
    with np.errstate(divide="ignore", invalid="ignore"):
        if c.pixel_rule == 2:
            loss[1], lb[1] = sums[0] / total, bnd[0] / total + 3 * U32 * abs(sums[0] / total)
        elif c.pixel_rule == 0 and sums[1] == 0:
            loss[1] = 0.0
        else:
            loss[1] = sums[0] / sums[1]
            lb[1] = bnd[0] / sums[1] + 2 * U32 * abs(loss[1])
        for d in range(8):
            lp, wp, ln, wn = sums[2 + 4 * d:6 + 4 * d]
            bp, bn = bnd[2 + 4 * d], bnd[4 + 4 * d]
            if c.link_gate:
                qp, qn, dp, dn = lp / wp, ln / wn, bp / wp, bn / wn
            else:
                qp, dp = (0.0, 0.0) if wp == 0 else (lp / wp, bp / wp)
                qn, dn = (0.0, 0.0) if wn == 0 else (ln / wn, bn / wn)
            loss[2 + d] = qp + qn
            lb[2 + d] = dp + dn + 2 * U32 * (abs(qp) + abs(qn)) + U32 * abs(qp + qn)
        loss[0] = 2 * loss[1] + loss[2:].sum()
        lb[0] = 2 * lb[1] + lb[2:].sum() + 9 * U32 * (2 * abs(loss[1]) + np.abs(loss[2:]).sum())
    r.loss, r.loss_bound = loss, lb
    return r


def _softmax_grad_ref(c, r, sums_dev, seed):
    """gradients in float64 from the sums the device wrote; seed = the f64 value of the f32 seed"""
    s = sums_dev.astype(f64)
    total = c.n * c.hw
    with np.errstate(divide="ignore", invalid="ignore"):
        if c.pixel_rule == 2:
            cpix = 2 * seed / total
        elif c.pixel_rule == 0:
            cpix = 2 * seed / s[1] if s[1] > 0 else 0.0
        else:
            cpix = 2 * seed / s[1]
        wp, wn = s[3::4], s[5::4]
        cpos = np.where((not c.link_gate) & (wp == 0), 0.0, seed / wp)
        cneg = np.where((not c.link_gate) & (wn == 0), 0.0, seed / wn)
        W = r.W.astype(f64)
        g1 = (r.p1 - r.pos) * W * cpix
        b1 = _g(M_GRAD) * (r.p1 + 1) * W * abs(cpix)
        live = (r.G != 0)[..., None]
        coef = np.where(r.lp & live, r.G[..., None] * cpos, 0.0) + np.where(r.ln & live, r.G[..., None] * cneg, 0.0)
        gl = r.dz1 * coef
        bl = (r.ddz1 + _g(5) * np.abs(r.dz1)) * np.abs(coef)
    bl = np.where(coef == 0, 0.0, bl)
    dpl = np.stack([-g1, g1], -1)
    dll = np.stack([-gl, gl], -1).reshape(c.n, c.hw, 16)
    return dpl, np.stack([b1, b1], -1), dll, np.stack([bl, bl], -1).reshape(c.n, c.hw, 16)


# ------------------------------------------------------------------------------------------------ softmax rows
def _softmax_case(n, hw, mode, key=0, neg_ratio=3.0, alpha=0.25, gamma=2.0):
    pr, lr, gate, focal = mode
    rng = _rng("softmax", n, hw, key)
    c = NS(n=n, hw=hw, pixel_rule=pr, label_rule=lr, link_gate=gate, focal=focal, neg_ratio=neg_ratio, alpha=alpha, gamma=gamma)
    c.pl = (2 * rng.standard_normal((n, hw, 2))).astype(f32)
    c.ll = (2 * rng.standard_normal((n, hw, 16))).astype(f32)
    vals = np.array([1, 0, 0.5, -1, 2], f32)
    c.plab = rng.choice(vals, (n, hw), p=[0.2, 0.65, 0.05, 0.05, 0.05])
    c.llab = rng.choice(vals, (n, hw, 8), p=[0.4, 0.45, 0.05, 0.05, 0.05])
    c.row = "n%d_hw%d_m%d%d%d%d" % (n, hw, pr, lr, gate, focal)
    return c


def _desc(L, c, **over):
    v = dict(n=c.n, hw=c.hw, pixel_rule=c.pixel_rule, label_rule=c.label_rule, link_gate=c.link_gate, focal=c.focal,
             neg_ratio=c.neg_ratio, alpha=c.alpha, gamma=c.gamma)
    v.update(over)
    return L.SoftmaxLossDesc(v["n"], v["hw"], v["pixel_rule"], v["label_rule"], v["link_gate"], v["focal"],
                             float(v["neg_ratio"]), float(v["alpha"]), float(v["gamma"]))


def _run_softmax(device, c, grads=True, check=True):
    """fwd, selected, bwd and bwd_dyn on one case; everything checked against _softmax_ref"""
    L, _ = _lib()
    d = _desc(L, c)
    dr = ctypes.byref(d)
    total = c.n * c.hw
    nb = int(L._fn("ocr_softmax_loss_workspace", SZ)(dr))
    assert nb == _blocks(total) * 34 * 4
    pl, ll, plab, llab = (_d32(a, device) for a in (c.pl, c.ll, c.plab, c.llab))
    thr, sums, loss, ws = (Guard(s, torch.float32, device) for s in ((c.n,), (34,), (10,), (nb // 4,)))
    assert _rc(L, "ocr_softmax_loss_fwd", dr, pl, ll, plab, llab, thr, sums, loss, ws, SZ(nb)) == OK
    mask = Guard((c.n, c.hw), torch.uint8, device)
    # rules 1 and 2 never read the threshold: a buffer of their own that must keep its fill
    assert _rc(L, "ocr_softmax_loss_selected", dr, pl, plab, thr, mask) == OK
    torch.cuda.synchronize()
    r = _softmax_ref(c) if check else None
    out = NS(r=r, sums=sums.raw(), loss=loss.raw(), mask=mask.raw())
    assert ws.ok()
    if c.pixel_rule == 0:
        out.thr = thr.np()
    else:
        assert thr.untouched()
    if check:
        if c.pixel_rule == 0:
            assert np.array_equal(out.thr.view(np.int32), r.thr.view(np.int32)), (out.thr, r.thr)
        assert np.array_equal(out.mask, r.W.astype(np.uint8)), "mined mask: %d pixels differ" % int((out.mask != r.W).sum())
        counts = np.ones(34, bool)
        counts[0], counts[2::4], counts[4::4] = False, False, False
        assert np.array_equal(out.sums[counts], r.sums[counts].astype(f32)), "the count sums are exact"
        _cmp("softmax_loss_fwd_sums", c.row, out.sums, r.sums, r.sums_bound)
        _cmp("softmax_loss_fwd", c.row, out.loss, r.loss, r.loss_bound)
    if not grads:
        return out
    scale = _d32(np.array([3.0], f32), device)
    for name, seed, extra in (("ocr_softmax_loss_bwd", f32(1.7), ()), ("ocr_softmax_loss_bwd_dyn", f32(0.85) * f32(3.0), (scale,))):
        dpl, dll = Guard((c.n, c.hw, 2), torch.float32, device), Guard((c.n, c.hw, 16), torch.float32, device)
        gs = FL(1.7) if not extra else FL(0.85)
        assert _rc(L, name, dr, pl, ll, plab, llab, thr, sums, gs, *extra, dpl, dll) == OK
        torch.cuda.synchronize()
        out.dpl, out.dll = dpl.raw(), dll.raw()
        if check:
            rp, bp, rl, bl = _softmax_grad_ref(c, r, out.sums, f64(seed))
            entry = name[4:]
            _cmp(entry + "_pixel", c.row, out.dpl, rp, bp)
            _cmp(entry + "_link", c.row, out.dll, rl, bl)
    for t, a in ((pl, c.pl), (ll, c.ll), (plab, c.plab), (llab, c.llab)):
        assert np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32)), "an input was written"
    return out


SHAPES = [(1, 1), (1, 63), (1, 1023), (1, 1024), (1, 1025), (3, 577), (5, 1000), (2, 2100)]
NET_MODES = [(0, 0, 1, 0), (1, 1, 0, 1), (2, 0, 0, 0)]
ALL_MODES = [(p, l, g, f) for p in range(3) for l in range(2) for g in range(2) for f in range(2)]


@pytest.mark.parametrize("mode", NET_MODES, ids=["m%d%d%d%d" % m for m in NET_MODES])
@pytest.mark.parametrize("n,hw", SHAPES)
def test_softmax(device, n, hw, mode):
    """a direction without positive or negative links (certain at hw = 1) gives the NaN the header documents under
    link_gate 1: the reference's 0 / 0 must land on the same outputs"""
    assert _blocks(5 * 1000) == 5 and _blocks(2 * 2100) == 5
    _run_softmax(device, _softmax_case(n, hw, mode))


@pytest.mark.parametrize("mode", ALL_MODES, ids=["m%d%d%d%d" % m for m in ALL_MODES])
@pytest.mark.parametrize("n,hw", [(3, 577), (1, 1025)])
def test_softmax_modes(device, n, hw, mode):
    _run_softmax(device, _softmax_case(n, hw, mode, key=1))


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.5, 0.0), (0.25, 1.5), (0.75, 0.7)])
def test_focal(device, alpha, gamma):
    c = _softmax_case(3, 577, (0, 0, 1, 1), key=2, alpha=alpha, gamma=gamma)
    c.row += "_a%g_g%g" % (alpha, gamma)
    out = _run_softmax(device, c)
    if gamma == 0.0:
        # (0.5, 0): FL = 0.5 CE — against the float64 CE sums of the same inputs
        c2 = _softmax_case(3, 577, (0, 0, 1, 0), key=2)
        r2 = _softmax_ref(c2)
        k = np.array([j for j in range(2, 34) if j % 2 == 0])
        _cmp("softmax_loss_fwd_sums", c.row + "_half_ce", out.sums[k], 0.5 * r2.sums[k], out.r.sums_bound[k])


def _directed(call):
    """images of hw = 1500 built for one mining decision each; returns (case, per-image notes)"""
    hw = 1500
    rng = _rng("directed", call)
    imgs, notes = [], []

    def image(n_pos, n_neg, d_neg, other=0.5):
        """labels: n_pos ones, n_neg zeros, the rest `other`; logit difference l1 - l0 of the negatives from d_neg"""
        y = np.full(hw, other, f32)
        y[:n_pos] = 1
        y[n_pos:n_pos + n_neg] = 0
        l = np.zeros((hw, 2), f32)
        l[:, 1] = rng.standard_normal(hw).astype(f32)
        l[n_pos:n_pos + n_neg, 1] = d_neg(n_neg)
        l[:, 0] = (rng.integers(-8, 9, hw) / 4).astype(f32)
        l[:, 1] = l[:, 1] + l[:, 0]
        perm = rng.permutation(hw)
        imgs.append((y[perm], l[perm]))

    def bits(j, step):
        return lambda m: (-(rng.integers(0, 200, m)) * step).astype(f32)

    ratio = 3.0
    if call == "ratio3":
        image(100, 1400, lambda m: rng.choice([-1.0, -0.25, 0.5, 2.0], m).astype(f32)); notes.append("grid4")
        image(10, 1490, lambda m: np.zeros(m, f32)); notes.append("all_equal")
        image(400, 1100, lambda m: np.where(rng.random(m) < 0.7, -17 - 8 * rng.random(m), rng.standard_normal(m)).astype(f32)); notes.append("score_one")
        image(100, 1400, lambda m: rng.choice([-100.0, -85.0, 85.0, 100.0, 0.0], m).astype(f32)); notes.append("clamp")
        image(50, 1450, bits(0, 2.0 ** -22)); notes.append("top24")
        image(50, 1450, bits(0, 2.0 ** -14)); notes.append("top16")
        image(50, 1450, bits(0, 2.0 ** -6)); notes.append("top8")
        image(600, 900, lambda m: rng.standard_normal(m).astype(f32)); notes.append("k_clipped")
        image(300, 900, lambda m: rng.standard_normal(m).astype(f32)); notes.append("k_is_n_neg")
        image(0, 1200, lambda m: rng.standard_normal(m).astype(f32)); notes.append("no_pos")
        image(700, 0, lambda m: rng.standard_normal(m).astype(f32)); notes.append("no_neg")
        image(0, 0, lambda m: rng.standard_normal(m).astype(f32)); notes.append("no_labels")
        imgs[-1][0][::2] = -1
    elif call == "ratio0.5":
        ratio = 0.5
        image(2, 1000, lambda m: rng.standard_normal(m).astype(f32)); notes.append("k1")
        image(1, 1000, lambda m: rng.standard_normal(m).astype(f32)); notes.append("k0")
        image(300, 1000, lambda m: rng.standard_normal(m).astype(f32)); notes.append("k150")
    else:
        ratio, n_pos = {"ratio0.7": (0.7, 10), "ratio0.35": (0.35, 20), "ratio0.9": (0.9, 10)}[call]
        image(n_pos, 1000, lambda m: rng.standard_normal(m).astype(f32)); notes.append("np%d" % n_pos)
        image(n_pos, 1490 - n_pos, lambda m: rng.standard_normal(m).astype(f32)); notes.append("np%d_b" % n_pos)
    c = _softmax_case(len(imgs), hw, (0, 0, 1, 0), key=call, neg_ratio=ratio)
    c.plab = np.stack([y for y, _ in imgs])
    c.pl = np.stack([l for _, l in imgs])
    c.row = "directed_" + call
    return c, notes


@pytest.mark.parametrize("call", ["ratio3", "ratio0.5", "ratio0.7", "ratio0.35", "ratio0.9"])
def test_directed_mining(device, call):
    """one call of several images (thr[img] indexing), each built for one decision of the radix select"""
    L, _ = _lib()
    c, notes = _directed(call)
    out = _run_softmax(device, c)
    r = out.r
    pos, neg = _labels(c.plab, 0)
    score = O.neg_score_f32(c.pl[..., 0], c.pl[..., 1])
    sel = {nm: int((r.W[i] & neg[i]).sum()) for i, nm in enumerate(notes)}
    u = {nm: score[i][neg[i]].view(np.uint32) for i, nm in enumerate(notes)}
    k = dict(zip(notes, r.ks))
    print("loss directed %s: k %s selected %s thr %s" % (call, k, sel, dict(zip(notes, out.thr.tolist()))))
    if call == "ratio3":
        assert sel["grid4"] > k["grid4"] == 300, "the threshold value's multiplicity must straddle k"
        assert sel["all_equal"] == 1490 and k["all_equal"] == 30
        assert out.thr[notes.index("score_one")] == 1.0 and sel["score_one"] == 1100 and (u["score_one"] == 0x3F800000).sum() > 500
        assert (u["clamp"] == 0x3F800000).any() and (score[notes.index("clamp")] < 1e-30).any()      # both ends of the clamp
        for nm, hi, lo in (("top24", 8, 0), ("top16", 16, 8), ("top8", 24, 16)):
            assert len(np.unique(u[nm] >> hi)) == 1 and len(np.unique(u[nm] >> lo)) > 50, nm
        assert k["k_clipped"] == 900 == sel["k_clipped"] and k["k_is_n_neg"] == 900 == sel["k_is_n_neg"]
        for nm in ("no_pos", "no_neg", "no_labels"):
            assert out.thr[notes.index(nm)] == -1.0 and sel[nm] == 0
        assert out.mask[notes.index("no_neg")].sum() == 700 and out.mask[notes.index("no_labels")].sum() == 0
    elif call == "ratio0.5":
        assert (k["k1"], sel["k1"], k["k0"], sel["k0"], k["k150"], sel["k150"]) == (1, 1, 0, 0, 150, 150)
        assert out.thr[1] == -1.0
    else:
        want = {"ratio0.7": 6, "ratio0.35": 6, "ratio0.9": 8}[call]
        assert list(k.values()) == [want, want] and list(sel.values()) == [want, want], (k, sel)
        # the helper on the same scores and masks selects the mask the fused loss mines
        selected = Guard((c.n, c.hw), torch.float32, device)
        assert _rc(L, "ocr_ohnm_select", _d32(score, device), torch.from_numpy(pos.astype(np.uint8)).to(device),
                   torch.from_numpy(neg.astype(np.uint8)).to(device), None, c.n, c.hw, FL(c.neg_ratio), None, selected) == OK
        torch.cuda.synchronize()
        assert np.array_equal(selected.np(), out.mask.astype(f32))


@pytest.mark.parametrize("name", ["rule0_no_pos", "rule1_no_pos", "gate1_empty_dirs", "gate0_empty_dirs"])
def test_degenerate(device, name):
    mode = {"rule0_no_pos": (0, 0, 0, 0), "rule1_no_pos": (1, 1, 0, 0), "gate1_empty_dirs": (0, 0, 1, 0), "gate0_empty_dirs": (0, 0, 0, 0)}[name]
    c = _softmax_case(2, 700, mode, key=name)
    c.row = name
    if name.endswith("no_pos"):
        c.plab = np.where(c.plab > 0, f32(0), c.plab)
    else:
        c.llab[..., 3] = np.where(c.llab[..., 3] == 1, f32(0), c.llab[..., 3])      # direction 3: no positive link
        c.llab[..., 5] = np.where(c.llab[..., 5] == 0, f32(1), c.llab[..., 5])      # direction 5: no negative link
    out = _run_softmax(device, c)
    if name == "rule0_no_pos":
        assert out.loss[1] == 0.0 and not out.dpl.any() and np.isfinite(out.loss).all()
    elif name == "rule1_no_pos":
        assert np.isnan(out.loss[1]) and np.isnan(out.loss[0]) and np.isfinite(out.loss[2:]).all()
    elif name == "gate1_empty_dirs":
        assert np.isnan(out.loss[[0, 5, 7]]).all() and np.isfinite(out.loss[[1, 2, 3, 4, 6, 8, 9]]).all()
        assert np.isfinite(out.dll).all() and out.dll[..., 6:8].any() and out.dll[..., 10:12].any()
    else:
        assert np.isfinite(out.loss).all() and np.isfinite(out.dll).all()


def test_nonfinite(device):
    """a NaN and an Inf logit make loss[0] and the gradient at those elements non-finite (the dynamic loss scale reads
    exactly that); every other gradient element stays finite"""
    c = _softmax_case(2, 300, (2, 0, 0, 0), key="nonfinite")
    c.pl[0, 5, 1] = np.nan
    c.ll[1, 7, 4] = np.inf
    out = _run_softmax(device, c, check=False)
    assert not np.isfinite(out.loss[0])
    assert not np.isfinite(out.dpl[0, 5]).any() and not np.isfinite(out.dll[1, 7, 4:6]).any()
    bad_p, bad_l = np.zeros(out.dpl.shape, bool), np.zeros(out.dll.shape, bool)
    bad_p[0, 5], bad_l[1, 7, 4:6] = True, True
    assert np.isfinite(out.dpl[~bad_p]).all() and np.isfinite(out.dll[~bad_l]).all()


def test_softmax_cap(device):
    """(4, 262 272): 1025 blocks' work on 1024 (a second grid-stride pass), 262 272 pixels per image through the radix
    select; rule 0, gated"""
    n, hw = 4, 262272
    assert _cdiv(n * hw, 1024) > 1024
    c = _softmax_case(n, hw, (0, 0, 1, 0), key="cap")
    c.plab = np.where(_rng("cap_lab").random((n, hw)) < 0.02, f32(1), f32(0))       # 262 272 labelled pixels, ~5 000 positive
    c.row = "cap"
    _run_softmax(device, c)


# ------------------------------------------------------------------------------------------------ mining helpers
LABEL_VALUES = np.array([0.0, -0.0, 1.0, 0.5, -1.0, 2.0, np.nan], f32)


@pytest.mark.parametrize("count", [1, 1023, 1025, 5000])
@pytest.mark.parametrize("rule", [0, 1])
def test_label_masks(device, rule, count):
    L, _ = _lib()
    y = LABEL_VALUES[(np.arange(count) * 5 + rule) % 7] if count < 8 else _rng("lm", count).choice(LABEL_VALUES, count)
    if count >= 8:
        y[:7] = LABEL_VALUES
    pos, neg = Guard((count,), torch.uint8, device), Guard((count,), torch.uint8, device)
    assert _rc(L, "ocr_label_masks", _d32(y, device), I64(count), rule, pos, neg) == OK
    torch.cuda.synchronize()
    rp, rn = _labels(y, rule)
    assert np.array_equal(pos.raw(), rp.astype(np.uint8)) and np.array_equal(neg.raw(), rn.astype(np.uint8))
    _note("label_masks", "rule%d_%d" % (rule, count), 0.0)


def _select_ref(scores, pos, neg, n_pos, ratio):
    n, hw = scores.shape
    sn = np.zeros((n, hw), f32)
    for i in range(n):
        npos = int(n_pos[i]) if n_pos is not None else int(pos[i].sum())
        k = _count(npos, ratio, neg[i].sum())
        if npos > 0 and k > 0:
            thr = np.sort(scores[i][neg[i]])[k - 1]
            sn[i] = neg[i] & (scores[i] <= thr)
    return sn, sn + (pos.astype(f32) if pos is not None else 0)


@pytest.mark.parametrize("kind", ["negative", "mixed", "zeros"])
@pytest.mark.parametrize("n,hw", [(1, 1), (2, 1023), (3, 1024), (4, 1025), (2, 5000)])
def test_ohnm_select(device, n, hw, kind):
    L, _ = _lib()
    rng = _rng("select", n, hw, kind)
    sc = rng.standard_normal((n, hw)).astype(f32)
    if kind == "negative":
        sc = -np.abs(sc) - f32(0.5)
    lab = rng.choice([0, 1, 2], (n, hw), p=[0.7, 0.2, 0.1])
    if hw == 1:
        lab[:] = 0
    pos, neg = lab == 1, lab == 0
    npos = np.maximum(pos.sum(1), 1).astype(np.int32)
    if kind == "zeros" and hw > 1:
        # a fifth negative-valued, two fifths -0.0 / +0.0 mixed, the rest positive; k (through n_pos_i32) lands inside the zeros
        q = rng.random((n, hw))
        sc = np.where(q < 0.2, -np.abs(sc) - f32(0.1), np.where(q < 0.4, f32(-0.0), np.where(q < 0.6, f32(0.0), np.abs(sc) + f32(0.1))))
        npos = np.array([max(int(((sc[i] < 0) & neg[i]).sum()) // 3 + 3, 1) for i in range(n)], np.int32)
    ratios = (3.0, 0.7) if kind == "mixed" else (3.0,)
    scd, posd, negd = _d32(sc, device), torch.from_numpy(pos.astype(np.uint8)).to(device), torch.from_numpy(neg.astype(np.uint8)).to(device)
    nposd = torch.from_numpy(npos).to(device)
    for ratio in ratios:
        for pm, cnt in ((posd, None), (None, nposd), (posd, nposd)):
            rs, ra = _select_ref(sc, pos if pm is not None else None, neg, npos if cnt is not None else None, ratio)
            if kind == "zeros" and hw > 1 and cnt is not None:
                zero = neg & (sc == 0)
                assert all(rs[i][zero[i]].all() and (np.signbit(sc[i][zero[i]]).any() and not np.signbit(sc[i][zero[i]]).all()) for i in range(n))
                assert all(not rs[i][neg[i] & (sc[i] > 0)].any() for i in range(n)), "the threshold falls on zero"
            for want in ((1, 1), (1, 0), (0, 1)):
                o = [Guard((n, hw), torch.float32, device) if w else None for w in want]
                assert _rc(L, "ocr_ohnm_select", scd, pm, negd, cnt, n, hw, FL(ratio), o[0], o[1]) == OK
                torch.cuda.synchronize()
                if o[0] is not None:
                    assert np.array_equal(o[0].np(), rs)
                if o[1] is not None:
                    assert np.array_equal(o[1].np(), ra)
    _note("ohnm_select", "n%d_hw%d_%s" % (n, hw, kind), 0.0)


# ------------------------------------------------------------------------------------------------ link CE
def _link_case(count, strides, key, zero_pos=False):
    gs, ps, ds = strides
    rng = _rng("link", count, strides, key)
    c = NS(count=count, gs=gs, ps=ps, ds=ds, row="c%d_s%d_%d_%d%s" % (count, gs, ps, ds, "_zero_pos" if zero_pos else ""))
    c.go, c.po = (3, 6) if gs == 8 else (0, 0)                 # direction 3 of 8- / 16-channel maps
    c.gt = rng.choice(np.array([1, 0, 0.5], f32), count, p=[0.45, 0.45, 0.1])
    c.pred = (2 * rng.standard_normal((count, 2))).astype(f32)
    w = rng.uniform(0, 2, count).astype(f32)
    c.w = np.where(rng.random(count) < 0.2, f32(0), w)
    if zero_pos:
        c.w = np.where(c.gt == 1, f32(0), c.w)
    return c


def _run_link(device, c):
    L, _ = _lib()
    P = c.count
    gt = Strided(P, c.gs, c.go, 1, device, c.gt[:, None])
    pred = Strided(P, c.ps, c.po, 2, device, c.pred)
    w = _d32(c.w, device)
    nb = int(L._fn("ocr_link_ce_workspace", SZ)(I64(P)))
    assert nb == _blocks(P) * 16
    sums, loss, ws = Guard((4,), torch.float32, device), Guard((1,), torch.float32, device), Guard((nb // 4,), torch.float32, device)
    gp, pp = gt.g.t.view(-1)[c.go:], pred.g.t.view(-1)[c.po:]
    assert _rc(L, "ocr_link_ce_fwd", gp, c.gs, pp, c.ps, w, I64(P), sums, loss, ws, SZ(nb)) == OK
    torch.cuda.synchronize()
    lp, ln = c.gt == 1, c.gt == 0
    ce, dce, q1, *_ = _ce64(c.pred[:, 0], c.pred[:, 1], lp)
    w64 = c.w.astype(f64)
    ref, bnd = np.zeros(4), np.zeros(4)
    for k, sel in ((0, lp), (2, ln)):
        ws_ = w64 * sel
        ref[k], bnd[k] = _reduced(ce * ws_, (dce + U32 * np.abs(ce)) * ws_, P)
        ref[k + 1], bnd[k + 1] = _reduced(ws_, 0 * ws_, P)
    sd = sums.raw()
    _cmp("link_ce_fwd_sums", c.row, sd, ref, bnd)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = [ref[0] / ref[1], ref[2] / ref[3]]
        db = [(bnd[k] + abs(q[k // 2]) * bnd[k + 1]) / ref[k + 1] * 1.01 + 2 * U32 * abs(q[k // 2]) for k in (0, 2)]
        _cmp("link_ce_fwd", c.row, loss.raw(), np.array([q[0] + q[1]]), np.array([db[0] + db[1] + U32 * abs(q[0] + q[1])]))
    assert ws.ok()
    scale = _d32(np.array([3.0], f32), device)
    s = sd.astype(f64)
    for name, seed, gsc, extra in (("ocr_link_ce_bwd", f32(1.7), 1.7, ()), ("ocr_link_ce_bwd_dyn", f32(0.85) * f32(3.0), 0.85, (scale,))):
        do = 1 if c.ds > 2 else 0
        dp = Strided(P, c.ds, do, 2, device)
        assert _rc(L, name, gp, c.gs, pp, c.ps, w, I64(P), sums, FL(gsc), *extra, dp.g.t.view(-1)[do:], c.ds) == OK
        torch.cuda.synchronize()
        live = np.zeros(c.ds, bool)
        live[do:do + 2] = True
        a = dp.g.raw()
        assert np.array_equal(a[:, ~live].view(np.int32), dp.host[:, ~live].view(np.int32)), "sentinel columns written"
        with np.errstate(divide="ignore", invalid="ignore"):
            cp, cn = f64(seed) / s[1], f64(seed) / s[3]
            coef = np.where(lp & (w64 != 0), w64 * cp, 0.0) + np.where(ln & (w64 != 0), w64 * cn, 0.0)
        gl = (q1 - lp) * coef
        bl = _g(M_GRAD) * (q1 + 1) * np.abs(coef)
        _cmp(name[4:], c.row, a[:, live], np.stack([-gl, gl], -1), np.stack([bl, bl], -1))
    gt.np(), pred.np()
    return loss.raw(), a[:, live]


LINK_STRIDES = [(1, 2, 2), (8, 16, 16), (3, 5, 7)]


@pytest.mark.parametrize("strides", LINK_STRIDES, ids=["s%d_%d_%d" % s for s in LINK_STRIDES])
@pytest.mark.parametrize("count", [1, 255, 257, 1025, 5 * 1024 + 1])
def test_link_ce(device, count, strides):
    """count = 1 has one class only: the other quotient is 0 / 0 and the loss NaN, as the reference's"""
    _run_link(device, _link_case(count, strides, 0))


def test_link_ce_zero_weight_positives(device):
    loss, grad = _run_link(device, _link_case(1025, (1, 2, 2), 1, zero_pos=True))
    assert np.isnan(loss[0]) and np.isfinite(grad).all() and grad.any()


def test_link_ce_cap(device):
    P = 1024 * 1024 + 77
    assert _cdiv(P, 1024) > 1024
    _run_link(device, _link_case(P, (1, 2, 2), 2))


# ------------------------------------------------------------------------------------------------ dice
def _dice_case(P, pc, G, kind, key=0):
    rng = _rng("dice", P, pc, G, kind, key)
    c = NS(P=P, pc=pc, G=G, kind=kind, row="P%d_pc%d_G%d_%s" % (P, pc, G, kind))
    if kind == "exact":
        d = lambda s: (rng.integers(0, 9, s) / 8.0).astype(f32)
        c.ytp, c.ypp, c.ytl, c.ypl, c.mask = d(P), d((P, pc)), d((P, 8)), d((P, 8 * G)), d(P)
    else:
        b = lambda s, p: (rng.random(s) < p).astype(f32)
        c.ytp, c.ytl = b(P, 0.3), b((P, 8), 0.4)
        c.ypp, c.ypl = rng.random((P, pc)).astype(f32), rng.random((P, 8 * G)).astype(f32)
        c.mask = b(P, 0.8) if kind == "binary" else rng.uniform(0, 1.5, P).astype(f32)
        if kind == "zero_mask":
            c.mask[:] = 0
        if kind == "zero_labels":
            c.ytp[:], c.ytl[:] = 0, 0
    return c


def _dice_ref(c):
    P, m = c.P, c.mask.astype(f64)
    sums, bnd = np.zeros(27), np.zeros(27)
    maps = [(c.ytp.astype(f64), c.ypp.astype(f64), c.pc)] + [(c.ytl[:, i].astype(f64), c.ypl[:, i * c.G:(i + 1) * c.G].astype(f64), c.G) for i in range(8)]
    for k, (y, p, ch) in enumerate(maps):
        ps, pa = p.sum(1), np.abs(p).sum(1)
        sums[3 * k], bnd[3 * k] = _reduced(y * ps * m, _g(ch + 1) * np.abs(y) * pa * np.abs(m), P)
        sums[3 * k + 1], bnd[3 * k + 1] = _reduced(y * m, _g(1) * np.abs(y * m), P)
        sums[3 * k + 2], bnd[3 * k + 2] = _reduced(ps * m, _g(ch) * pa * np.abs(m), P)
    I, U = sums[0::3], sums[1::3] + sums[2::3] + 1e-5
    dl = 1 - 2 * I / U
    db = 1.01 * (2 * bnd[0::3] / U + 2 * np.abs(I) * (bnd[1::3] + bnd[2::3]) / U ** 2) + U32 * np.abs(dl)
    wk = np.array([2.0] + [1.0] * 8)
    loss = np.concatenate([[(wk * dl).sum()], dl])
    lb = np.concatenate([[(wk * db).sum() + U32 * abs((wk * dl).sum())], db])
    return sums, bnd, loss, lb


def _dice_grad_ref(c, sums_dev, seed):
    s = sums_dev.astype(f64)
    I, U = s[0::3], s[1::3] + s[2::3] + f64(f32(1e-5))
    wk = np.array([2.0] + [1.0] * 8) * seed
    cU, cI = -2 * wk / U, 2 * wk * I / (U * U)
    m = c.mask.astype(f64)
    y = np.concatenate([c.ytp[:, None], c.ytl], 1).astype(f64)
    g = m[:, None] * (y * cU + cI)
    b = _g(11) * np.abs(m)[:, None] * (np.abs(y * cU) + np.abs(cI))
    return (np.repeat(g[:, :1], c.pc, 1), np.repeat(b[:, :1], c.pc, 1), np.repeat(g[:, 1:], c.G, 1), np.repeat(b[:, 1:], c.G, 1))


def _off(a, device, shift):
    """a device copy of `a` whose first element sits `shift` floats past a 16-byte boundary"""
    t = torch.empty(a.size + 4, dtype=torch.float32, device=device)
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, f32).ravel()))
    return v


class OffGuard:
    """Guard whose live region starts `shift` floats into the NaN fill; the skipped floats must keep their fill"""

    def __init__(self, shape, device, shift):
        self.n, self.shape, self.shift = int(np.prod(shape)), shape, shift
        self.g = Guard((self.n + 4,), torch.float32, device)
        self.t = self.g.t[shift:shift + self.n]

    def raw(self):
        a = self.g.raw().view(np.int32)
        assert (a[:self.shift] == -1).all() and (a[self.shift + self.n:] == -1).all(), "written outside the tensor"
        return a[self.shift:self.shift + self.n].view(f32).reshape(self.shape)


def _run_dice(device, c, shift=0, check=True):
    L, _ = _lib()
    P, pc, G = c.P, c.pc, c.G
    ytp, ypp, ytl, ypl, mask = (_off(a, device, shift) for a in (c.ytp, c.ypp, c.ytl, c.ypl, c.mask))
    nb = int(L._fn("ocr_dice_workspace", SZ)(ctypes.c_int(P)))
    assert nb == _blocks(P) * 27 * 4
    sums, loss, ws = Guard((27,), torch.float32, device), Guard((10,), torch.float32, device), Guard((nb // 4,), torch.float32, device)
    assert _rc(L, "ocr_dice_loss_fwd", ytp, ypp, pc, ytl, ypl, G, mask, P, sums, loss, ws, SZ(nb)) == OK
    torch.cuda.synchronize()
    out = NS(sums=sums.np(), loss=loss.np(), grads=[])
    assert ws.ok()
    if check:
        rs, bs, rl, bl = _dice_ref(c)
        if c.kind == "exact":
            # every f32 partial sum is exact and the finalisation adds them in double: the one rounding left is the last
            _bits_equal(out.sums, rs.astype(f32), "sums27 " + c.row)
            _note("dice_loss_fwd_sums", c.row, 0.0)
        else:
            _cmp("dice_loss_fwd_sums", c.row, out.sums, rs, bs)
        _cmp("dice_loss_fwd", c.row, out.loss, rl, bl)
    scale = _d32(np.array([3.0], f32), device)
    for name, seed, gsc, extra in (("ocr_dice_loss_bwd", f32(1.7), 1.7, ()), ("ocr_dice_loss_bwd_dyn", f32(0.85) * f32(3.0), 0.85, (scale,))):
        dpp, dpl = OffGuard((P, pc), device, shift), OffGuard((P, 8 * G), device, shift)
        assert _rc(L, name, ytp, pc, ytl, G, mask, P, sums, FL(gsc), *extra, dpp.t, dpl.t) == OK
        torch.cuda.synchronize()
        gp, gl = dpp.raw(), dpl.raw()
        assert not np.isnan(gp).any() and not np.isnan(gl).any()
        out.grads += [gp, gl]
        if check:
            rp, bp, rl_, bl_ = _dice_grad_ref(c, out.sums, f64(seed))
            _cmp(name[4:] + "_pixel", c.row, gp, rp, bp)
            _cmp(name[4:] + "_link", c.row, gl, rl_, bl_)
    return out


DICE_CH = [(1, 1), (2, 2), (2, 1), (1, 2), (3, 2), (1, 3)]
DICE_P = [1, 255, 257, 1023, 1025]


@pytest.mark.parametrize("kind", ["exact", "binary", "real"])
@pytest.mark.parametrize("pc,G", DICE_CH)
def test_dice(device, pc, G, kind):
    for P in DICE_P:
        _run_dice(device, _dice_case(P, pc, G, kind))


@pytest.mark.parametrize("P,rows", [(31 * 1024 + 5, 32), (33 * 1024, 33), (257 * 1024 + 3, 258)])
@pytest.mark.parametrize("pc,G", [(2, 2), (1, 1), (3, 2)])
def test_dice_partial_rows(device, pc, G, P, rows):
    """32 rows: every row group of dice_finalize_kernel has one; 33: one group has two; 258: the second trip of the
    eight-in-flight loop"""
    assert _blocks(P) == rows
    _run_dice(device, _dice_case(P, pc, G, "real"))
    _run_dice(device, _dice_case(P, pc, G, "exact"))


@pytest.mark.parametrize("pc,G", [(2, 2), (1, 1), (3, 2)])
def test_dice_zero_mask_and_labels(device, pc, G):
    out = _run_dice(device, _dice_case(1025, pc, G, "zero_mask"))
    assert np.array_equal(out.loss, np.array([10] + [1] * 9, f32)) and not out.sums.any()
    assert all(not g.any() for g in out.grads)
    out = _run_dice(device, _dice_case(1025, pc, G, "zero_labels"))
    assert np.array_equal(out.loss, np.array([10] + [1] * 9, f32))


def test_dice_cap(device):
    P = 1024 * 1024 + 1029
    assert _cdiv(P, 1024) > 1024
    _run_dice(device, _dice_case(P, 2, 2, "real"))


@pytest.mark.parametrize("pc,G", [(2, 2), (1, 1)])
def test_dice_unaligned(device, pc, G):
    """every tensor one float past a 16-byte boundary: the launchers take the generic kernels, which promise the same
    sums in the same order — bit-identical to the aligned run, forward and backward"""
    for P in (257, 5 * 1024 + 3):
        c = _dice_case(P, pc, G, "real", key="unaligned")
        a, b = _run_dice(device, c), _run_dice(device, c, shift=1)
        assert np.array_equal(a.sums.view(np.int32), b.sums.view(np.int32))
        assert np.array_equal(a.loss.view(np.int32), b.loss.view(np.int32))
        for x, y in zip(a.grads, b.grads):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
    _note("dice_unaligned", "pc%d_G%d" % (pc, G), 0.0)


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes(device):
    """every OCR_CHECK_ARG / OCR_CHECK_SHAPE of loss_softmax.hip and loss_dice.hip as read from the launchers, and both
    workspace checks one byte short.  Nothing may be written."""
    L, _ = _lib()
    n, hw, P = 2, 48, 96
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    pl, ll, plab, llab, w = z(n, hw, 2), z(n, hw, 16), z(n, hw), z(n, hw, 8), z(P)
    u8 = torch.zeros((n, hw), dtype=torch.uint8, device=device)
    i32 = torch.ones(n, dtype=torch.int32, device=device)
    scale = torch.ones(1, dtype=torch.float32, device=device)
    G = {k: Guard(s, d, device) for k, (s, d) in {
        "thr": ((n,), torch.float32), "s34": ((34,), torch.float32), "l10": ((10,), torch.float32), "ws": ((1024,), torch.float32),
        "dpl": ((n, hw, 2), torch.float32), "dll": ((n, hw, 16), torch.float32), "m8": ((n, hw), torch.uint8), "n8": ((n, hw), torch.uint8),
        "sel": ((n, hw), torch.float32), "sel2": ((n, hw), torch.float32), "s4": ((4,), torch.float32), "l1": ((1,), torch.float32),
        "s27": ((27,), torch.float32)}.items()}
    c = NS(n=n, hw=hw, pixel_rule=0, label_rule=0, link_gate=1, focal=0, neg_ratio=3.0, alpha=0.25, gamma=2.0)
    good = _desc(L, c)
    byref = ctypes.byref
    s34, s4, s27 = z(34), z(4), z(27)
    nb = SZ(int(L._fn("ocr_softmax_loss_workspace", SZ)(byref(good))))
    nbl = SZ(int(L._fn("ocr_link_ce_workspace", SZ)(I64(P))))
    nbd = SZ(int(L._fn("ocr_dice_workspace", SZ)(ctypes.c_int(P))))
    # entry: (arguments, indices of the required pointers)
    E = {
        "ocr_softmax_loss_fwd": ([byref(good), pl, ll, plab, llab, G["thr"], G["s34"], G["l10"], G["ws"], nb], [1, 2, 3, 4, 5, 6, 7, 8]),
        "ocr_softmax_loss_selected": ([byref(good), pl, plab, w, G["m8"]], [1, 2, 3, 4]),
        "ocr_softmax_loss_bwd": ([byref(good), pl, ll, plab, llab, w, s34, FL(1.0), G["dpl"], G["dll"]], [1, 2, 3, 4, 5, 6, 8, 9]),
        "ocr_softmax_loss_bwd_dyn": ([byref(good), pl, ll, plab, llab, w, s34, FL(1.0), scale, G["dpl"], G["dll"]], [1, 2, 3, 4, 5, 6, 8, 9, 10]),
        "ocr_label_masks": ([plab, I64(P), 0, G["m8"], G["n8"]], [0, 3, 4]),
        "ocr_ohnm_select": ([plab, u8, u8, i32, n, hw, FL(3.0), G["sel"], G["sel2"]], [0, 2]),
        "ocr_link_ce_fwd": ([plab, 1, pl, 2, w, I64(P), G["s4"], G["l1"], G["ws"], nbl], [0, 2, 4, 6, 7, 8]),
        "ocr_link_ce_bwd": ([plab, 1, pl, 2, w, I64(P), s4, FL(1.0), G["dpl"], 2], [0, 2, 4, 6, 8]),
        "ocr_link_ce_bwd_dyn": ([plab, 1, pl, 2, w, I64(P), s4, FL(1.0), scale, G["dpl"], 2], [0, 2, 4, 6, 8, 9]),
        "ocr_dice_loss_fwd": ([plab, pl, 2, llab, ll, 2, w, P, G["s27"], G["l10"], G["ws"], nbd], [0, 1, 3, 4, 6, 8, 9, 10]),
        "ocr_dice_loss_bwd": ([plab, 2, llab, 2, w, P, s27, FL(1.0), G["dpl"], G["dll"]], [0, 2, 4, 6, 8, 9]),
        "ocr_dice_loss_bwd_dyn": ([plab, 2, llab, 2, w, P, s27, FL(1.0), scale, G["dpl"], G["dll"]], [0, 2, 4, 6, 8, 9, 10]),
    }

    def bad(name, j, v, want=INVALID_ARG):
        a = list(E[name][0])
        a[j] = v
        assert _rc(L, name, *a) == want, (name, j, v)

    for name, (args, req) in E.items():
        for j in req:
            bad(name, j, None)
    # the descriptor: NULL, n, hw <= 0, each rule out of range, neg_ratio < 0 or NaN, n * hw beyond int
    for name in ("ocr_softmax_loss_fwd", "ocr_softmax_loss_selected", "ocr_softmax_loss_bwd", "ocr_softmax_loss_bwd_dyn"):
        bad(name, 0, None)
        for over in (dict(n=0), dict(n=-1), dict(hw=0), dict(hw=-3), dict(pixel_rule=-1), dict(pixel_rule=3), dict(label_rule=-1),
                     dict(label_rule=2), dict(link_gate=2), dict(link_gate=-1), dict(focal=2), dict(focal=-1), dict(neg_ratio=-0.5),
                     dict(neg_ratio=float("nan"))):
            bad(name, 0, byref(_desc(L, c, **over)))
        bad(name, 0, byref(_desc(L, c, n=65536, hw=32768)), UNSUPPORTED)
    assert int(L._fn("ocr_softmax_loss_workspace", SZ)(None)) == 0
    assert int(L._fn("ocr_softmax_loss_workspace", SZ)(byref(_desc(L, c, n=0)))) == 0
    bad("ocr_softmax_loss_fwd", 9, SZ(nb.value - 1), WORKSPACE)
    bad("ocr_link_ce_fwd", 9, SZ(nbl.value - 1), WORKSPACE)
    bad("ocr_dice_loss_fwd", 11, SZ(nbd.value - 1), WORKSPACE)
    for v in (0, -1):
        bad("ocr_label_masks", 1, I64(v))
        bad("ocr_ohnm_select", 4, v)
        bad("ocr_ohnm_select", 5, v)
        for name in ("ocr_link_ce_fwd", "ocr_link_ce_bwd", "ocr_link_ce_bwd_dyn"):
            bad(name, 5, I64(v))
            bad(name, 1, v)                                                  # gt_stride < 1
        bad("ocr_dice_loss_fwd", 7, v)
        bad("ocr_dice_loss_fwd", 2, v)
        bad("ocr_dice_loss_fwd", 5, v)
        for name in ("ocr_dice_loss_bwd", "ocr_dice_loss_bwd_dyn"):
            bad(name, 5, v)
            bad(name, 1, v)
            bad(name, 3, v)
    for v in (2, -1):
        bad("ocr_label_masks", 2, v)
    for name in ("ocr_link_ce_fwd", "ocr_link_ce_bwd", "ocr_link_ce_bwd_dyn"):
        bad(name, 3, 1)                                                      # pred_stride < 2
    bad("ocr_link_ce_bwd", 9, 1)                                             # d_stride < 2
    bad("ocr_link_ce_bwd_dyn", 10, 1)
    bad("ocr_ohnm_select", 6, FL(-1.0))
    bad("ocr_ohnm_select", 6, FL(float("nan")))
    a = list(E["ocr_ohnm_select"][0])                                        # pos_mask and n_pos_i32 both NULL; both outputs NULL
    a[1], a[3] = None, None
    assert _rc(L, "ocr_ohnm_select", *a) == INVALID_ARG
    a = list(E["ocr_ohnm_select"][0])
    a[7], a[8] = None, None
    assert _rc(L, "ocr_ohnm_select", *a) == INVALID_ARG
    torch.cuda.synchronize()
    for k, g in G.items():
        assert g.untouched(), k
    # and the same buffers take a well-formed call
    assert _rc(L, "ocr_label_masks", *E["ocr_label_masks"][0]) == OK
    torch.cuda.synchronize()
    assert bool((G["n8"].t == 1).all()) and not bool(G["m8"].t.any())
