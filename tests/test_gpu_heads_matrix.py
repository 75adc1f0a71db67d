"""GPU: every entry of csrc/heads.hip — the 1x1 wide-to-narrow MFMA convolutions, their input and weight gradients, the
small-channel f32 pyramid (sc_*), the sigmoid heads and the batched forms of all of these — against a float64 restatement
in NumPy on the same operands (no autograd, no oracle routine, no device route compared with another).  Every entry is
called through ctypes on the library tensorflow_ocr_amd.ops binds and the status of each call is asserted.  Operands the
kernels read as 16-bit are drawn on the storage grid; where a kernel rounds on load (dz * grad_scale in the input
gradient, dz in the MFMA and batched weight gradients) the reference rounds the float64 operand the same way first.
Weights go through ocr_pack_weights_small_f16, whose [32][cin] / [cin][32] layouts are asserted.  Every output sits in a
NaN-filled buffer between guard bands, every strided output inside sentinel columns; both must be bit-identical after
the call.  loss_dice.hip and loss_softmax.hip have their own matrix (test_gpu_loss_matrix.py); ocr_bn_finalize_batch and
ocr_bn_bwd_sums_batch are rows of test_gpu_bn_pool_matrix.py.

Kernels and the rows that reach them
  conv1x1_small_kernel                 test_conv: CONV_ROWS (P 1 | 31 | 33 | 129 | 257 x cin 16 | 48 | 80 | 128 | 1024 x
                                       cout 1 | 2 | 9 | 18 | 32, bias / NULL)
  conv1x1_small_batch_kernel           test_conv (count 1, statistics), test_conv_batch (count 1..4, statistics NULL /
                                       given), test_conv_batch_iters2 (P = 131 075: two groups per workgroup)
  conv1x1_small_dgrad_kernel           test_dgrad: DGRAD_ROWS (cin 32 | 96 | 128 | 1024, cout 1 | 9 | 17 | 18 | 32, P 1 | 33 |
                                       129, accumulate 0 | 1, grad_scale 1 | 2^-7 | 128)
  conv1x1_small_dgrad_batch_kernel     test_dgrad_batch: count 1..4, items alternating accumulate
  pad_dz_kernel, take_cols_kernel      test_small_wgrad rows mfma_* (the MFMA route of ocr_conv1x1_small_wgrad_f16)
  conv1x1_small_wgrad_narrow_kernel    test_small_wgrad rows narrow_* (1, 2 and 3 strips)
  conv1x1_small_wgrad_kernel           test_small_wgrad rows valu_* (1 strip, 2 strips, cin = 264: second grid row,
                                       cin = 20: no multiple of 8), test_small_wgrad_strip_cap (256 strips)
  head_wgrad_kernel, head_wgrad_reduce_kernel   test_head_wgrad (HW_ROWS, count 1..4), test_head_wgrad_capped
  sum_partials_kernel                  launched by no entry of the file (dead code; listed so the inventory is whole)
  sc_stats_kernel                      test_sc_stats (ocr_sc_stats, ocr_sc_colsum), SC_C x P 1 | lanes*8-1 | lanes*8+1,
                                       test_sc_block_cap (P = 114 703 at C = 18: 1024 blocks, second pass)
  sc_stats_batch_kernel                test_sc_stats (ocr_sc_colsum_batch, C <= 32), test_sc_block_cap
  sc_bn_bwd_kernel                     test_sc_bn_bwd (<0> and <1>, relu 0 | 1), test_sc_block_cap
  sc_bn_bwd_batch_kernel               test_sc_bn_bwd (C <= 32, count 3), test_sc_block_cap
  sc_fuse_kernel                       test_fuse: MAPS x C 1 | 18 x every subset of {a, b, prev} x affine or not x relu;
                                       test_fuse_cap ((1, 244, 244) at C = 18: 4187 blocks' work on 4096)
  sc_unpool_bwd_kernel                 test_unpool_bwd (explicit interpolation matrix, inner-product identity),
                                       test_fuse_cap (low map (1, 244, 244): second pass)
  sc_act_batch_kernel                  test_sigmoid_act (count 1..4, relu 0 | 1)
  sc_pointwise_fwd_kernel, sc_pointwise_dgrad_kernel, sc_pointwise_wgrad_kernel   test_pointwise 3->5, 18->7, 32->15
  sc_pointwise_square_kernel           test_pointwise 2->2 and 16->16 (forward and TRANSPOSE)
  sc_pointwise_wgrad16_kernel, sc_pointwise_wgrad2_kernel                         test_pointwise 16->16, 2->2
  sc_pointwise_pair_fwd_kernel, sc_pointwise_pair_dgrad_kernel, sc_pointwise_pair_wgrad_kernel, sum_rows_batch_kernel
                                       test_pair (P 1 | 1023 | 1025), test_pair_cap (P = 1 048 876)
  sc_sigmoid_kernel, sc_sigmoid_bwd_kernel, sc_sigmoid_split_kernel, sc_sigmoid_split_bwd_kernel   test_sigmoid_act
  every OCR_CHECK_ARG / OCR_CHECK_SHAPE of the file: test_status_codes (nothing may be written)

Exact rows (kind "exact"): operands k / 8 in [-4, 4] (weights of the MFMA convolutions: two entries of +-0.5 | +-1 per
output channel, so the squares of the outputs stay exact too), scales in {0.5, 1, 2}; every partial sum is exact in f32
and the device must match bit for bit, a zero's sign apart.

Random rows, derived bounds (u = storage half-ulp 2^-11 | 2^-8; g(m) = m 2^-24 / (1 - m 2^-24); S = sum of |terms| in
float64; m = the sequential f32 roundings on the longest path, one per addition, two per multiply-add that the compiler
need not fuse):
  f32 outputs        |dev - ref| <= g(m) S (+ 2^-149)
  16-bit outputs     |dev - ref| <= u |ref| + g(m) S + the smallest subnormal
  m per entry        conv1x1_small: cin + 1 (each product once, bias); its statistics: 16 iters + 4 on top of the outputs'
                     own bounds; dgrad: cout + 1; small_wgrad VALU: 2 strip + ceil(S / 64) + 6, narrow: 2 ceil(strip /
                     lanes) + lanes + ceil(S / 64) + 6, MFMA: P (any order of P terms); head_wgrad: 64 tiles_per_split +
                     ceil(splits / 64) + 6; sc_stats: n_it + lanes (sums), 2 n_it + lanes (squares), n_it = ceil(P / (T
                     lanes)); colsum: + ceil(T / 64) + 6 (batch: + 1, the f64 row sum rounded once); sc_bn_bwd dbeta as
                     colsum, dgamma + 3, dz 8; sc_fuse 8 (2 per affine, 4 for the two lerps, 2 additions); unpool_bwd 9;
                     pointwise fwd 2 cin, dgrad 2 cout, wgrad 2 strip + 32; pair statistics n_it + 9 on top of the
                     outputs' bounds; sigmoid 4 (expf 1 ulp, add, divide), sigmoid_bwd 3, act 2.
ReLU masks decide on the sign of an f32 z * sc + sh: evaluated fused and unfused in the reference; an element where the
two disagree in sign is fragile and skipped with every channel sum it feeds; the fragile share is asserted <= 0.1 % and at
least three quarters of the channels stay checked, from the reference alone.

Measured, largest |err| / bound per entry over its rows (f16 / bf16 library), from the `heads <entry> <row> ratio=`
lines: see MEASURED at the end of this docstring.

Findings
  * ocr_conv1x1_small_wgrad_f16 validated cin nowhere.  The VALU strip kernel walks channels one by one, so a cin that is
    no multiple of 8 is correct (row valu_cin20); cin <= 0 sized an empty grid: now OCR_ERR_UNSUPPORTED (test_status_codes).
  * ocr_sc_pointwise_fwd / _dgrad / _wgrad took any ld / offset: ldx < xo + cin or ldo < oo + cout (or a negative offset)
    read and wrote the neighbouring pixel's row.  Now OCR_ERR_INVALID_ARG; fwd and dgrad refuse cin or cout > 32 like
    wgrad (OCR_ERR_UNSUPPORTED), and wgrad answers the shape before the workspace (test_status_codes).
  * head_wgrad_plan returns the RECOMPUTED split count: at P = 524 800, cin = 128 it launches 249 splits of 33 tiles (the
    last one 16), not the 256 of the cap — no launched split is empty, and the slab has 249 rows
    (test_head_wgrad_capped asserts the slab size).  The kernel's empty-split path (mt_begin >= mt_end) is unreachable.
  * ocr_sc_bn_bwd and ocr_sc_colsum are documented to need (T + 1) * 2 * C floats of partial and write T * 2 * C: the
    last row stays untouched (asserted).  ocr_sc_colsum_batch uses C floats of that row, ocr_sc_bn_bwd_batch needs T * 2 * C.
  * grad_scale before or after the 16-bit rounding of dz differs only where one of the two leaves the normal range of
    the storage type: the random rows with grad_scale 2^-7 draw |dz| beyond 65504 and those with 128 draw dz below
    2^-14, so that dz * grad_scale is a normal f16 number and dz alone is not.  In the bf16 build the two orders agree
    (f32's exponent range).
  * sum_partials_kernel is launched by nothing.

MEASURED (largest |err| / bound over the rows, f16 / bf16 library; a stored 16-bit output that is right to the last bit
still shows its final rounding, up to 0.999 of u |ref|: the two dgrad lines)
  conv1x1_small                  0.054 / 0.051      sc_fuse                        0.282 / 0.282
  conv1x1_small_batch            0.122 / 0.110      sc_unpool_bwd                  0.465 / 0.465
  conv1x1_small_batch_stats      0.039 / 0.037      sc_act_batch                   0.496 / 0.496
  conv1x1_small_dgrad            0.995 / 0.995      sc_pointwise_fwd               0.435 / 0.435
  conv1x1_small_dgrad_batch      0.990 / 0.996      sc_pointwise_dgrad             0.335 / 0.335
  conv1x1_small_wgrad            0.034 / 0.019      sc_pointwise_wgrad             0.028 / 0.028
  conv1x1_small_wgrad_batch      0.020 / 0.018      sc_pointwise_pair_fwd          0.599 / 0.599
  sc_stats                       0.240 / 0.240      sc_pointwise_pair_fwd_stats    0.124 / 0.124
  sc_colsum                      0.079 / 0.079      sc_pointwise_pair_bwd          0.481 / 0.481
  sc_colsum_batch                0.053 / 0.053      sc_sigmoid, sc_sigmoid_split   0.486 / 0.486
  sc_bn_bwd                      0.408 / 0.408      sc_sigmoid_bwd                 0.607 / 0.607
  sc_bn_bwd_batch                0.388 / 0.388      sc_sigmoid_split_bwd           0.799 / 0.799
  The f32 entries read no 16-bit operand, so both libraries give the same figure.  Long sums stay far below m 2^-24 S
  (random signs); the short elementwise chains (2 to 4 roundings) come closest to it.  No row was over its bound.
  Time on the MI355X: the file's 180 tests 6.7 s (f16) / 5.9 s (bf16); slowest test_pair_cap 1.6 s (a float64 reference
  over 1 048 876 pixels on the host); the 524 800-pixel weight gradient 0.6 s, most of it drawing 67 M operands and the
  chunked float64 product on the host.
"""
import ctypes
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (FL, I64, INVALID_ARG, OK, SZ, TINY, U16, UNSUPPORTED, WORKSPACE, Guard, Strided, _bits_equal,
                            _cdiv, _d32, _dev, _exact32, _g, _h, _items, _lib, _ratio, _rc, _rng, f32, f64)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

KINDS = ("exact", "random")
_note = partial(matrix_support._note, "heads")


# ------------------------------------------------------------------------------------------------ host helpers
def _draw(rng, shape, kind, sd=1.0, grid=False):
    if kind == "exact":
        return (rng.integers(-32, 33, shape) / 8.0).astype(f32)
    v = (rng.standard_normal(shape) * sd).astype(f32)
    return _h(v) if grid else v


def _pow2(rng, shape, kind, lo=0.5, hi=1.5):
    if kind == "exact":
        return rng.choice([0.5, 1.0, 2.0], shape).astype(f32)
    return rng.uniform(lo, hi, shape).astype(f32)


def _c32(entry, row, got, ref, m, S, kind, skip=None):
    """an f32 output against float64: bit for bit on an exact row, |err| <= g(m) S otherwise"""
    got, ref = np.asarray(got), np.asarray(ref, f64)
    assert got.shape == ref.shape, (entry, got.shape, ref.shape)
    if kind == "exact":
        _bits_equal(got, _exact32(ref), "%s %s" % (entry, row), skip)
        return _note(entry, row + "_exact", 0.0)
    _note(entry, row, _ratio(np.abs(got.astype(f64) - ref), _g(m) * np.asarray(S, f64) + 2.0 ** -149, skip))


def _c16(entry, row, got, ref, m, S, kind):
    got, ref = np.asarray(got), np.asarray(ref, f64)
    assert got.shape == ref.shape
    if kind == "exact":
        _bits_equal(got, _h(_exact32(ref)), "%s %s" % (entry, row))
        return _note(entry, row + "_exact", 0.0)
    assert np.isfinite(got).all()
    _note(entry, row, _ratio(np.abs(got.astype(f64) - ref), U16 * np.abs(ref) + _g(m) * np.asarray(S, f64) + TINY))


# ------------------------------------------------------------------------------------------------ packed weights
def _pack(L, w, device):
    """w f32 [cin][cout] on the storage grid -> (w_kc32 [32][cin], w_ck32 [cin][32]), layouts asserted"""
    cin, cout = w.shape
    kc, ck = Guard((32, cin), O.STORAGE, device), Guard((cin, 32), O.STORAGE, device)
    assert _rc(L, "ocr_pack_weights_small_f16", _d32(w, device), cin, cout, kc, ck) == OK
    torch.cuda.synchronize()
    wk = np.zeros((32, cin), f32)
    wk[:cout] = w.T
    _bits_equal(kc.np(), wk, "w_kc32")
    _bits_equal(ck.np(), np.ascontiguousarray(wk.T), "w_ck32")
    assert not kc.np()[cout:].any() and not ck.np()[:, cout:].any()
    return kc, ck


def _conv_w(rng, cin, cout, kind):
    if kind == "exact":
        w = np.zeros((cin, cout), f32)
        for co in range(cout):
            w[rng.choice(cin, 2, replace=False), co] = rng.choice([-1.0, -0.5, 0.5, 1.0], 2)
        return w
    return _h(rng.standard_normal((cin, cout)) / np.sqrt(cin))


# ------------------------------------------------------------------------------------------------ conv1x1_small
CONV_ROWS = [(1, 16, 1, 0), (31, 48, 2, 1), (33, 80, 9, 0), (129, 128, 18, 1), (257, 1024, 32, 1), (129, 16, 18, 0),
             (33, 1024, 9, 1), (257, 48, 32, 0), (31, 128, 1, 1), (1, 80, 18, 1), (257, 80, 2, 0), (33, 128, 32, 1)]


def _conv_case(L, device, P, cin, cout, bias, kind, key):
    rng = _rng("conv", P, cin, cout, bias, kind, key)
    c = NS(P=P, cin=cin, cout=cout, kind=kind, row="P%d_ci%d_co%d_b%d" % (P, cin, cout, bias))
    c.x = _draw(rng, (P, cin), kind, grid=True)
    c.w = _conv_w(rng, cin, cout, kind)
    c.b = _draw(rng, (cout,), kind) if bias else None
    c.kc, c.ck = _pack(L, c.w, device)
    c.xd = _dev(c.x, device)
    c.bd = _d32(c.b, device) if bias else None
    c.ref = c.x.astype(f64) @ c.w.astype(f64) + (c.b.astype(f64) if bias else 0.0)
    c.S = np.abs(c.x).astype(f64) @ np.abs(c.w).astype(f64) + (np.abs(c.b).astype(f64) if bias else 0.0)
    c.m = cin + 1
    c.iters = _cdiv(P, 128 * 1024)
    c.T = _cdiv(P, 128 * c.iters)
    return c


def _check_conv_stats(entry, c, part):
    """per-workgroup sums of out and out^2 over ITS rows below P against float64 sums of the float64 product"""
    T, C, span = c.T, c.cout, 128 * c.iters
    blk = np.arange(c.P) // span
    bz = (_g(c.m) * c.S if c.kind != "exact" else 0.0 * c.S) + 2.0 ** -149
    s, q, ss, sq, bs, bq = (np.zeros((T, C)) for _ in range(6))
    np.add.at(s, blk, c.ref)
    np.add.at(q, blk, c.ref ** 2)
    np.add.at(ss, blk, np.abs(c.ref))
    np.add.at(bs, blk, bz)
    np.add.at(bq, blk, 2 * np.abs(c.ref) * bz + bz ** 2)
    m = 16 * c.iters + 4
    if c.kind == "exact":
        _bits_equal(part[:, 0], _exact32(s), entry + " sums")
        _bits_equal(part[:, 1], _exact32(q), entry + " squares")
        return _note(entry + "_stats", c.row + "_exact", 0.0)
    r = max(_ratio(np.abs(part[:, 0] - s), bs + _g(m) * ss), _ratio(np.abs(part[:, 1] - q), bq + _g(m + 1) * q))
    _note(entry + "_stats", c.row, r)


@pytest.mark.parametrize("P,cin,cout,bias", CONV_ROWS, ids=["P%d_ci%d_co%d_b%d" % r for r in CONV_ROWS])
@pytest.mark.parametrize("kind", KINDS)
def test_conv(device, P, cin, cout, bias, kind):
    L, ops = _lib()
    c = _conv_case(L, device, P, cin, cout, bias, kind, 0)
    out = Guard((P, cout), torch.float32, device)
    assert _rc(L, "ocr_conv1x1_small_f16", c.xd, c.kc, c.bd, P, cin, cout, out) == OK
    torch.cuda.synchronize()
    _c32("conv1x1_small", c.row, out.np(), c.ref, c.m, c.S, kind)
    assert int(L._fn("ocr_conv1x1_small_batch_rows", ctypes.c_int)(ctypes.c_int(P))) == c.T
    out2, part = Guard((P, cout), torch.float32, device), Guard((c.T, 2, cout), torch.float32, device)
    arr = _items(ops.HeadConvItem, [(c.xd, c.kc, c.bd, out2, part, P, cin, cout)])
    assert _rc(L, "ocr_conv1x1_small_batch_f16", arr, 1) == OK
    torch.cuda.synchronize()
    _c32("conv1x1_small_batch", c.row, out2.np(), c.ref, c.m, c.S, kind)
    _check_conv_stats("conv1x1_small_batch", c, part.np())


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_conv_batch(device, count, kind):
    """count items of different (P, cin, cout); statistics given on the even items, NULL on the odd ones"""
    L, ops = _lib()
    shapes = [(129, 48, 18, 1), (31, 128, 2, 0), (257, 16, 9, 1), (1, 80, 32, 1)][:count]
    cs = [_conv_case(L, device, *s, kind, count) for s in shapes]
    outs = [Guard((c.P, c.cout), torch.float32, device) for c in cs]
    parts = [Guard((c.T, 2, c.cout), torch.float32, device) if i % 2 == 0 else None for i, c in enumerate(cs)]
    arr = _items(ops.HeadConvItem, [(c.xd, c.kc, c.bd, o, p, c.P, c.cin, c.cout) for c, o, p in zip(cs, outs, parts)])
    assert _rc(L, "ocr_conv1x1_small_batch_f16", arr, count) == OK
    torch.cuda.synchronize()
    for i, (c, o, p) in enumerate(zip(cs, outs, parts)):
        _c32("conv1x1_small_batch", "n%d_i%d_%s" % (count, i, c.row), o.np(), c.ref, c.m, c.S, kind)
        if p is not None:
            _check_conv_stats("conv1x1_small_batch", c, p.np())


def test_conv_batch_iters2(device):
    """P just above 131 072: iters = 2, 513 workgroups of 256 pixels, the last one 3 pixels of its first group"""
    L, ops = _lib()
    c = _conv_case(L, device, 131075, 16, 18, 1, "random", 0)
    assert (c.iters, c.T) == (2, 513)
    out, part = Guard((c.P, 18), torch.float32, device), Guard((c.T, 2, 18), torch.float32, device)
    arr = _items(ops.HeadConvItem, [(c.xd, c.kc, c.bd, out, part, c.P, 16, 18)])
    assert _rc(L, "ocr_conv1x1_small_batch_f16", arr, 1) == OK
    torch.cuda.synchronize()
    _c32("conv1x1_small_batch", "iters2", out.np(), c.ref, c.m, c.S, "random")
    _check_conv_stats("conv1x1_small_batch", c, part.np())


# ------------------------------------------------------------------------------------------------ dgrad
DGRAD_ROWS = [(1, 32, 1, 0, 1.0), (33, 96, 9, 1, 2.0 ** -7), (129, 128, 17, 0, 128.0), (33, 1024, 18, 1, 1.0),
              (129, 96, 32, 0, 2.0 ** -7), (1, 128, 17, 1, 128.0), (33, 32, 18, 0, 1.0), (129, 1024, 9, 1, 1.0),
              (33, 128, 18, 1, 128.0)]


def _dgrad_case(L, device, P, cin, cout, acc, gs, kind, key):
    rng = _rng("dgrad", P, cin, cout, acc, gs, kind, key)
    c = NS(P=P, cin=cin, cout=cout, acc=acc, kind=kind, row="P%d_ci%d_co%d_a%d_gs%g" % (P, cin, cout, acc, gs))
    if kind == "exact":
        c.dz = _draw(rng, (P, cout), kind)
    elif gs < 1:     # |dz| beyond the f16 range, dz * gs inside it
        c.dz = (rng.standard_normal((P, cout)) * 256.0 / gs).astype(f32)
    elif gs > 1:     # dz below the smallest normal f16, dz * gs above it
        c.dz = (rng.standard_normal((P, cout)) * 2.0 ** -9 / gs).astype(f32)
    else:
        c.dz = rng.standard_normal((P, cout)).astype(f32)
    c.w = _draw(rng, (cin, cout), kind, 0.25, grid=True)
    c.old = _draw(rng, (P, cin), kind, float(np.abs(c.dz).mean() * gs), grid=True)
    _, c.ck = _pack(L, c.w, device)
    b = _h((c.dz.astype(f64) * gs).astype(f32)).astype(f64)            # (power-of-two scale: exact before the rounding)
    assert np.array_equal((c.dz.astype(f64) * gs).astype(f32).astype(f64), c.dz.astype(f64) * gs)
    c.ref = b @ c.w.astype(f64).T + (c.old.astype(f64) if acc else 0.0)
    c.S = np.abs(b) @ np.abs(c.w).astype(f64).T + (np.abs(c.old).astype(f64) if acc else 0.0)
    c.m = cout + 1
    c.dzd = _d32(c.dz, device)
    c.dx = Guard((P, cin), O.STORAGE, device, c.old)
    return c


@pytest.mark.parametrize("P,cin,cout,acc,gs", DGRAD_ROWS, ids=["P%d_ci%d_co%d_a%d_gs%g" % r for r in DGRAD_ROWS])
@pytest.mark.parametrize("kind", KINDS)
def test_dgrad(device, P, cin, cout, acc, gs, kind):
    L, ops = _lib()
    c = _dgrad_case(L, device, P, cin, cout, acc, gs, kind, 0)
    assert _rc(L, "ocr_conv1x1_small_dgrad_f16", c.dzd, c.ck, P, cin, cout, FL(gs), c.dx, acc) == OK
    torch.cuda.synchronize()
    _c16("conv1x1_small_dgrad", c.row, c.dx.np(), c.ref, c.m, c.S, kind)


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_dgrad_batch(device, count, kind):
    L, ops = _lib()
    gs = [1.0, 2.0 ** -7, 128.0, 1.0][count - 1]
    shapes = [(129, 96, 18), (33, 128, 17), (1, 1024, 9), (130, 32, 32)][:count]
    cs = [_dgrad_case(L, device, P, cin, cout, i % 2, gs, kind, count) for i, (P, cin, cout) in enumerate(shapes)]
    arr = _items(ops.HeadDgradItem, [(c.dzd, c.ck, c.dx, c.P, c.cin, c.cout, c.acc) for c in cs])
    assert _rc(L, "ocr_conv1x1_small_dgrad_batch_f16", arr, count, FL(gs)) == OK
    torch.cuda.synchronize()
    for i, c in enumerate(cs):
        _c16("conv1x1_small_dgrad_batch", "n%d_i%d_%s" % (count, i, c.row), c.dx.np(), c.ref, c.m, c.S, kind)


# ------------------------------------------------------------------------------------------------ small wgrad
def _narrow(cin):
    return cin in (8, 16, 32, 64)


def _small_wgrad_route(P, cin):
    if _narrow(cin):
        return "narrow"
    return "mfma" if P % 32 == 0 and cin % 32 == 0 else "valu"


SW_ROWS = {"mfma_ci128": (64, 128, 18), "mfma_co5": (96, 96, 5), "mfma_ci160": (32, 160, 1),
           "narrow_1strip": (1000, 16, 9), "narrow_2strips": (1025, 64, 18), "narrow_3strips": (2500, 8, 2),
           "valu_1strip": (100, 40, 9), "valu_2strips": (2049, 48, 2), "valu_ci264": (77, 264, 1), "valu_cin20": (100, 20, 18)}


def _small_wgrad(L, device, name, P, cin, cout, kind):
    rng = _rng("sw", name, kind)
    route = _small_wgrad_route(P, cin)
    assert route == name.split("_")[0]
    x = _draw(rng, (P, cin), kind, grid=True)
    dz = _draw(rng, (P, cout), kind)
    dzr = _h(dz) if route == "mfma" else dz
    nbytes = L.call_size("ocr_conv1x1_small_wgrad_workspace", ctypes.c_int(P), ctypes.c_int(cin), ctypes.c_int(cout))
    if route == "valu":
        S = min(_cdiv(P, 2048), 256)
        strip = _cdiv(P, S)
        m = 2 * strip + _cdiv(S, 64) + 6
        assert nbytes == S * cin * cout * 4
    elif route == "narrow":
        S = _cdiv(P, 1024)
        strip, lanes = _cdiv(P, S), 256 // (cin // 8)
        m = 2 * _cdiv(strip, lanes) + lanes + _cdiv(S, 64) + 6
        assert nbytes == S * cin * cout * 4
    else:
        m = P
    ws, dw = Guard((nbytes,), torch.uint8, device), Guard((cin, cout), torch.float32, device)
    xd, dzd = _dev(x, device), _d32(dz, device)
    assert _rc(L, "ocr_conv1x1_small_wgrad_f16", xd, dzd, P, cin, cout, dw, ws, SZ(nbytes - 1)) == WORKSPACE
    torch.cuda.synchronize()
    assert dw.untouched() and ws.untouched()
    assert _rc(L, "ocr_conv1x1_small_wgrad_f16", xd, dzd, P, cin, cout, dw, ws, SZ(nbytes)) == OK
    torch.cuda.synchronize()
    assert ws.ok()
    ref, Sm = np.zeros((cin, cout)), np.zeros((cin, cout))
    for p0 in range(0, P, 65536):
        xs, ds = x[p0:p0 + 65536].astype(f64), dzr[p0:p0 + 65536].astype(f64)
        ref += xs.T @ ds
        Sm += np.abs(xs).T @ np.abs(ds)
    _c32("conv1x1_small_wgrad", name, dw.np(), ref, m, Sm, kind)


@pytest.mark.parametrize("name", list(SW_ROWS))
@pytest.mark.parametrize("kind", KINDS)
def test_small_wgrad(device, name, kind):
    L, ops = _lib()
    _small_wgrad(L, device, name, *SW_ROWS[name], kind)


def test_small_wgrad_strip_cap(device):
    """P > 524 288 at the narrowest cin of the strip route: 256 strips of 2049 pixels, the last one 1858"""
    L, ops = _lib()
    P = 524353
    assert (min(_cdiv(P, 2048), 256), _cdiv(P, 256), P - 255 * 2049) == (256, 2049, 1858)
    _small_wgrad(L, device, "valu_cap", P, 3, 2, "random")


def test_small_wgrad_refusals(device):
    L, ops = _lib()
    for P, cin in ((100, 16), (100, 40)):        # the narrow and the strip route instantiate cout 1, 2, 8, 9, 16, 18
        ws, dw = Guard((1 << 16,), torch.uint8, device), Guard((cin, 5), torch.float32, device)
        x, dz = torch.zeros((P, cin), dtype=O.STORAGE, device=device), torch.zeros((P, 5), dtype=torch.float32, device=device)
        assert _rc(L, "ocr_conv1x1_small_wgrad_f16", x, dz, P, cin, 5, dw, ws, SZ(1 << 16)) == UNSUPPORTED
        assert _rc(L, "ocr_conv1x1_small_wgrad_f16", x, dz, P, 0, 5, dw, ws, SZ(1 << 16)) == UNSUPPORTED
        assert _rc(L, "ocr_conv1x1_small_wgrad_f16", x, dz, P, -8, 5, dw, ws, SZ(1 << 16)) == UNSUPPORTED
        torch.cuda.synchronize()
        assert dw.untouched() and ws.untouched()


# ------------------------------------------------------------------------------------------------ head wgrad (batched)
HW_ROWS = [(1, 128, 1), (63, 384, 18), (65, 128, 32), (2049, 384, 1), (4161, 128, 18)]


def _hw_plan(P):
    mt = _cdiv(P, 64)
    sp = max(min(_cdiv(mt, 32), 256), 1)
    tps = _cdiv(mt, sp)
    return mt, tps, _cdiv(mt, tps)


def _hw_case(L, device, P, cin, cout, kind, key):
    rng = _rng("hw", P, cin, cout, kind, key)
    c = NS(P=P, cin=cin, cout=cout, kind=kind, row="P%d_ci%d_co%d" % (P, cin, cout))
    x = _draw(rng, (P, cin), kind, grid=True)
    dz = _draw(rng, (P, cout), kind)
    mt, tps, sp = _hw_plan(P)
    nbytes = L.call_size("ocr_conv1x1_small_wgrad_batch_slab_bytes", ctypes.c_int(P), ctypes.c_int(cin))
    assert nbytes == sp * cin * 32 * 4
    c.slab, c.dw = Guard((nbytes,), torch.uint8, device), Guard((cin, cout), torch.float32, device)
    c.xd, c.dzd = _dev(x, device), _d32(dz, device)
    dzr = _h(dz).astype(f64)
    c.ref, c.S = x.astype(f64).T @ dzr, np.abs(x).astype(f64).T @ np.abs(dzr)
    c.m = 64 * tps + _cdiv(sp, 64) + 6
    return c


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_head_wgrad(device, count, kind):
    L, ops = _lib()
    assert [_hw_plan(P) for P in (2049, 4161)] == [(33, 17, 2), (66, 22, 3)]      # 17 + 16 and 22 + 22 + 21 tiles
    rows = [HW_ROWS[(count + i) % 5] for i in range(count)] if count > 1 else HW_ROWS
    for lo in range(0, len(rows), count):
        cs = [_hw_case(L, device, *r, kind, count) for r in rows[lo:lo + count]]
        if len(cs) < count:
            break
        arr = _items(ops.HeadWgradItem, [(c.xd, c.dzd, c.dw, c.slab, c.P, c.cin, c.cout) for c in cs])
        assert _rc(L, "ocr_conv1x1_small_wgrad_batch_f16", arr, count) == OK
        torch.cuda.synchronize()
        for i, c in enumerate(cs):
            assert c.slab.ok()
            _c32("conv1x1_small_wgrad_batch", "n%d_i%d_%s" % (count, i, c.row), c.dw.np(), c.ref, c.m, c.S, kind)


def test_head_wgrad_capped(device):
    """P = 524 800, cin = 128: 8200 tiles, the cap of 256 splits gives 33 tiles per split and 249 launched splits (the
    last one 16 tiles).  x is dyadic (k / 8, drawn as bytes), dz random; the reference is formed in chunks."""
    L, ops = _lib()
    P, cin, cout = 524800, 128, 18
    assert _hw_plan(P) == (8200, 33, 249)
    nbytes = L.call_size("ocr_conv1x1_small_wgrad_batch_slab_bytes", ctypes.c_int(P), ctypes.c_int(cin))
    assert nbytes == 249 * cin * 32 * 4
    rng = _rng("hw_cap")
    xi = rng.integers(-32, 33, (P, cin), dtype=np.int8)
    dz = rng.standard_normal((P, cout)).astype(f32)
    xd = (torch.from_numpy(xi).to(device).float() / 8).to(O.STORAGE)
    slab, dw = Guard((nbytes,), torch.uint8, device), Guard((cin, cout), torch.float32, device)
    arr = _items(ops.HeadWgradItem, [(xd, _d32(dz, device), dw, slab, P, cin, cout)])
    assert _rc(L, "ocr_conv1x1_small_wgrad_batch_f16", arr, 1) == OK
    dzr = _h(dz)
    ref, S = np.zeros((cin, cout)), np.zeros((cin, cout))
    for p0 in range(0, P, 32768):
        xs, ds = xi[p0:p0 + 32768].astype(f64) / 8, dzr[p0:p0 + 32768].astype(f64)
        ref += xs.T @ ds
        S += np.abs(xs).T @ np.abs(ds)
    torch.cuda.synchronize()
    assert slab.ok()
    _c32("conv1x1_small_wgrad_batch", "capped", dw.np(), ref, 64 * 33 + 4 + 6, S, "random")
    # 32-bit buffer offsets: P * cin * 2 >= 2^31 is refused before anything is touched
    dw2 = Guard((cin, cout), torch.float32, device)
    arr = _items(ops.HeadWgradItem, [(xd, xd, dw2, slab, 1 << 23, cin, cout)])
    assert _rc(L, "ocr_conv1x1_small_wgrad_batch_f16", arr, 1) == UNSUPPORTED
    torch.cuda.synchronize()
    assert dw2.untouched()


# ------------------------------------------------------------------------------------------------ sc_fuse / unpool
MAPS = [(1, 2, 2), (2, 2, 6), (1, 6, 2), (3, 4, 10)]


def _u1(l):
    """legacy bilinear x2 in one dimension: out[2i] = in[i], out[2i+1] = (in[i] + in[min(i+1, l-1)]) / 2"""
    U = np.zeros((2 * l, l))
    for i in range(l):
        U[2 * i, i] += 1.0
        U[2 * i + 1, i] += 0.5
        U[2 * i + 1, min(i + 1, l - 1)] += 0.5
    return U


def _along(U, a, axis):
    """U applied along one axis of a"""
    return np.moveaxis(np.tensordot(U, a, axes=(1, axis)), 0, axis)


def _unpool(prev):
    n, lh, lw, C = prev.shape
    return _along(_u1(lw), _along(_u1(lh), prev.astype(f64), 1), 2)


def _unpool_t(g):
    n, H, W, C = g.shape
    return _along(_u1(W // 2).T, _along(_u1(H // 2).T, g.astype(f64), 1), 2)


def _act_ref(z, sc, sh, relu):
    """(value, sum of |terms|, fragile) of act(z * sc + sh) with the f32 sign decided fused and unfused"""
    z, sc, sh = z.astype(f64), sc.astype(f64), sh.astype(f64)
    v = z * sc + sh
    fused = v.astype(f32)
    unf = ((z * sc).astype(f32).astype(f64) + sh).astype(f32)
    frag = ((fused < 0) != (unf < 0)) if relu else np.zeros(v.shape, bool)
    if relu:
        v = np.where(fused < 0, 0.0, v)
    return v, np.abs(z * sc) + np.abs(sh), frag


def _fragile_ok(frag, kind):
    share = float(frag.mean()) if frag.size else 0.0
    assert share <= 1e-3, share
    if kind == "exact":
        assert not frag.any()


def _fuse(L, device, n, h, w, C, use, aff, relu, kind, row):
    rng = _rng("fuse", n, h, w, C, use, aff, relu, kind)
    shape = (n, h, w, C)
    ref, S, frag = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
    args = []
    for k, name in enumerate("ab"):
        if name not in use:
            args += [None, None, None]
            continue
        z = _draw(rng, shape, kind)
        if aff[k]:
            sc, sh = _pow2(rng, C, kind), (_draw(rng, C, kind) * f32(0.5)).astype(f32)
            v, s, fr = _act_ref(z, sc, sh, relu)
            args += [_d32(z, device), _d32(sc, device), _d32(sh, device)]
        else:
            v, s, fr = z.astype(f64), np.abs(z).astype(f64), np.zeros(shape, bool)
            args += [_d32(z, device), None, None]
        ref, S, frag = ref + v, S + s, frag | fr
    if "p" in use:
        prev = _draw(rng, (n, h // 2, w // 2, C), kind)
        ref, S = ref + _unpool(prev), S + _unpool(np.abs(prev))
        args.append(_d32(prev, device))
    else:
        args.append(None)
    _fragile_ok(frag, kind)
    out = Guard(shape, torch.float32, device)
    assert _rc(L, "ocr_sc_fuse", *args, n, h, w, C, relu, out) == OK
    torch.cuda.synchronize()
    _c32("sc_fuse", row, out.np(), ref, 8, S, kind, frag)


SUBSETS = ["a", "b", "p", "ab", "ap", "bp", "abp"]


@pytest.mark.parametrize("n,h,w", MAPS, ids=["%dx%dx%d" % m for m in MAPS])
@pytest.mark.parametrize("C", [1, 18])
@pytest.mark.parametrize("kind", KINDS)
def test_fuse(device, n, h, w, C, kind):
    L, ops = _lib()
    for use in SUBSETS:
        affs = [(x, y) for x in ((0, 1) if "a" in use else (0,)) for y in ((0, 1) if "b" in use else (0,))]
        for aff in affs:
            for relu in ((0, 1) if any(aff) else (0,)):
                _fuse(L, device, n, h, w, C, use, aff, relu, kind, "%dx%dx%d_C%d_%s_aff%d%d_relu%d" % (n, h, w, C, use, *aff, relu))
    # odd h or w with prev
    t = torch.zeros(64, dtype=torch.float32, device=device)
    out = Guard((64,), torch.float32, device)
    for hh, ww in ((3, 2), (2, 3)):
        assert _rc(L, "ocr_sc_fuse", None, None, None, None, None, None, t, 1, hh, ww, 1, 0, out) == INVALID_ARG
    torch.cuda.synchronize()
    assert out.untouched()


@pytest.mark.parametrize("n,h,w", MAPS, ids=["%dx%dx%d" % m for m in MAPS])
@pytest.mark.parametrize("C", [1, 18])
@pytest.mark.parametrize("kind", KINDS)
def test_unpool_bwd(device, n, h, w, C, kind):
    """ocr_sc_unpool_bwd against the float64 transpose of the explicitly built (2lh 2lw) x (lh lw) interpolation matrix,
    and <unpool(x), g> = <x, unpool_bwd(g)> exactly on dyadic data (both sides from the device)"""
    L, ops = _lib()
    lh, lw = h // 2, w // 2
    rng = _rng("unpool_bwd", n, h, w, C, kind)
    U = np.kron(_u1(lh), _u1(lw))                                       # row (oy, ox) <- column (y, x)
    assert U.shape == (h * w, lh * lw) and np.array_equal(U.sum(1), np.ones(h * w))
    g = _draw(rng, (n, h, w, C), kind)
    ref = np.einsum("oi,noc->nic", U, g.reshape(n, h * w, C).astype(f64)).reshape(n, lh, lw, C)
    S = np.einsum("oi,noc->nic", U, np.abs(g).reshape(n, h * w, C).astype(f64)).reshape(n, lh, lw, C)
    assert np.allclose(ref, _unpool_t(g), rtol=0, atol=1e-12)
    gd = _d32(g, device)
    dprev = Guard((n, lh, lw, C), torch.float32, device)
    assert _rc(L, "ocr_sc_unpool_bwd", gd, n, lh, lw, C, dprev) == OK
    torch.cuda.synchronize()
    row = "%dx%dx%d_C%d" % (n, h, w, C)
    _c32("sc_unpool_bwd", row, dprev.np(), ref, 9, S, kind)
    if kind == "exact":
        x = _draw(rng, (n, lh, lw, C), kind)
        up = Guard((n, h, w, C), torch.float32, device)
        assert _rc(L, "ocr_sc_fuse", None, None, None, None, None, None, _d32(x, device), n, h, w, C, 0, up) == OK
        torch.cuda.synchronize()
        lhs = float((up.np().astype(f64) * g.astype(f64)).sum())
        rhs = float((x.astype(f64) * dprev.np().astype(f64)).sum())
        assert lhs == rhs, (lhs, rhs)


def test_fuse_cap(device):
    """above the 4096-block cap: sc_fuse on (1, 244, 244) at C = 18 (1 071 648 elements), sc_unpool_bwd onto a low map
    of that size; both grid-stride loops take a second pass"""
    L, ops = _lib()
    assert 244 * 244 * 18 > 4096 * 256
    _fuse(L, device, 1, 244, 244, 18, "abp", (1, 0), 1, "random", "cap")
    rng = _rng("unpool_cap")
    g = rng.standard_normal((1, 488, 488, 18)).astype(f32)
    dprev = Guard((1, 244, 244, 18), torch.float32, device)
    assert _rc(L, "ocr_sc_unpool_bwd", _d32(g, device), 1, 244, 244, 18, dprev) == OK
    torch.cuda.synchronize()
    _c32("sc_unpool_bwd", "cap", dprev.np(), _unpool_t(g), 9, _unpool_t(np.abs(g)), "random")


# ------------------------------------------------------------------------------------------------ sc statistics / BN backward
SC_C = [1, 2, 16, 18, 100, 128]


def _sc_T(P, C):
    lanes = 256 // C
    return max(min(_cdiv(P, lanes * 8), 1024), 1), lanes


def _block_sums(v, T, lanes):
    """[T][C] sums of v [P][C] the way the grid deals pixels: pixel p -> block (p // lanes) % T"""
    out = np.zeros((T, v.shape[1]))
    np.add.at(out, (np.arange(v.shape[0]) // lanes) % T, v)
    return out


def _sc_stats(L, ops, device, P, C, kind):
    T, lanes = _sc_T(P, C)
    assert int(L._fn("ocr_sc_num_partials", ctypes.c_int)(ctypes.c_int(P), ctypes.c_int(C))) == T
    n_it = _cdiv(P, T * lanes)
    row = "P%d_C%d" % (P, C)
    rng = _rng("sc_stats", P, C, kind)
    x = _draw(rng, (P, C), kind)
    xd, x64 = _d32(x, device), x.astype(f64)
    part = Guard((T, 2, C), torch.float32, device)
    assert _rc(L, "ocr_sc_stats", xd, P, C, part) == OK
    torch.cuda.synchronize()
    p = part.np()
    _c32("sc_stats", row + "_sum", p[:, 0], _block_sums(x64, T, lanes), n_it + lanes, _block_sums(np.abs(x64), T, lanes), kind)
    _c32("sc_stats", row + "_sq", p[:, 1], _block_sums(x64 ** 2, T, lanes), 2 * n_it + lanes, _block_sums(x64 ** 2, T, lanes), kind)
    # column sums: the documented (T + 1) * 2 * C floats of partial; the last row is not used by the per-map entry
    part = Guard((T + 1, 2, C), torch.float32, device)
    out = Guard((C,), torch.float32, device)
    assert _rc(L, "ocr_sc_colsum", xd, P, C, out, part) == OK
    torch.cuda.synchronize()
    assert np.isnan(part.raw()[T]).all() and not np.isnan(part.raw()[:T]).any()
    _c32("sc_colsum", row, out.np(), x64.sum(0), n_it + lanes + _cdiv(T, 64) + 6, np.abs(x64).sum(0), kind)
    part = Guard((T + 1, 2, C), torch.float32, device)
    out = Guard((C,), torch.float32, device)
    arr = _items(ops.ScColsumItem, [(xd, out, part, P, C)])
    rc = _rc(L, "ocr_sc_colsum_batch", arr, 1)
    torch.cuda.synchronize()
    if C > 32:
        assert rc == UNSUPPORTED and out.untouched() and part.untouched()
        return
    assert rc == OK
    _c32("sc_colsum_batch", row, out.np(), x64.sum(0), n_it + lanes + 1, np.abs(x64).sum(0), kind)
    assert part.ok()


@pytest.mark.parametrize("C", SC_C)
@pytest.mark.parametrize("kind", KINDS)
def test_sc_stats(device, C, kind):
    L, ops = _lib()
    lanes = 256 // C
    for P in (1, lanes * 8 - 1, lanes * 8 + 1):
        _sc_stats(L, ops, device, P, C, kind)
    if C <= 32:                                         # four maps in one launch
        rng = _rng("colsum4", C, kind)
        its = []
        for P in (lanes * 8 + 1, 1, 3 * lanes * 8 + 5, 7):
            x = _draw(rng, (P, C), kind)
            T, _ = _sc_T(P, C)
            its.append((x, _d32(x, device), Guard((C,), torch.float32, device), Guard((T + 1, 2, C), torch.float32, device), P, T))
        arr = _items(ops.ScColsumItem, [(xd, o, pt, P, C) for _, xd, o, pt, P, _ in its])
        assert _rc(L, "ocr_sc_colsum_batch", arr, 4) == OK
        torch.cuda.synchronize()
        for i, (x, _, o, pt, P, T) in enumerate(its):
            assert pt.ok()
            _c32("sc_colsum_batch", "n4_i%d_P%d_C%d" % (i, P, C), o.np(), x.astype(f64).sum(0), _cdiv(P, T * lanes) + lanes + 1,
                 np.abs(x).astype(f64).sum(0), kind)


def _bn_case(device, P, C, relu, kind):
    rng = _rng("sc_bn", P, C, relu, kind)
    c = NS(P=P, C=C, relu=relu, kind=kind)
    if kind == "exact":                                 # mean an integer, invstd 1: (z - mean) * invstd * dgamma / P stays exact
        c.z = (rng.integers(-16, 17, (P, C)) / 8.0).astype(f32)
        c.dout = (rng.integers(-16, 17, (P, C)) / 8.0).astype(f32)
        c.sc, c.sh = _pow2(rng, C, kind), (rng.integers(-4, 5, C) / 4.0).astype(f32)
        c.mu, c.inv = rng.integers(-1, 2, C).astype(f32), np.ones(C, f32)
    else:
        c.z, c.dout = _draw(rng, (P, C), kind), _draw(rng, (P, C), kind)
        c.sc, c.sh = _pow2(rng, C, kind), (rng.standard_normal(C) * 0.5).astype(f32)
        c.mu, c.inv = (rng.standard_normal(C) * 0.3).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    a, _, c.frag = _act_ref(c.z, c.sc, c.sh, relu)
    fused = (c.z.astype(f64) * c.sc + c.sh.astype(f64)).astype(f32)
    c.g = np.where(fused > 0, c.dout, f32(0)).astype(f64) if relu else c.dout.astype(f64)
    if relu:
        unf = ((c.z.astype(f64) * c.sc).astype(f32).astype(f64) + c.sh).astype(f32)
        c.frag = (fused > 0) != (unf > 0)
    _fragile_ok(c.frag, kind)
    c.okc = ~c.frag.any(0)
    assert c.okc.mean() >= 0.75
    c.xh = (c.z.astype(f64) - c.mu) * c.inv
    c.dev = [_d32(v, device) for v in (c.z, c.sc, c.sh, c.mu, c.inv, c.dout)]
    return c


def _check_bn(entry, row, c, dgamma, dbeta, dz, batch):
    T, lanes = _sc_T(c.P, c.C)
    n_it = _cdiv(c.P, T * lanes)
    red = 1 if batch else _cdiv(T, 64) + 6
    skipc = ~c.okc
    _c32(entry, row + "_dbeta", dbeta, c.g.sum(0), n_it + lanes + red, np.abs(c.g).sum(0), c.kind, skipc)
    _c32(entry, row + "_dgamma", dgamma, (c.g * c.xh).sum(0), n_it + lanes + red + 3, np.abs(c.g * c.xh).sum(0), c.kind, skipc)
    sc = c.sc.astype(f64)
    kd, kx = dbeta.astype(f64) / c.P, dgamma.astype(f64) / c.P                  # (referred to what the device wrote)
    ref = sc * (c.g - kd - c.xh * kx)
    S = np.abs(sc) * (np.abs(c.g) + np.abs(kd) + np.abs(c.xh * kx))
    _c32(entry, row + "_dz", dz, ref, 8, S, c.kind, c.frag)


def _sc_bn(L, ops, device, shapes, relu, kind, tag):
    cs = [_bn_case(device, P, C, relu, kind) for P, C in shapes]
    for c in cs:
        T, _ = _sc_T(c.P, c.C)
        o = [Guard((c.C,), torch.float32, device), Guard((c.C,), torch.float32, device), Guard((c.P, c.C), torch.float32, device)]
        part = Guard((T + 1, 2, c.C), torch.float32, device)                    # documented: (T + 1) * 2 * C floats
        assert _rc(L, "ocr_sc_bn_bwd", *c.dev, c.P, c.C, relu, o[0], o[1], o[2], part) == OK
        torch.cuda.synchronize()
        assert np.isnan(part.raw()[T]).all() and not np.isnan(part.raw()[:T]).any()
        _check_bn("sc_bn_bwd", "%sP%d_C%d_relu%d" % (tag, c.P, c.C, relu), c, o[0].np(), o[1].np(), o[2].np(), False)
    small = [c for c in cs if c.C <= 32]
    big = [c for c in cs if c.C > 32]
    for c in big:
        o = [Guard((c.C,), torch.float32, device) for _ in range(2)] + [Guard((c.P, c.C), torch.float32, device)]
        part = Guard((_sc_T(c.P, c.C)[0], 2, c.C), torch.float32, device)
        arr = _items(ops.ScBnBwdItem, [(*c.dev, o[0], o[1], o[2], part, c.P, c.C, relu)])
        assert _rc(L, "ocr_sc_bn_bwd_batch", arr, 1) == UNSUPPORTED
        torch.cuda.synchronize()
        assert all(v.untouched() for v in o) and part.untouched()
    if small:
        outs = []
        for c in small:
            T, _ = _sc_T(c.P, c.C)                                              # documented: T * 2 * C floats
            outs.append([Guard((c.C,), torch.float32, device), Guard((c.C,), torch.float32, device),
                         Guard((c.P, c.C), torch.float32, device), Guard((T, 2, c.C), torch.float32, device)])
        arr = _items(ops.ScBnBwdItem, [(*c.dev, o[0], o[1], o[2], o[3], c.P, c.C, relu) for c, o in zip(small, outs)])
        assert _rc(L, "ocr_sc_bn_bwd_batch", arr, len(small)) == OK
        torch.cuda.synchronize()
        for i, (c, o) in enumerate(zip(small, outs)):
            assert o[3].ok()
            _check_bn("sc_bn_bwd_batch", "%sn%d_i%d_P%d_C%d_relu%d" % (tag, len(small), i, c.P, c.C, relu), c, o[0].np(), o[1].np(), o[2].np(), True)


@pytest.mark.parametrize("C", SC_C)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_sc_bn_bwd(device, C, relu, kind):
    L, ops = _lib()
    lanes = 256 // C
    if kind == "exact":                                 # 1 / P must be exact: powers of two
        shapes = [(1, C), (64, C), (256, C)]
    else:
        shapes = [(1, C), (lanes * 8 - 1, C), (lanes * 8 + 1, C)]
    _sc_bn(L, ops, device, shapes, relu, kind, "")


def test_sc_block_cap(device):
    """P = 114 703 at C = 18: ceil(P / 112) = 1025 > the cap of 1024 blocks, every block's lanes take a second pixel"""
    L, ops = _lib()
    P, C = 114703, 18
    assert _sc_T(P, C) == (1024, 14) and _cdiv(P, 14 * 8) == 1025
    _sc_stats(L, ops, device, P, C, "random")
    _sc_bn(L, ops, device, [(P, C)], 1, "random", "cap_")


# ------------------------------------------------------------------------------------------------ pointwise
PW_SHAPES = [(2, 2), (16, 16), (3, 5), (18, 7), (32, 15)]


def _pw_wgrad_m(cin, cout, P):
    return 2 * _cdiv(P, 256) + 32


@pytest.mark.parametrize("cin,cout", PW_SHAPES, ids=["%dto%d" % s for s in PW_SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_pointwise(device, cin, cout, kind):
    L, ops = _lib()
    nbytes = L.call_size("ocr_sc_pointwise_wgrad_workspace", ctypes.c_int(cin), ctypes.c_int(cout))
    assert nbytes == 257 * (cin * cout + cout) * 4
    for j, P in enumerate((1, 255, 257, 1025)):
        strided = j != 1                                                        # P = 255: contiguous, ld = channel count
        xo, ldx = (3, 3 + cin + 2) if strided else (0, cin)
        oo, ldo = (1, 1 + cout + 3) if strided else (0, cout)
        bias = j % 2 == 0
        row = "%dto%d_P%d_%s" % (cin, cout, P, "strided" if strided else "dense")
        rng = _rng("pw", cin, cout, P, kind)
        x, w, d = _draw(rng, (P, cin), kind), _draw(rng, (cin, cout), kind, 0.5), _draw(rng, (P, cout), kind)
        b = _draw(rng, (cout,), kind)
        x64, w64, d64 = x.astype(f64), w.astype(f64), d.astype(f64)
        xs, ds = Strided(P, ldx, xo, cin, device, x), Strided(P, ldo, oo, cout, device, d)
        wd, bd = _d32(w, device), _d32(b, device) if bias else None
        out = Strided(P, ldo, oo, cout, device)
        assert _rc(L, "ocr_sc_pointwise_fwd", xs, ldx, xo, cin, wd, bd, P, out, ldo, oo, cout) == OK
        dx = Strided(P, ldx, xo, cin, device)
        assert _rc(L, "ocr_sc_pointwise_dgrad", ds, ldo, oo, cout, wd, P, dx, ldx, xo, cin) == OK
        ws = Guard((nbytes,), torch.uint8, device)
        dw, db = Guard((cin, cout), torch.float32, device), Guard((cout,), torch.float32, device) if bias else None
        assert _rc(L, "ocr_sc_pointwise_wgrad", xs, ldx, xo, cin, ds, ldo, oo, cout, P, dw, db, ws, SZ(nbytes - 1)) == WORKSPACE
        torch.cuda.synchronize()
        assert dw.untouched() and ws.untouched()
        assert _rc(L, "ocr_sc_pointwise_wgrad", xs, ldx, xo, cin, ds, ldo, oo, cout, P, dw, db, ws, SZ(nbytes)) == OK
        torch.cuda.synchronize()
        assert ws.ok()
        _c32("sc_pointwise_fwd", row, out.np(), x64 @ w64 + (b.astype(f64) if bias else 0.0), 2 * cin,
             np.abs(x64) @ np.abs(w64) + (np.abs(b).astype(f64) if bias else 0.0), kind)
        _c32("sc_pointwise_dgrad", row, dx.np(), d64 @ w64.T, 2 * cout, np.abs(d64) @ np.abs(w64).T, kind)
        m = _pw_wgrad_m(cin, cout, P)
        _c32("sc_pointwise_wgrad", row, dw.np(), x64.T @ d64, m, np.abs(x64).T @ np.abs(d64), kind)
        if bias:
            _c32("sc_pointwise_wgrad", row + "_db", db.np(), d64.sum(0), m, np.abs(d64).sum(0), kind)
        for s in (xs, ds):
            s.np()                                                              # the inputs came back whole


# ------------------------------------------------------------------------------------------------ predication pair
def _pair(L, device, P, kind, stats, bias, row):
    rng = _rng("pair", P, kind, stats, bias)
    x = _draw(rng, (P, 18), kind)
    if kind == "exact":                                 # +-0.5 twice per output: the squares of the outputs stay exact in f32
        w = [(np.sign(_conv_w(rng, c, c, kind)) * 0.5).astype(f32) for c in (2, 16)]
    else:
        w = [_draw(rng, (2, 2), kind, 0.5), _draw(rng, (16, 16), kind, 0.5)]
    b = [_draw(rng, (2,), kind), _draw(rng, (16,), kind)] if bias else [None, None]
    T = int(L._fn("ocr_sc_pointwise_pair_num_partials", ctypes.c_int)(ctypes.c_int(P)))
    assert T == max(min(_cdiv(P, 1024), 1024), 1)
    xd, wd = _d32(x, device), [_d32(v, device) for v in w]
    bd = [_d32(v, device) if bias else None for v in b]
    z = [Guard((P, 2), torch.float32, device), Guard((P, 16), torch.float32, device)]
    pt = [Guard((T, 2, 2), torch.float32, device), Guard((T, 2, 16), torch.float32, device)] if stats else [None, None]
    assert _rc(L, "ocr_sc_pointwise_pair_fwd", xd, wd[0], bd[0], wd[1], bd[1], P, z[0], z[1], pt[0], pt[1]) == OK
    torch.cuda.synchronize()
    x64 = x.astype(f64)
    sl = [slice(0, 2), slice(2, 18)]
    blk = (np.arange(P) // 256) % T
    n_it = _cdiv(P, T * 256)
    for k, name in enumerate(("px", "lk")):
        C = 2 if k == 0 else 16
        w64 = w[k].astype(f64)
        ref = x64[:, sl[k]] @ w64 + (b[k].astype(f64) if bias else 0.0)
        S = np.abs(x64[:, sl[k]]) @ np.abs(w64) + (np.abs(b[k]).astype(f64) if bias else 0.0)
        _c32("sc_pointwise_pair_fwd", row + "_" + name, z[k].np(), ref, 2 * C, S, kind)
        if stats:
            bz = (_g(2 * C) * S if kind != "exact" else 0.0 * S) + 2.0 ** -149
            s, q, ss, bs, bq = (np.zeros((T, C)) for _ in range(5))
            for acc, v in ((s, ref), (q, ref ** 2), (ss, np.abs(ref)), (bs, bz), (bq, 2 * np.abs(ref) * bz + bz ** 2)):
                np.add.at(acc, blk, v)
            p = pt[k].np()
            if kind == "exact":
                _bits_equal(p[:, 0], _exact32(s), "pair sums")
                _bits_equal(p[:, 1], _exact32(q), "pair squares")
            else:
                _note("sc_pointwise_pair_fwd_stats", row + "_" + name,
                      max(_ratio(np.abs(p[:, 0] - s), bs + _g(n_it + 9) * ss), _ratio(np.abs(p[:, 1] - q), bq + _g(2 * n_it + 9) * q)))
    # backward
    dz = [_draw(rng, (P, 2), kind), _draw(rng, (P, 16), kind)]
    dzd = [_d32(v, device) for v in dz]
    nbytes = L.call_size("ocr_sc_pointwise_pair_bwd_workspace")
    assert nbytes == 256 * (16 * 16 + 16 + 6) * 4
    ws = Guard((nbytes,), torch.uint8, device)
    dx = Guard((P, 18), torch.float32, device)
    dw = [Guard((2, 2), torch.float32, device), Guard((16, 16), torch.float32, device)]
    db = [Guard((2,), torch.float32, device), Guard((16,), torch.float32, device)] if bias else [None, None]
    a = (xd, dzd[0], dzd[1], wd[0], wd[1], P, dx, dw[0], db[0], dw[1], db[1], ws)
    assert _rc(L, "ocr_sc_pointwise_pair_bwd", *a, SZ(nbytes - 1)) == WORKSPACE
    torch.cuda.synchronize()
    assert dx.untouched() and ws.untouched()
    assert _rc(L, "ocr_sc_pointwise_pair_bwd", *a, SZ(nbytes)) == OK
    torch.cuda.synchronize()
    assert ws.ok()
    dxv = dx.np()
    m = 2 * _cdiv(P, 256) + 32
    for k, name in enumerate(("px", "lk")):
        C = 2 if k == 0 else 16
        d64, w64 = dz[k].astype(f64), w[k].astype(f64)
        _c32("sc_pointwise_pair_bwd", row + "_dx_" + name, dxv[:, sl[k]], d64 @ w64.T, 2 * C, np.abs(d64) @ np.abs(w64).T, kind)
        _c32("sc_pointwise_pair_bwd", row + "_dw_" + name, dw[k].np(), x64[:, sl[k]].T @ d64, m, np.abs(x64[:, sl[k]]).T @ np.abs(d64), kind)
        if bias:
            _c32("sc_pointwise_pair_bwd", row + "_db_" + name, db[k].np(), d64.sum(0), m, np.abs(d64).sum(0), kind)


@pytest.mark.parametrize("P", [1, 1023, 1025])
@pytest.mark.parametrize("kind", KINDS)
def test_pair(device, P, kind):
    L, ops = _lib()
    _pair(L, device, P, kind, True, True, "P%d" % P)
    _pair(L, device, P, kind, False, False, "P%d_nostats" % P)
    t = torch.zeros((P, 18), dtype=torch.float32, device=device)
    z = [Guard((P, 2), torch.float32, device), Guard((P, 16), torch.float32, device)]
    pt = Guard((4, 2, 16), torch.float32, device)
    assert _rc(L, "ocr_sc_pointwise_pair_fwd", t, t, None, t, None, P, z[0], z[1], pt, None) == INVALID_ARG
    assert _rc(L, "ocr_sc_pointwise_pair_fwd", t, t, None, t, None, P, z[0], z[1], None, pt) == INVALID_ARG
    torch.cuda.synchronize()
    assert z[0].untouched() and z[1].untouched() and pt.untouched()


def test_pair_cap(device):
    """above 1024 * 1024 pixels: 1024 partial rows with a second pixel per thread, the input gradient's 4096 blocks too"""
    L, ops = _lib()
    P = 1024 * 1024 + 300
    assert _cdiv(P, 1024) > 1024 and _cdiv(P, 256) > 4096
    _pair(L, device, P, "random", True, True, "cap")


# ------------------------------------------------------------------------------------------------ sigmoid heads, act
def _sig_grid(rng, n, kind):
    edge = np.array([0.0, -0.0, 88.0, -88.0, 104.0, -104.0], f32)
    if kind == "exact":
        return np.resize(np.array([0.0, -0.0, 104.0, -104.0], f32), n)
    body = np.concatenate([edge, np.linspace(-20, 20, 41).astype(f32), (rng.standard_normal(max(n, 64)) * 4).astype(f32)])
    return np.resize(body, n) if n > 1 else edge[2:3]


def _sig64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z.astype(f64)))


def _sig_ref(z, kind):
    """exact rows: 0 -> 0.5, 104 -> 1, -104 -> 0 (exp overflows to inf; the float64 value 6.8e-46 rounds to zero in f32)"""
    return _sig64(z).astype(f32).astype(f64) if kind == "exact" else _sig64(z)


@pytest.mark.parametrize("kind", KINDS)
def test_sigmoid_act(device, kind):
    L, ops = _lib()
    rng = _rng("sigmoid", kind)
    for n in (1, 257):
        z = _sig_grid(rng, n, kind)
        zd = _d32(z, device)
        out = Guard((n,), torch.float32, device)
        assert _rc(L, "ocr_sc_sigmoid", zd, I64(n), out) == OK
        torch.cuda.synchronize()
        s = out.np()
        _c32("sc_sigmoid", "n%d" % n, s, _sig_ref(z, kind), 4, _sig64(z), kind)
        sv = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], n).astype(f32) if kind == "exact" else s
        d = _draw(rng, (n,), kind)
        dz = Guard((n,), torch.float32, device)
        assert _rc(L, "ocr_sc_sigmoid_bwd", _d32(sv, device), _d32(d, device), I64(n), dz) == OK
        torch.cuda.synchronize()
        ref = d.astype(f64) * sv.astype(f64) * (1.0 - sv.astype(f64))
        _c32("sc_sigmoid_bwd", "n%d" % n, dz.np(), ref, 3, np.abs(ref), kind)
    C = 9
    for P in (1, 257):
        for c0 in (1, C - 1):
            row = "P%d_c0_%d" % (P, c0)
            z = _sig_grid(rng, P * C, kind).reshape(P, C)
            o = [Guard((P, c0), torch.float32, device), Guard((P, C - c0), torch.float32, device)]
            assert _rc(L, "ocr_sc_sigmoid_split", _d32(z, device), P, C, c0, o[0], o[1]) == OK
            torch.cuda.synchronize()
            s = np.concatenate([o[0].np(), o[1].np()], 1)
            _c32("sc_sigmoid_split", row, s, _sig_ref(z, kind), 4, _sig64(z), kind)
            sv = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], (P, C)).astype(f32) if kind == "exact" else s
            d = _draw(rng, (P, C), kind)
            sd = [_d32(sv[:, :c0], device), _d32(sv[:, c0:], device)]
            dd = [_d32(d[:, :c0], device), _d32(d[:, c0:], device)]
            for null in (None, 0, 1):
                dn = [None if null == k else dd[k] for k in range(2)]
                d64 = d.astype(f64).copy()
                if null == 0:
                    d64[:, :c0] = 0
                if null == 1:
                    d64[:, c0:] = 0
                dz = Guard((P, C), torch.float32, device)
                assert _rc(L, "ocr_sc_sigmoid_split_bwd", sd[0], dn[0], sd[1], dn[1], P, C, c0, dz) == OK
                torch.cuda.synchronize()
                ref = d64 * sv.astype(f64) * (1.0 - sv.astype(f64))
                _c32("sc_sigmoid_split_bwd", "%s_null%s" % (row, null), dz.np(), ref, 3, np.abs(ref), kind)
    # act(z * scale + shift), up to four tensors per launch
    for count in (1, 2, 3, 4):
        for relu in (0, 1):
            its = []
            for P, C in [(257, 2), (33, 16), (1, 18), (1025, 7)][:count]:
                z, sc, sh = _draw(rng, (P, C), kind), _pow2(rng, C, kind), (_draw(rng, C, kind) * f32(0.5)).astype(f32)
                its.append((z, sc, sh, Guard((P, C), torch.float32, device), [_d32(v, device) for v in (z, sc, sh)], P, C))
            arr = _items(ops.ScActItem, [(dv[0], dv[1], dv[2], o, P * C, C) for _, _, _, o, dv, P, C in its])
            assert _rc(L, "ocr_sc_act_batch", arr, count, relu) == OK
            torch.cuda.synchronize()
            for i, (z, sc, sh, o, _, P, C) in enumerate(its):
                ref, S, frag = _act_ref(z, sc, sh, relu)
                _fragile_ok(frag, kind)
                _c32("sc_act_batch", "n%d_i%d_relu%d" % (count, i, relu), o.np(), ref, 2, S, kind, frag)


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes(device):
    """Every OCR_CHECK_ARG / OCR_CHECK_SHAPE of the file: NULL required pointers and non-positive extents answer
    OCR_ERR_INVALID_ARG, unsupported channel counts OCR_ERR_UNSUPPORTED, count 0 and 5 of the batched forms
    OCR_ERR_INVALID_ARG.  No refused call launches: every output buffer is untouched afterwards."""
    L, ops = _lib()
    P, cin, C = 64, 128, 18
    h16 = torch.zeros((P, cin), dtype=O.STORAGE, device=device)
    t32 = torch.zeros((P, 32), dtype=torch.float32, device=device)
    v = torch.ones(128, dtype=torch.float32, device=device)
    G = {k: Guard(s, d, device) for k, (s, d) in {
        "o32": ((P, 32), torch.float32), "o16": ((P, cin), O.STORAGE), "dw": ((cin, 32), torch.float32),
        "v0": ((128,), torch.float32), "v1": ((128,), torch.float32), "part": ((64, 2, 128), torch.float32),
        "ws": ((1 << 20,), torch.uint8), "o32b": ((P, 32), torch.float32)}.items()}
    nb = SZ(1 << 20)
    # entry: (arguments, required pointers, (index, bad values -> INVALID_ARG), (index, bad values -> UNSUPPORTED))
    E = {
        "ocr_conv1x1_small_f16": ([h16, h16, None, P, cin, C, G["o32"]], [0, 1, 6], [(3, (0, -1))], [(4, (0, 8, 24)), (5, (0, 33))]),
        "ocr_conv1x1_small_dgrad_f16": ([t32, h16, P, cin, C, FL(1.0), G["o16"], 0], [0, 1, 6], [(2, (0, -1))], [(3, (0, 16, 48)), (4, (0, 33))]),
        "ocr_conv1x1_small_wgrad_f16": ([h16, t32, P, cin, C, G["dw"], G["ws"], nb], [0, 1, 5, 6], [(2, (0, -1))], [(3, (0, -8)), (4, (0, 33))]),
        "ocr_sc_stats": ([t32, P, C, G["part"]], [0, 3], [(1, (0, -1))], [(2, (0, 129))]),
        "ocr_sc_fuse": ([t32, v, v, t32, v, v, None, 1, 8, 8, C, 1, G["o32"]], [12], [(7, (0,)), (8, (0,)), (9, (0,)), (10, (0,))], []),
        "ocr_sc_unpool_bwd": ([t32, 1, 2, 2, C, G["o32"]], [0, 5], [(1, (0,)), (2, (0,)), (3, (0,)), (4, (0,))], []),
        "ocr_sc_bn_bwd": ([t32, v, v, v, v, t32, P, C, 1, G["v0"], G["v1"], G["o32"], G["part"]], [0, 1, 2, 3, 4, 5, 9, 10, 11, 12], [],
                          [(6, (0, -1)), (7, (0, 129))]),
        "ocr_sc_pointwise_fwd": ([t32, 40, 2, 16, v, None, P, G["o32"], 40, 0, 16], [0, 4, 7],
                                 [(6, (0,)), (3, (0,)), (10, (0,)), (1, (17,)), (2, (-1, 25)), (8, (15,)), (9, (-1, 25))], [(3, (33,)), (10, (33,))]),
        "ocr_sc_pointwise_dgrad": ([t32, 40, 0, 16, v, P, G["o32"], 40, 2, 16], [0, 4, 6],
                                   [(5, (0,)), (3, (0,)), (9, (0,)), (1, (15,)), (2, (-1, 25)), (7, (17,)), (8, (-1, 25))], [(3, (33,)), (9, (33,))]),
        "ocr_sc_pointwise_wgrad": ([t32, 40, 2, 16, t32, 40, 0, 16, P, G["dw"], G["v0"], G["ws"], nb], [0, 4, 9, 11],
                                   [(8, (0,)), (3, (0,)), (7, (0,)), (1, (17,)), (2, (-1, 25)), (5, (15,)), (6, (-1, 25))], [(3, (33,)), (7, (33,))]),
        "ocr_sc_colsum": ([t32, P, C, G["v0"], G["part"]], [0, 3, 4], [(1, (0, -1))], [(2, (0, 129))]),
        "ocr_sc_sigmoid_split": ([t32, P, 9, 1, G["o32"], G["o32b"]], [0, 4, 5], [(1, (0,)), (2, (1,)), (3, (0, 9))], []),
        "ocr_sc_sigmoid_split_bwd": ([t32, t32, t32, t32, P, 9, 1, G["o32"]], [0, 2, 7], [(4, (0,)), (5, (1,)), (6, (0, 9))], []),
        "ocr_sc_sigmoid": ([t32, I64(64), G["o32"]], [0, 2], [(1, (I64(0), I64(-1)))], []),
        "ocr_sc_sigmoid_bwd": ([t32, t32, I64(64), G["o32"]], [0, 1, 3], [(2, (I64(0),))], []),
        "ocr_sc_pointwise_pair_fwd": ([t32, v, None, v, None, P, G["o32"], G["o32b"], None, None], [0, 1, 3, 6, 7], [(5, (0, -1))], []),
        "ocr_sc_pointwise_pair_bwd": ([t32, t32, t32, v, v, P, G["o32"], G["v0"], None, G["dw"], None, G["ws"], nb], [0, 1, 2, 3, 4, 6, 7, 9, 11],
                                      [(5, (0, -1))], []),
    }
    for name, (args, req, inv, uns) in E.items():
        for j in req:
            a = list(args)
            a[j] = None
            assert _rc(L, name, *a) == INVALID_ARG, (name, j)
        for code, lst in ((INVALID_ARG, inv), (UNSUPPORTED, uns)):
            for j, bads in lst:
                for bad in bads:
                    a = list(args)
                    a[j] = bad
                    assert _rc(L, name, *a) == code, (name, j, bad)
    # scale without shift (and the reverse) in sc_fuse
    a = list(E["ocr_sc_fuse"][0])
    for j in (1, 2, 4, 5):
        b = list(a)
        b[j] = None
        assert _rc(L, "ocr_sc_fuse", *b) == INVALID_ARG
    for name in ("ocr_conv1x1_small_wgrad_f16", "ocr_sc_pointwise_wgrad", "ocr_sc_pointwise_pair_bwd"):
        a = list(E[name][0])
        a[-1] = SZ(7)
        assert _rc(L, name, *a) == WORKSPACE, name
    # the size queries
    ci = ctypes.c_int
    assert int(L._fn("ocr_sc_num_partials", ci)(ci(0), ci(18))) == UNSUPPORTED
    assert int(L._fn("ocr_sc_num_partials", ci)(ci(8), ci(129))) == UNSUPPORTED
    assert int(L._fn("ocr_sc_num_partials", ci)(ci(8), ci(0))) == UNSUPPORTED
    assert int(L._fn("ocr_conv1x1_small_batch_rows", ci)(ci(0))) == INVALID_ARG
    assert int(L._fn("ocr_sc_pointwise_pair_num_partials", ci)(ci(0))) == INVALID_ARG
    assert L.call_size("ocr_conv1x1_small_wgrad_batch_slab_bytes", ci(0), ci(128)) == 0
    assert L.call_size("ocr_conv1x1_small_wgrad_batch_slab_bytes", ci(64), ci(0)) == 0
    # batched forms: (struct, good row, pointer fields, (field index, bad -> INVALID_ARG), (field index, bad -> UNSUPPORTED), extra args)
    B = {
        "ocr_conv1x1_small_batch_f16": (ops.HeadConvItem, [h16, h16, None, G["o32"], None, P, cin, C], [0, 1, 3], [(5, (0,))], [(6, (0, 8)), (7, (0, 33))], ()),
        "ocr_conv1x1_small_dgrad_batch_f16": (ops.HeadDgradItem, [t32, h16, G["o16"], P, cin, C, 0], [0, 1, 2], [(3, (0,))], [(4, (0, 16)), (5, (0, 33))], (FL(1.0),)),
        "ocr_conv1x1_small_wgrad_batch_f16": (ops.HeadWgradItem, [h16, t32, G["dw"], G["ws"], P, cin, C], [0, 1, 2, 3], [(4, (0,))], [(5, (64, 0)), (6, (0, 33))], ()),
        "ocr_sc_bn_bwd_batch": (ops.ScBnBwdItem, [t32, v, v, v, v, t32, G["v0"], G["v1"], G["o32"], G["part"], P, C, 1], list(range(10)), [],
                                [(10, (0,)), (11, (0, 33, 100))], ()),
        "ocr_sc_colsum_batch": (ops.ScColsumItem, [t32, G["v0"], G["part"], P, C], [0, 1, 2], [(3, (0,))], [(4, (0, 33))], ()),
        "ocr_sc_act_batch": (ops.ScActItem, [t32, v, v, G["o32"], P * C, C], [0, 1, 2, 3], [(4, (0,)), (5, (0,))], [], (1,)),
    }
    for name, (cls, good, ptrs, inv, uns, extra) in B.items():
        one = _items(cls, [good])
        five = _items(cls, [good] * 5)
        assert _rc(L, name, None, 1, *extra) == INVALID_ARG, name
        assert _rc(L, name, one, 0, *extra) == INVALID_ARG, name
        assert _rc(L, name, five, 5, *extra) == INVALID_ARG, name
        for j in ptrs:
            r = list(good)
            r[j] = None
            assert _rc(L, name, _items(cls, [good, r]), 2, *extra) == INVALID_ARG, (name, j)
        for code, lst in ((INVALID_ARG, inv), (UNSUPPORTED, uns)):
            for j, bads in lst:
                for bad in bads:
                    r = list(good)
                    r[j] = bad
                    assert _rc(L, name, _items(cls, [good, r]), 2, *extra) == code, (name, j, bad)
    torch.cuda.synchronize()
    for k, g in G.items():
        assert g.untouched(), k
    # and the same buffers take a well-formed call
    assert _rc(L, "ocr_sc_sigmoid", t32, I64(P * 32), G["o32"]) == OK
    torch.cuda.synchronize()
    assert bool((G["o32"].t == 0.5).all()) and G["o32"].ok()
