"""GPU: the batch-norm, pool and unpool entries of csrc/bn_pool.hip and every entry of csrc/guest_bn.hip — batch-norm forward and backward, the fused 2x2 pool,
the general max-pool, the legacy bilinear unpool, bias+ReLU backward and the ticketed reduce_finalize_kernel — against a
float64 restatement in NumPy on the same 16-bit-exact operands (no autograd, no oracle routine, no device route compared
with another).  Every entry is called through ctypes on the library tensorflow_ocr_amd.ops binds: the status of each call
is part of what is asserted, and several wrappers hide an argument (max_workgroups, ws_bytes, T).  Not covered here:
ocr_prep_images_f16 / _norm_f16.

Kernels and the rows that reach them (ROWS, FIN_SHAPES, WINDOWS below):
  reduce_finalize_kernel<BnFin|BnBwdFin|BnBwdFinC>  FIN_SHAPES: (1,8) one partial row; (1024,64) | (1025,64) the R = 1 /
                            R > 1 switch; (6400,256) R = 16; (70000,8) rows = 2048, R = 35: ticket groups of 32 and 3 and
                            the second ticket level; (300,18) the scalar C % 4 branch; (2000,100) second channel group
                            half empty; exact rows for all three instantiations.  test_ticket_slots_reused: 20 calls
                            over the 16 self-resetting slots, at R = 5 (one first-level group) and at R = 35 (two
                            groups and the second-level counter).
                            Behind the row entries: tickets_c64 (T = 1049, rows 256, R = 5, last block 25 rows),
                            c2048_cap (32 channel groups).
  bn_finalize_batch_kernel                  test_finalize_batch (ocr_bn_finalize_batch, ocr_bn_bwd_sums_batch): C 1 | 3 | 18 |
                            32 (row lanes RL = 1024 / 2C = 512 | 170 | 28 | 16; at C = 3 and 18 the last 4 | 16 threads
                            own no lane) x T 1 | RL - 1 | RL | RL + 1 | 8 RL - 1 | 8 RL + 1 | 2048 (those <= 2048: the
                            launcher refuses more), all T of a C in one launch; test_finalize_batch_mixed: count 1..8,
                            C and T differing between the items, gamma / beta, moving statistics, save buffers given
                            or NULL per item; out0 against kind 0 and out1 against kind 1 separately (a swap of the
                            BnBwdFin{out1, out0} wiring fails both); test_batch_status_codes
  bn_inference_params_kernel                test_forward, every row
  bn_relu_kernel<relu, 0 | 2>               test_forward: pool 0 | 2 x relu 0 | 1 x with / without a_full; the index form
                            with / without a_full and y_pool; stream_cap: the capped grid's second pass (pool 0)
  bn_relu_bwd_kernel<0 | 1>                 test_backward: pool 0; pool 2 with / without da_full; the reduce-only and
                            apply-only entries; c2048_cap: one lane per block, 2070 units on 2048 blocks
  bn_pool_bwd_idx_kernel<0 | 1>             test_backward: the stored-index forms (apply form: partials formed here)
  bn_relu_bwd_gather_kernel<3,2> <0,0>      test_maxpool rows k3s2 and k5s3, with / without da_full_out
  bn_apply_affine_kernel, bn_pool_apply_affine_kernel, bn_poolfull_apply_affine_kernel, bn_reduce_rows_kernel,
  bn_poolfull_reduce_rows_kernel            test_guests: max_workgroups 0 | 256 | 3 (3: the grid-stride loops run)
  channel_stats_kernel, bias_relu_bwd_kernel, bn_add_relu_kernel<proj, bits>, relu_bwd_kernel, add_inplace_kernel
                                            test_elementwise, every row but stream_cap
  unpool_f16_kernel, unpool_bwd_f16_kernel, unpool_add_stats_kernel   test_unpool
  maxpool_fwd_kernel<bn, 0 | 2 | 3>, maxpool_bwd_idx_kernel<2,2> <3,2> <3,1> <1,2> <0,0>, maxpool_bwd_kernel
                                            test_maxpool: WINDOWS x odd / even map, 3x3/2 on a c = 24 map (three
                            chunks per pixel); stream_cap: capped grid (3x3/2)

Reference.  Operands are drawn on the storage grid.  The stored activation is round16(f32(y*scale + shift)), evaluated in
float64 two ways: fused (one rounding to f32) and unfused (the product rounded to f32, then the sum) — and, in the f16
build, a third way: the fused result rounded ONCE to f16 (see Findings).  An element is
FRAGILE when they disagree in stored value or sign, a pool window when its first maximum or its value differs; fragile
elements are skipped, and so is every per-channel sum they feed (and what is computed from such a sum).  The fragile
share is asserted <= 0.1 % per row from the reference alone, and at least three quarters of the channels must stay
checked.  Exact ties are not fragile: the first maximum in (dy, dx) order must win.  On the three large rows
(c2048_cap, tickets_c64, stream_cap) scale and shift are themselves on the storage grid (the product is then exact in
f32, fused and unfused agree and only the single-rounding cases remain), or a channel of 33 540 elements would never
be free of a fragile one.

Exact rows (dyadic operands: y and gradients k / 8 in [-4, 4], scale in {0.5, 1, 2}, shift k / 4, mean k / 2, invstd in
{0.5, 1, 2}, neighbouring pixels often equal, the first two map rows all negative) must match bit for bit (a zero's sign
apart): activations, pooled activations, index bytes (bits 0-1 position, bit 2 sign), y_pool, mask bits, routed
gradients (the apply entries get all-zero partials or B = 0 coefficients, so dy = scale * dz exactly), dgamma / dbeta,
max-pool indices and scatter, unpool and its transpose.

Random rows, derived bars (u = storage half-ulp 2^-11 | 2^-8, tiny = the smallest subnormal):
  stored 16-bit outputs   |dev - ref| <= u |ref| + 4 * 2^-24 * M + tiny, M = sum of |terms| of the expression
  per-channel sums        |dev - ref| <= m * 2^-24 * sum |term|, m = ceil(units / (T * lanes)) + lanes: the per-thread
                          loop plus the LDS column sum (T * lanes = the row count for the guests, whose rows carry
                          (sum dz y - mean sum dz) * invstd: terms |dz y| invstd and |mean dz| invstd).  Printed on
                          lines of their own (`<entry>_sums`).
  finalize outputs        the sum bounds propagated through bn_fin_apply's closed forms to first order, plus one
                          2^-24 per f32 operation (_fin_bounds, _coef_bounds)
An apply pass is referred to the dgamma / dbeta the device wrote (each checked against float64 on its own).

Measured, largest |err| / bound per entry over all rows (f16 / bf16 library), from the `bn_pool <entry> <row> ratio=`
lines: see MEASURED at the end of this docstring.

Findings
  * In the f16 build hipcc folds `(half_t)fmaf(y, scale, shift)` and `(half_t)(y * scale + shift)` into
    v_fma_mixlo_f16: the exact sum is rounded once to f16, not to f32 and then to f16.  The stored
    activation therefore differs by one f16 ulp from round16(f32(y * scale + shift)) in about 4 of 10^6 elements with
    full-f32 coefficients (15 of 4.2 M on c2048_cap, 10 of 2.1 M on tickets_c64 in the projection of
    ocr_bn_add_relu_f16); never in the bf16 build.  The single rounding is the more accurate one and every kernel of
    the file gets it alike, so nothing is changed; such elements are counted as fragile (a third evaluation).  That
    takes the device's rounding into the reference's fragile set: a kernel that mixed the two roundings between a
    forward and a backward pass on exactly those elements would not be noticed here.
  * The second ticket level of reduce_finalize_kernel (R > 32) is reached by no caller inside the library: bwd_blocks
    and the num_partials entries cap T at 2048 (rows 256, R = 8), the conv epilogues' statistics stay below that too.
    Only ocr_bn_finalize / ocr_bn_bwd_sums / ocr_bn_bwd_coefficients called directly with T > 65536 (32 blocks of 2048 rows) get there
    ((70000, 8) here); it is correct.
  * The pooled forms on the tickets_c64 map have T = ceil(2 * 65 * 65 / 32) = 265 partial rows (32 unit lanes at
    c = 64), R = 1 — not 529, which is the count at c = 128.
  * ocr_bn_relu_bwd_f16, ocr_bn_relu_bwd_reduce_f16 and ocr_bn_relu_bwd_apply_f16 sized a grid from n, h, w without
    checking them; they now answer OCR_ERR_INVALID_ARG for a non-positive extent (asserted in test_status_codes).
  * The guests take c / 4 a power of two up to 1024 channels: c = 2048 and c = 24 answer OCR_ERR_UNSUPPORTED there,
    as do odd h / w in the pooled forms (asserted in test_status_codes and test_guests).

MEASURED (largest |err| / bound over the rows, f16 / bf16 library; a stored 16-bit output that is right to the last bit
still shows the final rounding, up to 0.999 of u |ref|; 0.000 = the stored value equals the reference's everywhere)
  bn_finalize                        0.977 / 0.977      bn_relu_bwd                        0.999 / 0.996
  bn_finalize (NULL gamma, beta)     0.482 / 0.482      bn_relu_bwd_reduce (coefficients)  0.481 / 0.437
  bn_bwd_sums                        0.983 / 0.983      bn_relu_bwd_reduce_pooled          0.998 / 0.996
  bn_bwd_coefficients                0.983 / 0.983      bn_relu_bwd_apply                  0.998 / 0.996
  bn_inference_params                0.645 / 0.645      bn_relu_pool_bwd_idx               0.998 / 0.996
  bn_relu, bn_relu_pool_idx          0.000 / 0.000      bn_relu_pool_bwd_idx_apply         0.998 / 0.996
  bn_relu_maxpool                    0.000 / 0.000      bn_relu_bwd_apply_affine           0.998 / 0.996
  bn_add_relu                        0.999 / 0.996      bn_relu_pool_bwd_idx_apply_affine  0.996 / 0.995
  add_inplace                        0.999 / 0.996      bn_relu_poolfull_bwd_apply_affine  0.996 / 0.995
  channel_stats                      0.083 / 0.053      bn_relu_bwd_reduce_rows            0.029 / 0.030
  bias_relu_bwd (bias gradient)      0.047 / 0.040      maxpool_bwd                        0.999 / 0.996
  unpool                             0.998 / 0.996      unpool_bwd                         0.996 / 0.996
  unpool_add_stats                   0.999 / 0.996
  bn_finalize_batch                  0.971 / same       bn_bwd_sums_batch out0, out1       0.977, 0.994 / same
  (the batched entries read f32 partials only: one figure for both libraries, like bn_finalize / bn_bwd_sums)
  per-channel sums (`_sums` lines):  bn_relu_bwd 0.099 / 0.163, bn_relu_bwd_reduce 0.083 / 0.163,
                                     bn_relu_pool_bwd_idx 0.099 / 0.079, bn_relu_bwd_reduce_pooled 0.043 / 0.045
  The (T, C) sums sit at 0.98 because their bar is one f32 rounding of the result (the f64 stage adds nothing
  measurable).  Per-channel f32 sums stay below a fifth of m * 2^-24 * sum |term|.
  Statistics under cancellation (mean 8, deviation 0.05, 3200 values per channel, m = 33): the bound allows invstd 10 %
  (9.4 % bf16); measured 0.022 / 0.000 of it on scale, shift and invstd, 0.028 / 0.019 on the mean: the f32 partial sums
  of 32 values each lose far less than the one-pass bound, and the rest of the reduction is f64.
"""
import ctypes
import zlib
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (DB, F16, FL, I64, INVALID_ARG, OK, SZ, TINY, U16, U32, UNSUPPORTED, WORKSPACE, Guard, _bits_equal,
                            _d32, _dev, _exact32, _h, _ratio, _rc, _rng, f32, f64)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "bn_pool")

# name: ([shapes (n, h, w, c)], storage-grid scale/shift)
ROWS = {
    "tiny_c8": ([(1, 3, 5, 8)], False),
    "one_pixel": ([(1, 1, 1, 8), (2, 1, 7, 64)], False),
    "odd_c64": ([(2, 9, 11, 64)], False),
    "even_c128": ([(2, 8, 12, 128)], False),
    "c24": ([(2, 5, 7, 24)], False),
    "c2048_cap": ([(1, 46, 45, 2048)], True),
    "tickets_c64": ([(2, 130, 129, 64)], True),
}
STREAM_CAP = (2, 130, 129, 512)
SMALL = ["tiny_c8", "one_pixel", "odd_c64", "even_c128", "c24"]
BWD_ROWS = ["tiny_c8", "one_pixel", "odd_c64", "even_c128", "c2048_cap", "tickets_c64"]
GUEST_ROWS = ["tiny_c8", "odd_c64", "even_c128", "tickets_c64"]
KINDS = ("exact", "random")
FIN_SHAPES = [(1, 8), (1024, 64), (1025, 64), (6400, 256), (70000, 8), (300, 18), (2000, 100)]
FIN_R = {(1, 8): 1, (1024, 64): 1, (1025, 64): 5, (6400, 256): 16, (70000, 8): 35, (300, 18): 1, (2000, 100): 8}
WINDOWS = {"k2s2": (2, 2), "k3s2": (3, 2), "k3s1": (3, 1), "k1s2": (1, 2), "k5s3": (5, 3)}
POOL_MAPS = {"odd": (2, 7, 9, 64), "even": (2, 8, 6, 64), "c24": (2, 5, 7, 24)}
POOL_CASES = [(win, m) for m in ("odd", "even") for win in WINDOWS] + [("k3s2", "c24")]
BATCH_C = [1, 3, 18, 32]
N_TESTS = (2 * len(BATCH_C) + 8 + 1 + 2 * len(FIN_SHAPES) + 3 + 2 * len(SMALL) + 1 + 2 * len(ROWS) + 2 * 3 + 2 * len(BWD_ROWS)
           + 2 * 3 * len(GUEST_ROWS) + 2 * len(POOL_CASES) + 1)

_CACHE = {}


# ------------------------------------------------------------------------------------------------ host helpers
def red_rows(T):
    if T <= 1024:
        return (T + 63) // 64 * 64
    return min(max(((T + 15) // 16 + 31) // 32 * 32, 256), 2048)


def bwd_blocks(units, c):
    lanes = 256 // (c // 8)
    return min((units + lanes - 1) // lanes, 2048)


def _r16(got, ref, M, skip=None):
    """stored 16-bit output against float64"""
    ref = np.asarray(ref, f64)
    over = np.abs(got.astype(f64) - ref) > U16 * np.abs(ref) + 4 * U32 * np.asarray(M, f64) + TINY
    if skip is not None:
        over = over & ~skip
    for j in np.argwhere(over)[:3]:
        print("  got %r ref %r M %r at %s" % (float(got[tuple(j)]), float(ref[tuple(j)]), float(np.broadcast_to(M, ref.shape)[tuple(j)]), j.tolist()))
    return _ratio(np.abs(got.astype(f64) - ref), U16 * np.abs(ref) + 4 * U32 * np.asarray(M, f64) + TINY, skip)


def _rsum(got, ref, m, terms, okc=None):
    skip = None if okc is None else ~okc
    return _ratio(np.abs(got.astype(f64) - ref), m * U32 * terms, skip)


def _eq16(got, ref, what, skip=None):
    """a stored 16-bit output of an exact row: the exact value rounded once to the storage type"""
    _bits_equal(got, _h(np.asarray(ref, f32)), what, skip)


# ------------------------------------------------------------------------------------------------ device helpers
def _ws(L, T, c, device):
    nbytes = L.call_size("ocr_bn_reduce_workspace", ctypes.c_int(T), ctypes.c_int(c))
    rows = red_rows(T)
    assert nbytes == -(-T // rows) * 2 * c * 8
    return Guard((nbytes,), torch.uint8, device), SZ(nbytes)


# ------------------------------------------------------------------------------------------------ float64 reference
def _r16once(v64):
    """float64 -> storage type in ONE rounding where the f16 build can do that (v_fma_mixlo_f16: the fused multiply-add's
    exact result goes straight to f16); the bf16 build has no such instruction and rounds the f32 result"""
    return np.asarray(v64, f64).astype(np.float16).astype(f32) if F16 else _h(np.asarray(v64, f64).astype(f32))


def _act(P, mode, relu):
    y = P.y.astype(f64)
    if mode == "m":
        v = _r16once(y * P.sc + P.sh)
        return np.where(v > 0, v, f32(0)) if relu else v
    if mode == "f":
        v = (y * P.sc + P.sh).astype(f32)
    else:
        v = ((y * P.sc).astype(f32).astype(f64) + P.sh).astype(f32)
    if relu:
        v = np.where(v > 0, v, f32(0))
    return _h(v)


def _pool2(a):
    """2x2/2 SAME: (pooled value, position dy*2+dx of the FIRST maximum); candidates over an odd edge do not exist"""
    n, h, w, c = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    p = np.full((n, 2 * oh, 2 * ow, c), -np.inf, f32)
    p[:, :h, :w] = a
    cand = np.stack([p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]], 0)
    return cand.max(0), cand.argmax(0)


def _route2(idx, g, h, w):
    n, oh, ow, c = g.shape
    out = np.zeros((n, 2 * oh, 2 * ow, c), f64)
    for k in range(4):
        out[:, k >> 1::2, k & 1::2] = np.where(idx == k, g, 0.0)
    return out[:, :h, :w]


def _up2(m, h, w):
    """pooled-resolution mask -> every position of the window"""
    return np.repeat(np.repeat(m, 2, 1), 2, 2)[:, :h, :w]


def _same(h, k, s):
    oh = -(-h // s)
    return oh, max((oh - 1) * s + k - h, 0) // 2


def _maxpool(x, k, s):
    """general SAME max-pool: (y, position ky*k+kx of the first maximum, pads)"""
    n, h, w, c = x.shape
    (oh, pt), (ow, pl) = _same(h, k, s), _same(w, k, s)
    xp = np.full((n, pt + h + k + s, pl + w + k + s, c), -np.inf, f32)
    xp[:, pt:pt + h, pl:pl + w] = x
    cand = np.stack([xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] for ky in range(k) for kx in range(k)], 0)
    return cand.max(0), cand.argmax(0), (pt, pl)


def _maxpool_bwd(idx, dy, k, s, h, w, pads):
    """(scatter of dy to the first maxima, sum of |terms|) in float64"""
    n, oh, ow, c = dy.shape
    pt, pl = pads
    g = np.zeros((n, pt + h + k + s, pl + w + k + s, c), f64)
    m = np.zeros_like(g)
    for ky in range(k):
        for kx in range(k):
            t = np.where(idx == ky * k + kx, dy, 0.0)
            g[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] += t
            m[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] += np.abs(t)
    return g[:, pt:pt + h, pl:pl + w], m[:, pt:pt + h, pl:pl + w]


def _prep(row, i, kind):
    """operands of one shape of a row, their fragile sets (from the reference alone) and the shared float64 pieces"""
    key = (row, i, kind)
    if key in _CACHE:
        return _CACHE[key]
    shape = STREAM_CAP if row == "stream_cap" else ROWS[row][0][i]
    grid = True if row == "stream_cap" else ROWS[row][1]
    n, h, w, c = shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    rng = _rng(row, i, kind)
    P = NS(shape=shape, n=n, h=h, w=w, c=c, oh=oh, ow=ow, kind=kind, row="%s%s" % (row, "" if i == 0 else "_b"))
    if kind == "exact":
        y = rng.integers(-32, 33, shape) / 8.0
        same = rng.random(shape) < 0.5
        y[:, :, 1:] = np.where(same[:, :, 1:], y[:, :, :-1], y[:, :, 1:])          # ties inside the windows
        y[:, 1:] = np.where(rng.random((n, h - 1, w, c)) < 0.3, y[:, :-1], y[:, 1:])
        y[:, :2] = -(np.abs(y[:, :2]) % 2) - 2.0                                         # windows with nothing positive
        P.y = y.astype(f32)
        P.sc = rng.choice([0.5, 1.0, 2.0], c)
        P.sh = rng.integers(-4, 5, c) / 4.0
        P.mu = rng.integers(-2, 3, c) / 2.0
        P.inv = rng.choice([0.5, 1.0, 2.0], c)
        P.da = (rng.integers(-32, 33, shape) / 8.0).astype(f32)
        P.dap = (rng.integers(-32, 33, (n, oh, ow, c)) / 8.0).astype(f32)
        assert np.array_equal(_h(P.y), P.y) and np.array_equal(_h(P.da), P.da)
    else:
        P.y = _h(rng.standard_normal(shape))
        P.sc = rng.uniform(0.5, 1.5, c).astype(f32).astype(f64)
        P.sh = (rng.standard_normal(c) * 0.5).astype(f32).astype(f64)
        if grid:
            P.sc, P.sh = _h(P.sc).astype(f64), _h(P.sh).astype(f64)
        P.mu = (rng.standard_normal(c) * 0.3).astype(f32).astype(f64)
        P.inv = rng.uniform(0.5, 2.0, c).astype(f32).astype(f64)
        P.da = _h(rng.standard_normal(shape) * 0.5)
        P.dap = _h(rng.standard_normal((n, oh, ow, c)) * 0.5)
    # fragile sets
    zf, zu, zm = _act(P, "f", False), _act(P, "u", False), _act(P, "m", False)
    fe = (zf != zu) | ((zf > 0) != (zu > 0)) | (zf != zm)
    fw = np.zeros((n, oh, ow, c), bool)
    P.a, P.pool, P.idx = {}, {}, {}
    for relu in (0, 1):
        af = np.where(zf > 0, zf, f32(0)) if relu else zf
        au = np.where(zu > 0, zu, f32(0)) if relu else zu
        (pf, jf), (pu, ju) = _pool2(af), _pool2(au)
        pm, jm = _pool2(np.where(zm > 0, zm, f32(0)) if relu else zm)
        fw |= (jf != ju) | (pf != pu) | (jf != jm) | (pf != pm)
        P.a[relu], P.pool[relu], P.idx[relu] = af, pf, jf
    P.z = zf
    fwin = np.zeros((n, 2 * oh, 2 * ow, c), bool)
    fwin[:, :h, :w] = fe
    fw |= fwin[:, 0::2, 0::2] | fwin[:, 0::2, 1::2] | fwin[:, 1::2, 0::2] | fwin[:, 1::2, 1::2]
    P.fe, P.fw = fe | _up2(fw, h, w), fw
    share = float(P.fe.mean())
    assert share <= 1e-3, (row, kind, share)
    P.okc = ~P.fe.any(axis=(0, 1, 2))
    assert P.okc.mean() >= 0.75, (row, kind, float(P.okc.mean()))
    if kind == "exact":
        assert not P.fe.any()
    P.xh = (P.y.astype(f64) - P.mu) * P.inv
    _CACHE[key] = P
    return P


def _dz(P, relu, pool, full):
    """(dz, sum of the |gradient terms| that enter it) of the batch-norm backward in float64"""
    if not pool:
        g, ga = P.da.astype(f64), np.abs(P.da.astype(f64))
        mask = P.z > 0
    else:
        g = _route2(P.idx[relu], P.dap.astype(f64), P.h, P.w)
        ga = np.abs(g)
        if full:
            g, ga = g + P.da, ga + np.abs(P.da.astype(f64))
        mask = P.a[relu] > 0
    if relu:
        g, ga = np.where(mask, g, 0.0), np.where(mask, ga, 0.0)
    return g, ga


def _sums(P, dz, dza):
    """per-channel (dbeta, dgamma, sum |dz|, sum |dz xhat|)"""
    ax = (0, 1, 2)
    return dz.sum(ax), (dz * P.xh).sum(ax), dza.sum(ax), (dza * np.abs(P.xh)).sum(ax)


def _apply_ref(P, dz, dza, dgamma, dbeta):
    """dy = scale * (dz - dbeta / N - xhat * dgamma / N) and M, with the sums the device holds"""
    N = P.n * P.h * P.w
    kd, kx = dbeta.astype(f64) / N, dgamma.astype(f64) / N
    return P.sc * (dz - kd - P.xh * kx), np.abs(P.sc) * (dza + np.abs(kd) + np.abs(P.xh * kx))


def _chain(units, T, lanes):
    """m of the per-channel sum bars: the per-thread loop plus the LDS column sum"""
    return -(-units // (T * lanes)) + lanes


def _bn_args(P, device):
    return NS(y=_dev(P.y, device), sc=_d32(P.sc, device), sh=_d32(P.sh, device), mu=_d32(P.mu, device),
              inv=_d32(P.inv, device), da=_dev(P.da, device), dap=_dev(P.dap, device))


def _argmax_bytes(P, relu):
    return (P.idx[relu] | ((P.pool[relu] > 0).astype(np.int64) << 2)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ finalize family
def _fin_bounds(s, q, ds, dq, count, g, b, eps, d32, mm, mv):
    """bn_fin_apply<BnFin> in float64 and first-order bounds on every output (one 2^-24 per f32 operation)"""
    omd = f64(f32(1) - f32(d32))
    mean, dmean = s / count, ds / count
    var = q / count - mean * mean
    dvar = dq / count + 2 * np.abs(mean) * dmean + dmean ** 2
    assert (var - dvar > 0).all()
    inv = 1 / np.sqrt(var + eps)
    dinv = 0.5 * (var - dvar + eps) ** -1.5 * dvar + U32 * inv
    sc = g * inv
    dsc = np.abs(g) * dinv + U32 * np.abs(sc)
    sh = b - mean * sc
    dsh = np.abs(mean) * dsc + np.abs(sc) * dmean + U32 * (2 * np.abs(mean * sc) + np.abs(sh)) + dmean * dsc
    unb = var * count / (count - 1) if count > 1 else var
    dunb = dvar * (count / (count - 1) if count > 1 else 1)
    nmm = mm * f64(d32) + mean * omd
    dmm = omd * dmean + 4 * U32 * (np.abs(mm * f64(d32)) + np.abs(mean * omd))
    nmv = mv * f64(d32) + unb * omd
    dmv = omd * dunb + 4 * U32 * (np.abs(mv * f64(d32)) + np.abs(unb * omd))
    return {"scale": (sc, dsc), "shift": (sh, dsh), "save_mean": (mean, dmean + U32 * np.abs(mean)),
            "save_invstd": (inv, dinv), "moving_mean": (nmm, dmm), "moving_var": (nmv, dmv)}


def _coef_bounds(s, q, ds, dq, count, sc, mu, inv):
    """bn_fin_apply<BnBwdFinC>: A = scale, B = -scale invstd dgamma / N, C = scale (mean invstd dgamma / N - dbeta / N)"""
    B = -sc * inv * q / count
    dB = 6 * U32 * np.abs(B) + np.abs(sc * inv) * dq / count
    C = sc * (mu * inv * q / count - s / count)
    dC = 7 * U32 * (np.abs(sc * mu * inv * q / count) + np.abs(sc * s / count)) + np.abs(sc) * (np.abs(mu * inv) * dq + ds) / count
    return {"dbeta": (s, ds + U32 * np.abs(s)), "dgamma": (q, dq + U32 * np.abs(q)), "A": (sc, 0 * sc), "B": (B, dB), "C": (C, dC)}


def _fin_partials(T, C, kind, seed=0):
    rng = _rng(T, C, kind, seed)
    if kind == "exact":
        return (rng.integers(-32, 33, (T, 2, C)) / 8.0).astype(f32)
    mean, var = rng.standard_normal(C) * 0.5, rng.uniform(0.5, 2.0, C)
    p = np.empty((T, 2, C), f32)
    p[:, 0] = 16 * (mean + 0.1 * rng.standard_normal((T, C)))
    p[:, 1] = 16 * (var + mean ** 2 + 0.1 * rng.standard_normal((T, C)))
    return p


def _fin_partials_stats(T, C):
    """dyadic partials whose column sums are count * mean and count * (var + mean^2) exactly, count = 1024, mean k / 2,
    var in {0.25, 1, 4}: every closed form of bn_fin_apply<BnFin> is then exact (eps = 0, decay = 0.5) but the
    unbiased variance var * count / (count - 1)"""
    rng = _rng(T, C, "stats")
    p = rng.integers(-32, 33, (T, 2, C)) / 8.0
    mean, var, count = rng.integers(-2, 3, C) / 2.0, rng.choice([0.25, 1.0, 4.0], C), 1024.0
    p[0, 0] += count * mean - p[:, 0].sum(0)
    p[0, 1] += count * (var + mean ** 2) - p[:, 1].sum(0)
    p32 = p.astype(f32)
    assert np.array_equal(p32.astype(f64), p)
    assert np.array_equal(p32[:, 0].sum(0, dtype=f64), count * mean) and np.array_equal(p32[:, 1].sum(0, dtype=f64), count * (var + mean ** 2))
    return p32, mean, var, count


def _check_outs(entry, row, outs, refs):
    worst = 0.0
    for name, (ref, bound) in refs.items():
        got = outs[name].np().astype(f64)
        worst = max(worst, _ratio(np.abs(got - ref), bound + 1e-300))
    _note(entry, row, worst)


@pytest.mark.parametrize("T,C", FIN_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_finalize_family(device, T, C, kind):
    """ocr_bn_finalize, ocr_bn_bwd_sums and ocr_bn_bwd_coefficients on synthetic partials [T][2][C]: the f64 stage adds
    T * 2^-53 sum|partial| at most.  Exact rows, bit for bit: the sums of k / 8 partials; dgamma, dbeta and A, B, C with a
    power-of-two count and dyadic scale, mean, invstd; scale, shift, save_mean, save_invstd and moving_mean on partials
    with dyadic statistics (_fin_partials_stats), the moving variance inside its bar."""
    from tensorflow_ocr_amd import _lib as L
    rows = red_rows(T)
    assert -(-T // rows) == FIN_R[(T, C)]
    if (T, C) == (70000, 8):
        assert rows == 2048 and (-(-35 // 32), 35 - 32) == (2, 3)
    row = "T%d_C%d" % (T, C)
    p = _fin_partials(T, C, kind)
    pd = _d32(p, device)
    s, q = p[:, 0].sum(0, dtype=f64), p[:, 1].sum(0, dtype=f64)
    ds, dq = T * 2.0 ** -53 * np.abs(p[:, 0]).sum(0, dtype=f64), T * 2.0 ** -53 * np.abs(p[:, 1]).sum(0, dtype=f64)
    ws, nb = _ws(L, T, C, device)
    o = {k: Guard((C,), torch.float32, device) for k in ("out0", "out1")}
    assert _rc(L, "ocr_bn_bwd_sums", pd, T, C, o["out0"], o["out1"], ws, nb) == OK
    torch.cuda.synchronize()
    if kind == "exact":
        _bits_equal(o["out0"].np(), s.astype(f32), "sums kind 0")
        _bits_equal(o["out1"].np(), q.astype(f32), "sums kind 1")
        rng = np.random.default_rng(T * 17 + C)
        sc, mu, inv = rng.choice([0.5, 1.0, 2.0], C), rng.integers(-2, 3, C) / 2.0, rng.choice([0.5, 1.0, 2.0], C)
        count = 2.0 ** 20
        o = {k: Guard((C,), torch.float32, device) for k in ("dgamma", "dbeta", "A", "B", "C")}
        assert _rc(L, "ocr_bn_bwd_coefficients", pd, T, C, DB(count), _d32(sc, device), _d32(mu, device), _d32(inv, device),
                   o["dgamma"], o["dbeta"], o["A"], o["B"], o["C"], ws, nb) == OK
        torch.cuda.synchronize()
        for k, ref in (("dbeta", s), ("dgamma", q), ("A", sc), ("B", -sc * inv * q / count), ("C", sc * (mu * inv * q / count - s / count))):
            _bits_equal(o[k].np(), _exact32(ref), "coefficients " + k)
        p2, mean, var, count = _fin_partials_stats(T, C)
        g, b, mm, mv = rng.choice([0.5, 1.0, 2.0], C), rng.integers(-4, 5, C) / 4.0, rng.integers(-4, 5, C) / 4.0, rng.choice([0.5, 1.0, 2.0], C)
        o = {k: Guard((C,), torch.float32, device) for k in ("scale", "shift", "save_mean", "save_invstd")}
        o["moving_mean"], o["moving_var"] = Guard((C,), torch.float32, device, mm), Guard((C,), torch.float32, device, mv)
        assert _rc(L, "ocr_bn_finalize", _d32(p2, device), T, C, DB(count), _d32(g, device), _d32(b, device), FL(0.0), FL(0.5),
                   o["moving_mean"], o["moving_var"], o["scale"], o["shift"], o["save_mean"], o["save_invstd"], ws, nb) == OK
        torch.cuda.synchronize()
        inv = 1.0 / np.sqrt(var)
        for k, ref in (("scale", g * inv), ("shift", b - mean * g * inv), ("save_mean", mean), ("save_invstd", inv),
                       ("moving_mean", 0.5 * mm + 0.5 * mean)):
            _bits_equal(o[k].np(), _exact32(ref), "finalize " + k)
        fb = _fin_bounds(count * mean, count * (var + mean ** 2), 0.0, 0.0, count, g, b, 0.0, f32(0.5), mm, mv)
        assert _ratio(np.abs(o["moving_var"].np() - fb["moving_var"][0]), fb["moving_var"][1]) <= 1
        assert ws.ok()
        return
    _check_outs("bn_bwd_sums", row, o, {"out0": (s, ds + U32 * np.abs(s)), "out1": (q, dq + U32 * np.abs(q))})
    rng = np.random.default_rng(T * 131 + C)
    sc, mu, inv = (rng.uniform(0.5, 1.5, C).astype(f32), (rng.standard_normal(C) * 0.3).astype(f32),
                   rng.uniform(0.5, 2.0, C).astype(f32))
    count = 16.0 * T
    o = {k: Guard((C,), torch.float32, device) for k in ("dgamma", "dbeta", "A", "B", "C")}
    ws2, _ = _ws(L, T, C, device)
    assert _rc(L, "ocr_bn_bwd_coefficients", pd, T, C, DB(count), _d32(sc, device), _d32(mu, device), _d32(inv, device),
               o["dgamma"], o["dbeta"], o["A"], o["B"], o["C"], ws2, nb) == OK
    torch.cuda.synchronize()
    _check_outs("bn_bwd_coefficients", row, o, _coef_bounds(s, q, ds, dq, count, sc.astype(f64), mu.astype(f64), inv.astype(f64)))
    assert np.array_equal(o["A"].np(), sc)
    g, b, mm, mv = (rng.uniform(0.5, 1.5, C).astype(f32), rng.standard_normal(C).astype(f32),
                    rng.standard_normal(C).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32))
    eps, dec = f32(1e-5), f32(0.997)
    names = ("scale", "shift", "save_mean", "save_invstd")
    o = {k: Guard((C,), torch.float32, device) for k in names}
    o["moving_mean"], o["moving_var"] = Guard((C,), torch.float32, device, mm), Guard((C,), torch.float32, device, mv)
    ws3, _ = _ws(L, T, C, device)
    assert _rc(L, "ocr_bn_finalize", pd, T, C, DB(count), _d32(g, device), _d32(b, device), FL(eps), FL(dec), o["moving_mean"],
               o["moving_var"], o["scale"], o["shift"], o["save_mean"], o["save_invstd"], ws3, nb) == OK
    torch.cuda.synchronize()
    _check_outs("bn_finalize", row, o, _fin_bounds(s, q, ds, dq, count, g.astype(f64), b.astype(f64), f64(eps), dec,
                                                   mm.astype(f64), mv.astype(f64)))
    # gamma / beta / moving_* / save_* NULL: scale = invstd, shift = -mean * invstd
    o2 = {k: Guard((C,), torch.float32, device) for k in ("scale", "shift")}
    assert _rc(L, "ocr_bn_finalize", pd, T, C, DB(count), None, None, FL(eps), FL(dec), None, None, o2["scale"], o2["shift"],
               None, None, ws3, nb) == OK
    torch.cuda.synchronize()
    fb = _fin_bounds(s, q, ds, dq, count, np.ones(C), np.zeros(C), f64(eps), dec, mm.astype(f64), mv.astype(f64))
    _check_outs("bn_finalize_null", row, o2, {k: fb[k] for k in ("scale", "shift")})
    assert ws.ok() and ws2.ok() and ws3.ok()
    assert np.array_equal(pd.cpu().numpy(), p)


# ---- the batched finalisation (bn_finalize_batch_kernel): up to eight small reductions per launch ----
class BnSumsItem(ctypes.Structure):
    """ocr_bn_sums_item (include/ocr_hip.h)"""
    _fields_ = [("partial", ctypes.c_void_p), ("T", ctypes.c_int32), ("C", ctypes.c_int32), ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p)]


def _batch_T(C):
    RL = 1024 // (2 * C)
    return [T for T in (1, RL - 1, RL, RL + 1, 8 * RL - 1, 8 * RL + 1, 2048) if T <= 2048]


def _dp(v):
    return None if v is None else (v.t if isinstance(v, Guard) else v).data_ptr()


def _run_batch(device, spec, kind, tag):
    """spec: [(T, C, opts)], opts bit 0: gamma / beta given, bit 1: moving statistics, bit 2: save buffers.  One launch
    of ocr_bn_bwd_sums_batch and one of ocr_bn_finalize_batch over all items, against the float64 references of the
    single forms."""
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd import ops
    n = len(spec)
    exact = kind == "exact"
    its = []
    for i, (T, C, opts) in enumerate(spec):
        it = NS(T=T, C=C, opts=opts, row="%s_i%d_T%d_C%d_o%d" % (tag, i, T, C, opts))
        it.p = _fin_partials(T, C, kind, seed=i)
        it.pd = Guard((T, 2, C), torch.float32, device, it.p)
        it.o = {k: Guard((C,), torch.float32, device) for k in ("out0", "out1")}
        its.append(it)
    arr = (BnSumsItem * n)(*[BnSumsItem(_dp(it.pd), it.T, it.C, _dp(it.o["out0"]), _dp(it.o["out1"])) for it in its])
    assert _rc(L, "ocr_bn_bwd_sums_batch", arr, n) == OK
    torch.cuda.synchronize()
    for it in its:
        p, T = it.p, it.T
        it.s, it.q = p[:, 0].sum(0, dtype=f64), p[:, 1].sum(0, dtype=f64)
        it.ds, it.dq = T * 2.0 ** -53 * np.abs(p[:, 0]).sum(0, dtype=f64), T * 2.0 ** -53 * np.abs(p[:, 1]).sum(0, dtype=f64)
        if exact:
            _bits_equal(it.o["out0"].np(), it.s.astype(f32), "batch sums kind 0 " + it.row)
            _bits_equal(it.o["out1"].np(), it.q.astype(f32), "batch sums kind 1 " + it.row)
        else:
            _check_outs("bn_bwd_sums_batch_out0", it.row, it.o, {"out0": (it.s, it.ds + U32 * np.abs(it.s))})
            _check_outs("bn_bwd_sums_batch_out1", it.row, it.o, {"out1": (it.q, it.dq + U32 * np.abs(it.q))})
        assert np.array_equal(it.pd.np(), p)
    eps, dec = (f32(0.0), f32(0.5)) if exact else (f32(1e-5), f32(0.997))
    rows = []
    for i, it in enumerate(its):
        T, C, opts = it.T, it.C, it.opts
        rng = np.random.default_rng(T * 131 + C + i)
        if exact:
            it.p2, it.mean, it.var, it.count = _fin_partials_stats(T, C)
            g, b, mm, mv = rng.choice([0.5, 1.0, 2.0], C), rng.integers(-4, 5, C) / 4.0, rng.integers(-4, 5, C) / 4.0, rng.choice([0.5, 1.0, 2.0], C)
        else:
            it.p2, it.count = it.p, 16.0 * T
            g, b, mm, mv = rng.uniform(0.5, 1.5, C), rng.standard_normal(C), rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
        it.g, it.b, it.mm, it.mv = (np.asarray(v, f32) for v in (g, b, mm, mv))
        it.pd2 = _d32(it.p2, device)
        it.f = {k: Guard((C,), torch.float32, device) for k in ("scale", "shift")}
        if opts & 2:
            it.f["moving_mean"], it.f["moving_var"] = Guard((C,), torch.float32, device, it.mm), Guard((C,), torch.float32, device, it.mv)
        if opts & 4:
            it.f["save_mean"], it.f["save_invstd"] = Guard((C,), torch.float32, device), Guard((C,), torch.float32, device)
        gd, bd = (_d32(it.g, device), _d32(it.b, device)) if opts & 1 else (None, None)
        it.keep = (gd, bd)
        rows.append((_dp(it.pd2), T, C, float(it.count), _dp(gd), _dp(bd), _dp(it.f.get("moving_mean")), _dp(it.f.get("moving_var")),
                     _dp(it.f["scale"]), _dp(it.f["shift"]), _dp(it.f.get("save_mean")), _dp(it.f.get("save_invstd"))))
    arr = (ops.BnFinalizeItem * n)(*[ops.BnFinalizeItem(*r) for r in rows])
    assert _rc(L, "ocr_bn_finalize_batch", arr, n, FL(eps), FL(dec)) == OK
    torch.cuda.synchronize()
    for it in its:
        C = it.C
        g64, b64 = (it.g.astype(f64), it.b.astype(f64)) if it.opts & 1 else (np.ones(C), np.zeros(C))
        if exact:
            inv = 1.0 / np.sqrt(it.var)
            want = {"scale": g64 * inv, "shift": b64 - it.mean * g64 * inv, "save_mean": it.mean, "save_invstd": inv,
                    "moving_mean": 0.5 * it.mm.astype(f64) + 0.5 * it.mean}
            for k, ref in want.items():
                if k in it.f:
                    _bits_equal(it.f[k].np(), _exact32(ref), "finalize_batch %s %s" % (k, it.row))
            fb = _fin_bounds(it.count * it.mean, it.count * (it.var + it.mean ** 2), 0.0, 0.0, it.count, g64, b64, 0.0, dec,
                             it.mm.astype(f64), it.mv.astype(f64))
            if "moving_var" in it.f:
                assert _ratio(np.abs(it.f["moving_var"].np() - fb["moving_var"][0]), fb["moving_var"][1]) <= 1
        else:
            fb = _fin_bounds(it.s, it.q, it.ds, it.dq, it.count, g64, b64, f64(eps), dec, it.mm.astype(f64), it.mv.astype(f64))
            _check_outs("bn_finalize_batch", it.row, it.f, {k: fb[k] for k in it.f})


@pytest.mark.parametrize("C", BATCH_C)
@pytest.mark.parametrize("kind", KINDS)
def test_finalize_batch(device, C, kind):
    """every T of one C in ONE launch (up to seven items): the row-lane edges RL - 1 | RL | RL + 1, the eight-in-flight
    loop's 8 RL - 1 | 8 RL + 1 and the largest T the launcher takes"""
    Ts = _batch_T(C)
    assert (1024 // (2 * C), len(Ts)) == {1: (512, 5), 3: (170, 7), 18: (28, 7), 32: (16, 7)}[C]
    _run_batch(device, [(T, C, (1, 7, 0, 3, 5, 6, 2)[i]) for i, T in enumerate(Ts)], kind, "C%d" % C)


@pytest.mark.parametrize("count", range(1, 9))
def test_finalize_batch_mixed(device, count):
    """count items whose C and T all differ; optional operands given or NULL per item"""
    pool = [(29, 18, 7), (2048, 1, 0), (171, 3, 5), (16, 32, 2), (225, 18, 1), (1, 32, 6), (1361, 3, 3), (513, 1, 4)]
    spec = (pool[count - 1:] + pool[:count - 1])[:count]
    _run_batch(device, spec, "random" if count % 2 else "exact", "n%d" % count)


def test_batch_status_codes(device):
    """count 0 | 9, T 0 | 2049, C 0 | 33, a NULL partial / scale / shift / out0 / out1, count <= 0.0, in the first item
    and in the second of two: nothing is written (the items are validated before the launch)"""
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd import ops
    T, C = 20, 18
    part = torch.zeros((T, 2, C), dtype=torch.float32, device=device)
    G = {k: Guard((C,), torch.float32, device) for k in ("a0", "a1", "b0", "b1")}
    pp = part.data_ptr()

    def fin(**over):
        v = dict(partial=pp, T=T, C=C, count=64.0, gamma=None, beta=None, moving_mean=None, moving_var=None,
                 scale=_dp(G["a0"]), shift=_dp(G["a1"]), save_mean=None, save_invstd=None)
        v.update(over)
        return ops.BnFinalizeItem(**v)

    def sums(**over):
        v = dict(partial=pp, T=T, C=C, out0=_dp(G["b0"]), out1=_dp(G["b1"]))
        v.update(over)
        return BnSumsItem(**v)

    def rc_fin(items, n=None):
        return _rc(L, "ocr_bn_finalize_batch", (ops.BnFinalizeItem * max(len(items), 1))(*items), len(items) if n is None else n, FL(1e-5), FL(0.9))

    def rc_sums(items, n=None):
        return _rc(L, "ocr_bn_bwd_sums_batch", (BnSumsItem * max(len(items), 1))(*items), len(items) if n is None else n)

    for mk, rc, nulls in ((fin, rc_fin, ("partial", "scale", "shift")), (sums, rc_sums, ("partial", "out0", "out1"))):
        assert rc([mk()], 0) == INVALID_ARG and rc([mk()] * 9) == INVALID_ARG and rc([mk()], -1) == INVALID_ARG
        for lead in ([], [mk()]):
            for k in nulls:
                assert rc(lead + [mk(**{k: None})]) == INVALID_ARG, k
            for k, v in (("T", 0), ("T", 2049), ("C", 0), ("C", 33)):
                assert rc(lead + [mk(**{k: v})]) == UNSUPPORTED, (k, v)
    assert _rc(L, "ocr_bn_finalize_batch", None, 1, FL(1e-5), FL(0.9)) == INVALID_ARG
    assert _rc(L, "ocr_bn_bwd_sums_batch", None, 1) == INVALID_ARG
    for cnt in (0.0, -1.0):
        assert rc_fin([fin(count=cnt)]) == INVALID_ARG and rc_fin([fin(), fin(count=cnt)]) == INVALID_ARG
    torch.cuda.synchronize()
    for k, g in G.items():
        assert g.untouched(), k
    assert rc_fin([fin()]) == OK and rc_sums([sums()]) == OK
    torch.cuda.synchronize()
    assert all(g.ok() for g in G.values()) and not G["b0"].np().any() and not G["b1"].np().any()


@pytest.mark.parametrize("T,C,R", [(1025, 64, 5), (70000, 8, 35)], ids=["R5", "R35"])
def test_ticket_slots_reused(device, T, C, R):
    """20 R > 1 reductions in a row on the same partials: more calls than the 16 rotating ticket slots, so every slot is
    used again after its self-reset.  All 20 results bit-identical to the first and inside the bar.  R = 5: one first-level
    group per slot; R = 35: two groups (32 and 3) and the second-level counter reset and reused as well."""
    from tensorflow_ocr_amd import _lib as L
    assert -(-T // red_rows(T)) == R
    p = _fin_partials(T, C, "random", 1)
    pd = _d32(p, device)
    s, q = p[:, 0].sum(0, dtype=f64), p[:, 1].sum(0, dtype=f64)
    first = None
    for call in range(20):
        ws, nb = _ws(L, T, C, device)
        o0, o1 = Guard((C,), torch.float32, device), Guard((C,), torch.float32, device)
        assert _rc(L, "ocr_bn_bwd_sums", pd, T, C, o0, o1, ws, nb) == OK
        torch.cuda.synchronize()
        got = (o0.np(), o1.np())
        assert ws.ok()
        if first is None:
            first = got
            ds, dq = T * 2.0 ** -53 * np.abs(p[:, 0]).sum(0, dtype=f64), T * 2.0 ** -53 * np.abs(p[:, 1]).sum(0, dtype=f64)
            r = max(_ratio(np.abs(got[0] - s), ds + U32 * np.abs(s)), _ratio(np.abs(got[1] - q), dq + U32 * np.abs(q)))
            _note("bn_bwd_sums", "20_calls_R%d" % R, r)
        assert np.array_equal(got[0].view(np.int32), first[0].view(np.int32)), call
        assert np.array_equal(got[1].view(np.int32), first[1].view(np.int32)), call


def test_stats_under_cancellation(device):
    """ocr_channel_stats_f16 -> ocr_bn_finalize with per-channel mean ~ 8, standard deviation ~ 0.05: the variance is
    q / count - mean^2 on f32 partial sums.  The bar is the one-pass bound on the partial sums (m * 2^-24 * sum|term|)
    propagated to invstd through _fin_bounds."""
    from tensorflow_ocr_amd import _lib as L
    n, h, w, c = 2, 40, 40, 64
    rng = np.random.default_rng(7)
    x = _h(8.0 + 0.05 * rng.standard_normal((n, h, w, c)))
    npix = n * h * w
    T = L.call_int("ocr_channel_stats_num_partials", I64(npix), ctypes.c_int(c))
    lanes = 256 // (c // 8)
    assert T == min(-(-npix // lanes), 2048) == 100
    part = Guard((T, 2, c), torch.float32, device)
    assert _rc(L, "ocr_channel_stats_f16", _dev(x, device), I64(npix), c, part) == OK
    x64 = x.astype(f64).reshape(-1, c)
    s, q = x64.sum(0), (x64 * x64).sum(0)
    m = _chain(npix, T, lanes)
    ds, dq = m * U32 * np.abs(x64).sum(0), m * U32 * q
    got = part.np().astype(f64)
    _note("channel_stats", "cancellation", max(_ratio(np.abs(got[:, 0].sum(0) - s), ds), _ratio(np.abs(got[:, 1].sum(0) - q), dq)))
    o = {k: Guard((c,), torch.float32, device) for k in ("scale", "shift", "save_mean", "save_invstd")}
    ws, nb = _ws(L, T, c, device)
    assert _rc(L, "ocr_bn_finalize", part, T, c, DB(npix), None, None, FL(1e-5), FL(0.997), None, None, o["scale"], o["shift"],
               o["save_mean"], o["save_invstd"], ws, nb) == OK
    torch.cuda.synchronize()
    fb = _fin_bounds(s, q, ds, dq, float(npix), np.ones(c), np.zeros(c), f64(f32(1e-5)), f32(0.997), np.zeros(c), np.ones(c))
    worst = 0.0
    for k in o:
        ref, bound = fb[k]
        r = _ratio(np.abs(o[k].np().astype(f64) - ref), bound)
        print("bn_pool cancellation %s: ratio=%.3f  (bound / value: %.2e)" % (k, r, float((bound / np.abs(ref)).max())))
        worst = max(worst, r)
    _note("bn_finalize", "cancellation", worst)


# ------------------------------------------------------------------------------------------------ forward
def _fwd_row(L, device, row, i, kind):
    P = _prep(row, i, kind)
    n, h, w, c, oh, ow = P.n, P.h, P.w, P.c, P.oh, P.ow
    D = _bn_args(P, device)
    exact = kind == "exact"
    worst = {}

    def chk(entry, got, ref, skip, M=None):
        if exact:
            _bits_equal(got, ref, "%s %s" % (entry, P.row), skip)
        else:
            worst[entry] = max(worst.get(entry, 0.0), _r16(got, ref, np.abs(ref) if M is None else M, skip))

    Mfull = np.abs(P.y.astype(f64) * P.sc) + np.abs(P.sh)
    Mpool = {r: np.abs(P.pool[r].astype(f64)) + 2 * np.abs(P.sh) for r in (0, 1)}     # |y scale| <= |a| + |shift|
    for relu in (0, 1):
        full = Guard(P.shape, O.STORAGE, device)
        assert _rc(L, "ocr_bn_relu_f16", D.y, D.sc, D.sh, n, h, w, c, relu, 0, full, None) == OK
        chk("bn_relu", full.np(), P.a[relu], P.fe, Mfull)
        for with_full in (0, 1):
            full = Guard(P.shape, O.STORAGE, device) if with_full else None
            pooled = Guard((n, oh, ow, c), O.STORAGE, device)
            assert _rc(L, "ocr_bn_relu_f16", D.y, D.sc, D.sh, n, h, w, c, relu, 2, full, pooled) == OK
            chk("bn_relu", pooled.np(), P.pool[relu], P.fw, Mpool[relu])
            if full:
                chk("bn_relu", full.np(), P.a[relu], P.fe, Mfull)
            for with_yp in (0, 1):
                full = Guard(P.shape, O.STORAGE, device) if with_full else None
                pooled = Guard((n, oh, ow, c), O.STORAGE, device)
                am = Guard((n, oh, ow, c), torch.uint8, device)
                yp = Guard((n, oh, ow, c), O.STORAGE, device) if with_yp else None
                assert _rc(L, "ocr_bn_relu_pool_idx_f16", D.y, D.sc, D.sh, n, h, w, c, relu, full, pooled, am, yp) == OK
                chk("bn_relu_pool_idx", pooled.np(), P.pool[relu], P.fw, Mpool[relu])
                bad = (am.np() != _argmax_bytes(P, relu)) & ~P.fw          # (random rows too: an index is right or wrong)
                assert not bad.any(), (P.row, relu, np.argwhere(bad)[:4].tolist())
                if full:
                    chk("bn_relu_pool_idx", full.np(), P.a[relu], P.fe, Mfull)
                if yp:
                    ypad = np.zeros((n, 2 * oh, 2 * ow, c), f32)
                    ypad[:, :h, :w] = P.y
                    cand = np.stack([ypad[:, 0::2, 0::2], ypad[:, 0::2, 1::2], ypad[:, 1::2, 0::2], ypad[:, 1::2, 1::2]], 0)
                    ref = np.take_along_axis(cand, P.idx[relu][None], 0)[0]
                    _bits_equal(yp.np(), ref, "y_pool %s" % P.row, P.fw)
    # inference parameters: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
    rng = np.random.default_rng(c)
    if exact:
        g, b, mm, mv, eps = rng.choice([0.5, 1, 2], c), rng.integers(-4, 5, c) / 4.0, rng.integers(-4, 5, c) / 4.0, rng.choice([0.25, 1, 4], c), 0.0
    else:
        g, b, mm, mv, eps = rng.uniform(0.5, 1.5, c), rng.standard_normal(c), rng.standard_normal(c), rng.uniform(0.5, 2, c), 1e-5
    g, b, mm, mv = [np.asarray(v, f32) for v in (g, b, mm, mv)]
    for null in (0, 1):
        osc, osh = Guard((c,), torch.float32, device), Guard((c,), torch.float32, device)
        assert _rc(L, "ocr_bn_inference_params", None if null else _d32(g, device), None if null else _d32(b, device),
                   _d32(mm, device), _d32(mv, device), FL(eps), c, osc, osh) == OK
        g64, b64 = (np.ones(c), np.zeros(c)) if null else (g.astype(f64), b.astype(f64))
        rsc = g64 / np.sqrt(mv.astype(f64) + f64(f32(eps)))
        rsh = b64 - mm.astype(f64) * rsc
        if exact:
            _bits_equal(osc.np(), rsc.astype(f32), "inference scale")
            _bits_equal(osh.np(), rsh.astype(f32), "inference shift")
        else:   # add, sqrt, divide, multiply: 4 operations on scale; the product and the difference on shift
            r = max(_ratio(np.abs(osc.np() - rsc), 4 * U32 * np.abs(rsc)),
                    _ratio(np.abs(osh.np() - rsh), U32 * (6 * np.abs(mm * rsc) + np.abs(rsh)) + 1e-300))
            worst["bn_inference_params"] = max(worst.get("bn_inference_params", 0.0), r)
    torch.cuda.synchronize()
    for entry, r in worst.items():
        _note(entry, P.row, r)


@pytest.mark.parametrize("row", SMALL)
@pytest.mark.parametrize("kind", KINDS)
def test_forward(device, row, kind):
    """ocr_bn_relu_f16 (pool 0 | 2, relu 0 | 1, with / without a_full), ocr_bn_relu_pool_idx_f16 (with / without a_full
    and y_pool) and ocr_bn_inference_params."""
    from tensorflow_ocr_amd import _lib as L
    for i in range(len(ROWS[row][0])):
        _fwd_row(L, device, row, i, kind)


def test_stream_cap(device):
    """2 146 560 chunk items > 8192 x 256: the stream_grid cap applies and the grid-stride loop's second pass runs, in
    ocr_bn_relu_f16 (pool 0) and ocr_maxpool_bwd_f16 (stored index, 3x3/2)."""
    from tensorflow_ocr_amd import _lib as L
    P = _prep("stream_cap", 0, "random")
    n, h, w, c = P.shape
    assert n * h * w * (c // 8) == 2146560 > 8192 * 256
    D = NS(y=_dev(P.y, device), sc=_d32(P.sc, device), sh=_d32(P.sh, device))
    full = Guard(P.shape, O.STORAGE, device)
    assert _rc(L, "ocr_bn_relu_f16", D.y, D.sc, D.sh, n, h, w, c, 1, 0, full, None) == OK
    _note("bn_relu", "stream_cap", _r16(full.np(), P.a[1], np.abs(P.y.astype(f64) * P.sc) + np.abs(P.sh), P.fe))
    k, s = 3, 2
    _, idx, pads = _maxpool(P.y, k, s)
    oh, ow = idx.shape[1:3]
    dy = P.dap[:, :oh, :ow].copy()
    assert dy.shape == idx.shape
    ref, M = _maxpool_bwd(idx, dy.astype(f64), k, s, h, w, pads)
    dx = Guard(P.shape, O.STORAGE, device)
    assert _rc(L, "ocr_maxpool_bwd_f16", None, torch.from_numpy(idx.astype(np.uint8)).to(device), _dev(dy, device), n, h, w, c,
               k, s, pads[0], pads[1], oh, ow, dx, 0) == OK
    _note("maxpool_bwd", "stream_cap", _r16(dx.np(), ref, M))


# ------------------------------------------------------------------------------------------------ element-wise, statistics
@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("kind", KINDS)
def test_elementwise(device, row, kind):
    """ocr_channel_stats_f16, ocr_bias_relu_bwd_f16 (relu 0 | 1), ocr_bn_add_relu_f16 (with / without projection and
    mask_bits), ocr_relu_bwd_f16, ocr_add_inplace_f16.  c = 24: the entries with a lane-per-chunk thread map answer
    OCR_ERR_UNSUPPORTED (and so do their num_partials), the streaming ones must be right."""
    from tensorflow_ocr_amd import _lib as L
    exact = kind == "exact"
    for i in range(len(ROWS[row][0])):
        P = _prep(row, i, kind)
        n, h, w, c = P.shape
        npix = n * h * w
        D = _bn_args(P, device)
        worst = {}
        y64 = P.y.astype(f64).reshape(-1, c)
        if c == 24:
            assert int(L._fn("ocr_channel_stats_num_partials", ctypes.c_int)(I64(npix), ctypes.c_int(c))) == UNSUPPORTED
            assert int(L._fn("ocr_bias_relu_bwd_num_partials", ctypes.c_int)(I64(npix), ctypes.c_int(c))) == UNSUPPORTED
            assert int(L._fn("ocr_bn_bwd_num_partials", ctypes.c_int)(n, h, w, c, 0)) == UNSUPPORTED
            part = Guard((8, 2, c), torch.float32, device)
            dz = Guard(P.shape, O.STORAGE, device)
            assert _rc(L, "ocr_channel_stats_f16", D.y, I64(npix), c, part) == UNSUPPORTED
            assert _rc(L, "ocr_bias_relu_bwd_f16", D.y, D.da, I64(npix), c, 1, dz, part, part) == UNSUPPORTED
            assert part.untouched() and dz.untouched()
        else:
            lanes = 256 // (c // 8)
            T = L.call_int("ocr_channel_stats_num_partials", I64(npix), ctypes.c_int(c))
            assert T == min(-(-npix // lanes), 2048)
            if row == "c2048_cap":
                assert (lanes, npix, T) == (1, 2070, 2048)
            part = Guard((T, 2, c), torch.float32, device)
            assert _rc(L, "ocr_channel_stats_f16", D.y, I64(npix), c, part) == OK
            got = part.np().astype(f64)
            s, q, sa = y64.sum(0), (y64 * y64).sum(0), np.abs(y64).sum(0)
            if exact:
                _bits_equal(got[:, 0].sum(0).astype(f32), s.astype(f32), "channel sums")
                _bits_equal(got[:, 1].sum(0).astype(f32), q.astype(f32), "channel square sums")
            else:
                m = _chain(npix, T, lanes)
                worst["channel_stats"] = max(_rsum(got[:, 0].sum(0), s, m, sa), _rsum(got[:, 1].sum(0), q, m, q))
            for relu in (0, 1):
                a = P.a[1]                                             # the stored activation the mask is read from
                dz = Guard(P.shape, O.STORAGE, device)
                dbias = Guard((c,), torch.float32, device)
                part = Guard((T, c), torch.float32, device)
                assert _rc(L, "ocr_bias_relu_bwd_f16", _dev(a, device), D.da, I64(npix), c, relu, dz, dbias, part) == OK
                ref = np.where(a > 0, P.da, f32(0)) if relu else P.da
                _bits_equal(dz.np(), ref, "bias_relu_bwd dz")             # a selection: exact in every row
                r64 = ref.astype(f64).reshape(-1, c)
                if exact:
                    _bits_equal(dbias.np(), r64.sum(0).astype(f32), "dbias")
                else:
                    m = _chain(npix, T, lanes)
                    worst["bias_relu_bwd"] = max(worst.get("bias_relu_bwd", 0), _rsum(dbias.np(), r64.sum(0), m, np.abs(r64).sum(0)))
        # out = relu(round16(fma(y, scale, shift)) + shortcut'), shortcut' = round16(fma(shortcut, sc_scale, sc_shift))
        short = P.da
        z = P.z.astype(f64)
        for proj in (0, 1):
            if proj:
                sv = _h((short.astype(f64) * P.inv + P.mu).astype(f32)).astype(f64)
                sv_u = _h(((short.astype(f64) * P.inv).astype(f32).astype(f64) + P.mu).astype(f32)).astype(f64)
                skip = P.fe | (sv != sv_u) | (sv != _r16once(short.astype(f64) * P.inv + P.mu))
            else:
                sv, skip = short.astype(f64), P.fe
            ref = np.maximum(z + sv, 0.0)
            refbits = np.packbits((_h(ref.astype(f32)) > 0).reshape(-1, 8), axis=1, bitorder="little").reshape(n, h, w, c // 8)
            for bits in (0, 1):
                out = Guard(P.shape, O.STORAGE, device)
                mb = Guard((n, h, w, c // 8), torch.uint8, device) if bits else None
                assert _rc(L, "ocr_bn_add_relu_f16", D.y, D.sc, D.sh, D.da, D.inv if proj else None, D.mu if proj else None,
                           I64(npix), c, out, mb) == OK
                got = out.np()
                if exact:
                    _eq16(got, ref, "bn_add_relu", skip)
                else:
                    worst["bn_add_relu"] = max(worst.get("bn_add_relu", 0), _r16(got, ref, np.abs(z) + np.abs(sv), skip))
                if bits:                                               # the mask is that of the STORED output
                    gotbits = np.packbits((got > 0).reshape(-1, 8), axis=1, bitorder="little").reshape(n, h, w, c // 8)
                    assert np.array_equal(mb.np(), gotbits)
                    if exact:
                        assert np.array_equal(mb.np(), refbits)
        dz = Guard(P.shape, O.STORAGE, device)
        assert _rc(L, "ocr_relu_bwd_f16", _dev(P.a[1], device), D.da, I64(npix * c), dz) == OK
        _bits_equal(dz.np(), np.where(P.a[1] > 0, P.da, f32(0)), "relu_bwd")
        acc = Guard(P.shape, O.STORAGE, device, P.y)
        assert _rc(L, "ocr_add_inplace_f16", acc, D.da, I64(npix * c)) == OK
        ref = P.y.astype(f64) + P.da
        if exact:
            _eq16(acc.np(), ref, "add_inplace")
        else:
            worst["add_inplace"] = _r16(acc.np(), ref, np.abs(P.y.astype(f64)) + np.abs(P.da.astype(f64)))
        torch.cuda.synchronize()
        for entry, r in worst.items():
            _note(entry, P.row, r)


def _unpool(x):
    """out[2i] = in[i], out[2i+1] = (in[i] + in[min(i+1, H-1)]) / 2, separably (float64)"""
    def up(a, ax):
        nxt = np.concatenate([np.take(a, range(1, a.shape[ax]), ax), np.take(a, [a.shape[ax] - 1], ax)], ax)
        out = np.stack([a, (a + nxt) / 2], ax + 1)
        shp = list(a.shape)
        shp[ax] *= 2
        return out.reshape(shp)
    return up(up(x.astype(f64), 2), 1)


def _unpool_T(dy, lh, lw):
    """the transpose of _unpool: weights 1, 1/2 to the next odd row (1 at the last), 1/2 from the previous odd row"""
    def down(a, ax, l):
        a = np.moveaxis(a, ax, 0)
        ev, od = a[0::2], a[1::2]
        g = ev + od * 0.5
        g[l - 1] += od[l - 1] * 0.5
        g[1:] += od[:-1] * 0.5
        return np.moveaxis(g, 0, ax)
    return down(down(dy.astype(f64), 1, lh), 2, lw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 24), (2, 4, 6, 128)], ids=["one_pixel", "c24", "c128"])
def test_unpool(device, shape, kind):
    """ocr_unpool_f16, ocr_unpool_bwd_f16 (accumulate 0 | 1) and ocr_unpool_add_stats_f16 (with / without partial)."""
    from tensorflow_ocr_amd import _lib as L
    n, lh, lw, c = shape
    H, W = 2 * lh, 2 * lw
    exact = kind == "exact"
    rng = _rng(shape, kind)
    draw = (lambda s: (rng.integers(-32, 33, s) / 8.0).astype(f32)) if exact else (lambda s: _h(rng.standard_normal(s)))
    x, dy, old, yold = draw(shape), draw((n, H, W, c)), draw(shape), draw((n, H, W, c))
    worst = {}
    out = Guard((n, H, W, c), O.STORAGE, device)
    assert _rc(L, "ocr_unpool_f16", _dev(x, device), n, lh, lw, c, out) == OK
    ref = _unpool(x)
    Mx = _unpool(np.abs(x))
    if exact:
        _eq16(out.np(), ref, "unpool")
    else:
        worst["unpool"] = _r16(out.np(), ref, 3 * Mx)                 # top + (bot - top) * wy: each value enters up to three times
    for accumulate in (0, 1):
        dx = Guard(shape, O.STORAGE, device, old)
        assert _rc(L, "ocr_unpool_bwd_f16", _dev(dy, device), n, lh, lw, c, dx, accumulate) == OK
        ref = _unpool_T(dy, lh, lw) + (old if accumulate else 0)
        M = _unpool_T(np.abs(dy), lh, lw) + np.abs(old)
        if exact:
            _eq16(dx.np(), ref, "unpool_bwd")
        else:
            worst["unpool_bwd"] = max(worst.get("unpool_bwd", 0), _r16(dx.np(), ref, M))
    npix = n * H * W
    pow2 = (c // 8) & (c // 8 - 1) == 0
    for with_partial in (0, 1):
        yb = Guard((n, H, W, c), O.STORAGE, device, yold)
        if not pow2:
            part = Guard((4, 2, c), torch.float32, device)
            assert _rc(L, "ocr_unpool_add_stats_f16", _dev(x, device), n, lh, lw, c, yb, part) == UNSUPPORTED
            assert part.untouched() and np.array_equal(yb.np(), yold)
            continue
        lanes = 256 // (c // 8)
        T = L.call_int("ocr_channel_stats_num_partials", I64(npix), ctypes.c_int(c))
        assert T == min(-(-npix // lanes), 2048)
        part = Guard((T, 2, c), torch.float32, device) if with_partial else None
        assert _rc(L, "ocr_unpool_add_stats_f16", _dev(x, device), n, lh, lw, c, yb, part) == OK
        got = yb.np()
        ref = yold.astype(f64) + _unpool(x)
        if exact:
            _eq16(got, ref, "unpool_add")
        else:
            worst["unpool_add_stats"] = max(worst.get("unpool_add_stats", 0), _r16(got, ref, np.abs(yold) + 3 * Mx))
        if part:                                                       # statistics of the STORED result
            g64 = got.astype(f64).reshape(-1, c)
            pg = part.np().astype(f64)
            m = _chain(npix, T, lanes)
            r = max(_rsum(pg[:, 0].sum(0), g64.sum(0), m, np.abs(g64).sum(0)), _rsum(pg[:, 1].sum(0), (g64 * g64).sum(0), m, (g64 * g64).sum(0)))
            if exact:
                assert r == 0.0
            else:
                worst["unpool_add_stats"] = max(worst["unpool_add_stats"], r)
    torch.cuda.synchronize()
    for entry, r in worst.items():
        _note(entry, "x".join(map(str, shape)), r)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("row", BWD_ROWS)
@pytest.mark.parametrize("kind", KINDS)
def test_backward(device, row, kind):
    """ocr_bn_relu_bwd_f16 (pool 0; pool 2 with da_full NULL and given), ocr_bn_relu_bwd_reduce_f16 (with / without
    da_pool), ocr_bn_relu_bwd_apply_f16, ocr_bn_relu_pool_bwd_idx_f16, ocr_bn_relu_pool_bwd_idx_apply_f16."""
    from tensorflow_ocr_amd import _lib as L
    exact = kind == "exact"
    big = row in ("c2048_cap", "tickets_c64")
    for i in range(len(ROWS[row][0])):
        P = _prep(row, i, kind)
        n, h, w, c, oh, ow = P.n, P.h, P.w, P.c, P.oh, P.ow
        N = n * h * w
        D = _bn_args(P, device)
        lanes = 256 // (c // 8)
        T = {0: L.call_int("ocr_bn_bwd_num_partials", n, h, w, c, 0), 2: L.call_int("ocr_bn_bwd_num_partials", n, h, w, c, 2)}
        assert T[0] == bwd_blocks(N, c) and T[2] == bwd_blocks(n * oh * ow, c)
        if row == "c2048_cap":
            assert (lanes, N, T[0]) == (1, 2070, 2048)
        if row == "tickets_c64":
            assert (T[0], red_rows(T[0]), -(-T[0] // 256), T[0] - 4 * 256) == (1049, 256, 5, 25) and (T[2], red_rows(T[2])) == (265, 320)
        if row == "tiny_c8":
            assert (lanes, N, T[0]) == (256, 15, 1)
        worst = {}

        def sums_chk(entry, dg, db, ref, m):
            rb, rg, ab, ag = ref
            if exact:
                assert np.array_equal(rb.astype(f32).astype(f64), rb) and np.array_equal(rg.astype(f32).astype(f64), rg)
                _bits_equal(db, rb.astype(f32), entry + " dbeta")
                _bits_equal(dg, rg.astype(f32), entry + " dgamma")
            else:
                worst[entry + "_sums"] = max(worst.get(entry + "_sums", 0), _rsum(db, rb, m, ab, P.okc), _rsum(dg, rg, m, ag, P.okc))

        def dy_chk(entry, got, dz, dza, dg, db):
            ref, M = _apply_ref(P, dz, dza, dg, db)
            skip = P.fe | ~P.okc[None, None, None, :]
            worst[entry] = max(worst.get(entry, 0), _r16(got, ref, M, skip))

        def outs():
            return Guard((c,), torch.float32, device), Guard((c,), torch.float32, device), Guard(P.shape, O.STORAGE, device)

        relus = (1,) if big else (0, 1)
        for relu in relus:
            forms = [(0, 1)] if row == "c2048_cap" else [(0, 1), (2, 0), (2, 1)]
            for pool, full in forms:
                dz, dza = _dz(P, relu, pool, full)
                ref = _sums(P, dz, dza)
                m = _chain(n * oh * ow if pool else N, T[pool], lanes)
                dg, db, dy = outs()
                part = Guard((T[pool], 2, c), torch.float32, device)
                ws, nb = _ws(L, T[pool], c, device)
                assert _rc(L, "ocr_bn_relu_bwd_f16", D.y, D.sc, D.sh, D.mu, D.inv, D.da if full else None, D.dap if pool else None,
                           n, h, w, c, relu, pool, dg, db, dy, part, ws, nb) == OK
                sums_chk("bn_relu_bwd", dg.np(), db.np(), ref, m)
                dy_chk("bn_relu_bwd", dy.np(), dz, dza, dg.np(), db.np())
                part.np()
                assert ws.ok()
                if pool == 2 and not full:
                    continue
                # the reduce-only entry: the same sums and the coefficients of dy = A dz + B y + C
                dg, db, _ = outs()
                co = {k: Guard((c,), torch.float32, device) for k in "ABC"}
                part = Guard((T[pool], 2, c), torch.float32, device)
                assert _rc(L, "ocr_bn_relu_bwd_reduce_f16", D.y, D.sc, D.sh, D.mu, D.inv, D.da, D.dap if pool else None, n, h, w, c, relu,
                           dg, db, co["A"], co["B"], co["C"], part, ws, nb) == OK
                sums_chk("bn_relu_bwd_reduce", dg.np(), db.np(), ref, m)
                # the coefficients from the sums the device holds: a few f32 operations each
                cb = _coef_bounds(db.np().astype(f64), dg.np().astype(f64), 0.0, 0.0, float(N), P.sc, P.mu, P.inv)
                r = max(_ratio(np.abs(co[k].np() - cb[k][0]), cb[k][1] + 1e-300) for k in "ABC")
                worst["bn_relu_bwd_reduce"] = max(worst.get("bn_relu_bwd_reduce", 0), r)
            # the apply-only entry: partials formed here (zero in the exact rows: dy = scale * dz exactly)
            dz, dza = _dz(P, relu, 0, 1)
            rng = np.random.default_rng(5)
            Tp = 3
            pp = np.zeros((Tp, 2, c), f32) if exact else rng.standard_normal((Tp, 2, c)).astype(f32)
            dg, db, dy = outs()
            ws, nb = _ws(L, Tp, c, device)
            assert _rc(L, "ocr_bn_relu_bwd_apply_f16", D.y, D.sc, D.sh, D.mu, D.inv, D.da, n, h, w, c, relu, _d32(pp, device), Tp,
                       dg, db, dy, ws, nb) == OK
            _bits_equal(db.np(), pp[:, 0].sum(0, dtype=f64).astype(f32), "apply dbeta")
            _bits_equal(dg.np(), pp[:, 1].sum(0, dtype=f64).astype(f32), "apply dgamma")
            if exact:
                _eq16(dy.np(), P.sc * dz, "bn_relu_bwd_apply routed dz")
            else:
                ref, M = _apply_ref(P, dz, dza, dg.np(), db.np())
                worst["bn_relu_bwd_apply"] = max(worst.get("bn_relu_bwd_apply", 0), _r16(dy.np(), ref, M, P.fe))
            if row == "c2048_cap":
                continue
            # the stored-index forms: the index bytes and y_pool come from the reference
            am = torch.from_numpy(_argmax_bytes(P, relu)).to(device)
            g = np.where(P.pool[relu] > 0, P.dap, f32(0)) if relu else P.dap
            dz = _route2(P.idx[relu], g.astype(f64), h, w)
            dza = np.abs(dz)
            ref = _sums(P, dz, dza)
            m = _chain(n * oh * ow, T[2], lanes)
            dg, db, dy = outs()
            part = Guard((T[2], 2, c), torch.float32, device)
            ws, nb = _ws(L, T[2], c, device)
            assert _rc(L, "ocr_bn_relu_pool_bwd_idx_f16", D.y, D.sc, D.mu, D.inv, None, am, D.dap, n, h, w, c, relu, dg, db, dy,
                       part, ws, nb) == OK
            sums_chk("bn_relu_pool_bwd_idx", dg.np(), db.np(), ref, m)
            ref_dy, M = _apply_ref(P, dz, dza, dg.np(), db.np())
            worst["bn_relu_pool_bwd_idx"] = max(worst.get("bn_relu_pool_bwd_idx", 0), _r16(dy.np(), ref_dy, M, ~P.okc[None, None, None, :] & np.ones(P.shape, bool)))
            # ... apply form: partial rows (sum dz, sum dz * xhat(y_pool)) per pooled image row, formed here from y_pool
            if exact:
                pp = np.zeros((n * oh, 2, c), f32)
            else:
                ypad = np.zeros((n, 2 * oh, 2 * ow, c), f64)
                ypad[:, :h, :w] = P.y
                cand = np.stack([ypad[:, 0::2, 0::2], ypad[:, 0::2, 1::2], ypad[:, 1::2, 0::2], ypad[:, 1::2, 1::2]], 0)
                ypool = np.take_along_axis(cand, P.idx[relu][None], 0)[0]
                g64 = g.astype(f64)
                pp = np.stack([g64.sum(2), (g64 * (ypool - P.mu) * P.inv).sum(2)], 2).reshape(n * oh, 2, c).astype(f32)
            Tp = n * oh
            dg, db, dy = outs()
            ws, nb = _ws(L, Tp, c, device)
            assert _rc(L, "ocr_bn_relu_pool_bwd_idx_apply_f16", D.y, D.sc, D.mu, D.inv, am, D.dap, n, h, w, c, relu, _d32(pp, device),
                       Tp, dg, db, dy, ws, nb) == OK
            _bits_equal(db.np(), pp[:, 0].sum(0, dtype=f64).astype(f32), "idx apply dbeta")
            _bits_equal(dg.np(), pp[:, 1].sum(0, dtype=f64).astype(f32), "idx apply dgamma")
            if exact:
                _eq16(dy.np(), P.sc * dz, "bn_relu_pool_bwd_idx_apply routed dz")
            else:
                # the partials formed from y_pool sum to the layer's sums (dz is zero off the first maxima)
                assert _rsum(db.np(), ref[0], 2, ref[2] + 1e-300) <= 1 and _rsum(dg.np(), ref[1], 2 + n * oh, ref[3] + 1e-300) <= 1
                ref_dy, M = _apply_ref(P, dz, dza, dg.np(), db.np())
                worst["bn_relu_pool_bwd_idx_apply"] = max(worst.get("bn_relu_pool_bwd_idx_apply", 0), _r16(dy.np(), ref_dy, M))
        torch.cuda.synchronize()
        for entry, r in worst.items():
            _note(entry, P.row, r)


# ------------------------------------------------------------------------------------------------ guests
@pytest.mark.parametrize("row", GUEST_ROWS)
@pytest.mark.parametrize("mw", [0, 256, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_guests(device, row, mw, kind):
    """The four guest entries with max_workgroups 0, 256 and 3 (3: every grid-stride loop runs past its first pass on
    the rows with more than 3 workgroups of units).  Coefficients are operands here: B = 0 in the exact rows.  The pooled
    forms accept even h and w only."""
    from tensorflow_ocr_amd import _lib as L
    exact = kind == "exact"
    P = _prep(row, 0, kind)
    n, h, w, c, oh, ow = P.n, P.h, P.w, P.c, P.oh, P.ow
    N = n * h * w
    D = _bn_args(P, device)
    even = h % 2 == 0 and w % 2 == 0
    lanes = 256 // (c // 4)
    rng = np.random.default_rng(zlib.crc32(row.encode()))
    if exact:
        cB, cC = np.zeros(c), rng.integers(-4, 5, c) / 4.0
    else:
        cB, cC = (rng.standard_normal(c) * 0.1).astype(f32).astype(f64), (rng.standard_normal(c) * 0.1).astype(f32).astype(f64)
    dB, dC = _d32(cB, device), _d32(cC, device)
    y64 = P.y.astype(f64)
    worst = {}

    def affine(entry, got, dz, dza, skip):
        ref = P.sc * dz + cB * y64 + cC
        if exact:
            _eq16(got, ref, entry, skip)
        else:
            worst[entry] = max(worst.get(entry, 0), _r16(got, ref, np.abs(P.sc) * dza + np.abs(cB * y64) + np.abs(cC), skip))

    def rows_chk(entry, part, dz, dza, m, skipc):
        got = part.np().astype(f64)
        s, q = dz.sum((0, 1, 2)), (dz * P.xh).sum((0, 1, 2))
        if exact:
            assert np.array_equal(q.astype(f32).astype(f64), q)
            _bits_equal(got[:, 0].sum(0).astype(f32), s.astype(f32), entry + " sum dz")
            _bits_equal(got[:, 1].sum(0).astype(f32), q.astype(f32), entry + " sum dz xhat")
        else:
            terms = P.inv * ((dza * np.abs(y64)).sum((0, 1, 2)) + np.abs(P.mu) * dza.sum((0, 1, 2)))
            worst[entry] = max(worst.get(entry, 0), _rsum(got[:, 0].sum(0), s, m, dza.sum((0, 1, 2)), skipc),
                               _rsum(got[:, 1].sum(0), q, m, terms, skipc))

    for relu in (0, 1):
        dz, dza = _dz(P, relu, 0, 1)
        dy = Guard(P.shape, O.STORAGE, device)
        assert _rc(L, "ocr_bn_relu_bwd_apply_affine_f16", D.y, D.da, D.sc, D.sh, dB, dC, n, h, w, c, relu, dy, mw) == OK
        affine("bn_relu_bwd_apply_affine", dy.np(), dz, dza, P.fe)
        # rows: one per thread lane of the launch
        R = int(L._fn("ocr_bn_relu_bwd_reduce_rows_count", ctypes.c_int)(n, h, w, c, 0, mw))
        cap = mw if 0 < mw < 256 else 256
        grid = max(1, min(-(-N // (lanes * 4)), cap))
        assert R == grid * lanes
        if mw == 3 and row != "tiny_c8":
            assert grid == 3 and N > 3 * lanes * 4                       # the loop's second pass runs
        part = Guard((R, 2, c), torch.float32, device)
        assert _rc(L, "ocr_bn_relu_bwd_reduce_rows_f16", D.y, D.da, None, None, D.sc, D.sh, D.mu, D.inv, n, h, w, c, relu, part, mw) == OK
        rows_chk("bn_relu_bwd_reduce_rows", part, dz, dza, _chain(N, grid, lanes), P.okc)
        # pooled forms
        am = torch.from_numpy(_argmax_bytes(P, relu)).to(device)
        dy = Guard(P.shape, O.STORAGE, device)
        co = (D.sc, dB, dC)
        rc = _rc(L, "ocr_bn_relu_pool_bwd_idx_apply_affine_f16", D.y, am, D.dap, *co, n, h, w, c, relu, dy, mw)
        if not even:
            assert rc == UNSUPPORTED and dy.untouched()
        else:
            assert rc == OK
            g = np.where(P.pool[relu] > 0, P.dap, f32(0)) if relu else P.dap
            dzp = _route2(P.idx[relu], g.astype(f64), h, w)
            affine("bn_relu_pool_bwd_idx_apply_affine", dy.np(), dzp, np.abs(dzp), np.zeros(P.shape, bool))
        dy = Guard(P.shape, O.STORAGE, device)
        rc = _rc(L, "ocr_bn_relu_poolfull_bwd_apply_affine_f16", D.y, D.da, D.dap, am, D.sc, D.sh, dB, dC, n, h, w, c, relu, dy, mw)
        Rp = int(L._fn("ocr_bn_relu_bwd_reduce_rows_count", ctypes.c_int)(n, h, w, c, 1, mw))
        part = Guard((max(Rp, 1), 2, c), torch.float32, device)
        rc2 = _rc(L, "ocr_bn_relu_bwd_reduce_rows_f16", D.y, D.da, D.dap, am, D.sc, D.sh, D.mu, D.inv, n, h, w, c, relu, part, mw)
        if not even or not relu:                                         # (no net builds a pooled end point without ReLU)
            assert rc == UNSUPPORTED and rc2 == UNSUPPORTED and dy.untouched() and part.untouched()
        else:
            assert rc == OK and rc2 == OK
            dzf, dzfa = _dz(P, relu, 2, 1)
            affine("bn_relu_poolfull_bwd_apply_affine", dy.np(), dzf, dzfa, P.fe)
            units = n * (h // 2) * (w // 2)
            grid = max(1, min(-(-units // lanes), cap))
            assert Rp == grid * lanes
            rows_chk("bn_relu_bwd_reduce_rows", part, dzf, dzfa, _chain(units, grid, lanes), P.okc)
    torch.cuda.synchronize()
    for entry, r in worst.items():
        _note(entry, "%s_mw%d" % (P.row, mw), r)


# ------------------------------------------------------------------------------------------------ general max-pool
@pytest.mark.parametrize("win,parity", POOL_CASES, ids=["%s_%s" % wm for wm in POOL_CASES])
@pytest.mark.parametrize("kind", KINDS)
def test_maxpool(device, win, parity, kind):
    """ocr_maxpool_f16, ocr_bn_relu_maxpool_f16, ocr_maxpool_bwd_f16 (stored index and x re-scan, accumulate 0 | 1) on one
    row per compiled instantiation of maxpool_bwd_idx_kernel and the run-time 5x5/3, SAME padding, windows half outside
    the map; ocr_bn_relu_bwd_reduce_pooled_f16 on 3x3/2 and 5x5/3 with and without da_full_out.  c24: three chunks per
    pixel — the pools must be right, the fused reduce must answer OCR_ERR_UNSUPPORTED."""
    from tensorflow_ocr_amd import _lib as L
    k, s = WINDOWS[win]
    shape = POOL_MAPS[parity]
    n, h, w, c = shape
    exact = kind == "exact"
    name = "%s_%s" % (win, parity)
    rng = _rng(win, parity, kind)
    P = NS(shape=shape, n=n, h=h, w=w, c=c)
    if exact:
        P.y = (rng.integers(-8, 9, shape) / 2.0).astype(f32)              # few values: ties in most windows
        P.sc, P.sh = rng.choice([0.5, 1.0, 2.0], c), rng.integers(-4, 5, c) / 4.0
        P.mu, P.inv = rng.integers(-2, 3, c) / 2.0, rng.choice([0.5, 1.0, 2.0], c)
        draw = lambda sh: (rng.integers(-32, 33, sh) / 8.0).astype(f32)
    else:
        P.y = _h(rng.standard_normal(shape))
        P.sc, P.sh = rng.uniform(0.5, 1.5, c).astype(f32).astype(f64), (rng.standard_normal(c) * 0.5).astype(f32).astype(f64)
        P.mu, P.inv = (rng.standard_normal(c) * 0.3).astype(f32).astype(f64), rng.uniform(0.5, 2, c).astype(f32).astype(f64)
        draw = lambda sh: _h(rng.standard_normal(sh) * 0.5)
    ref_y, idx, pads = _maxpool(P.y, k, s)
    oh, ow = idx.shape[1:3]
    assert pads == (_same(h, k, s)[1], _same(w, k, s)[1])
    dyv, old = draw(idx.shape), draw(shape)
    D = NS(y=_dev(P.y, device), sc=_d32(P.sc, device), sh=_d32(P.sh, device), mu=_d32(P.mu, device), inv=_d32(P.inv, device))
    geo = (n, h, w, c, k, s, pads[0], pads[1], oh, ow)
    worst = {}
    out, am = Guard(idx.shape, O.STORAGE, device), Guard(idx.shape, torch.uint8, device)
    assert _rc(L, "ocr_maxpool_f16", D.y, *geo, out, am) == OK
    _bits_equal(out.np(), ref_y, "maxpool")                               # a selection: exact in every row
    assert np.array_equal(am.np(), idx.astype(np.uint8))
    out = Guard(idx.shape, O.STORAGE, device)
    assert _rc(L, "ocr_maxpool_f16", D.y, *geo, out, None) == OK
    _bits_equal(out.np(), ref_y, "maxpool without index")
    # the batch-norm form: windows over the stored activation
    for relu in (0, 1):
        af, au = _act(P, "f", relu), _act(P, "u", relu)
        (pf, jf, _), (pu, ju, _), (pm, jm, _) = _maxpool(af, k, s), _maxpool(au, k, s), _maxpool(_act(P, "m", relu), k, s)
        fw = (pf != pu) | (jf != ju) | (pf != pm) | (jf != jm)
        assert fw.mean() <= 1e-3
        out, am = Guard(idx.shape, O.STORAGE, device), Guard(idx.shape, torch.uint8, device)
        assert _rc(L, "ocr_bn_relu_maxpool_f16", D.y, D.sc, D.sh, relu, *geo, out, am) == OK
        assert not ((am.np() != jf.astype(np.uint8)) & ~fw).any()
        if exact:
            _bits_equal(out.np(), pf, "bn_relu_maxpool", fw)
        else:
            worst["bn_relu_maxpool"] = max(worst.get("bn_relu_maxpool", 0), _r16(out.np(), pf, np.abs(pf) + 2 * np.abs(P.sh), fw))
    # backward: stored index and re-scan of x
    ref, M = _maxpool_bwd(idx, dyv.astype(f64), k, s, h, w, pads)
    amd = torch.from_numpy(idx.astype(np.uint8)).to(device)
    for route in ("index", "x"):
        for accumulate in (0, 1):
            dx = Guard(shape, O.STORAGE, device, old)
            assert _rc(L, "ocr_maxpool_bwd_f16", D.y if route == "x" else None, amd if route == "index" else None, _dev(dyv, device),
                       *geo, dx, accumulate) == OK
            r, m = (ref + old, M + np.abs(old)) if accumulate else (ref, M)
            if exact:
                _eq16(dx.np(), r, "maxpool_bwd %s" % route)
            else:
                worst["maxpool_bwd"] = max(worst.get("maxpool_bwd", 0), _r16(dx.np(), r, m))
    # the gather + batch-norm reduce in one pass
    if c == 24:
        o = {q: Guard((c,), torch.float32, device) for q in ("dg", "db", "A", "B", "C")}
        da_out, part, wsg = Guard(shape, O.STORAGE, device), Guard((8, 2, c), torch.float32, device), Guard((4096,), torch.uint8, device)
        assert _rc(L, "ocr_bn_relu_bwd_reduce_pooled_f16", D.y, D.sc, D.sh, D.mu, D.inv, _dev(dyv, device), amd, *geo, 1, da_out,
                   o["dg"], o["db"], o["A"], o["B"], o["C"], part, wsg, SZ(4096)) == UNSUPPORTED
        torch.cuda.synchronize()
        assert da_out.untouched() and part.untouched() and wsg.untouched() and all(g.untouched() for g in o.values())
    elif win in ("k3s2", "k5s3"):
        N = n * h * w
        lanes = 256 // (c // 8)
        T = bwd_blocks(N, c)
        g16 = _h(ref.astype(f32))                                         # the gathered gradient as it is stored
        z = _act(P, "f", 0)
        fe = (z != _act(P, "u", 0)) | ((z > 0) != (_act(P, "u", 0) > 0)) | (z != _act(P, "m", 0))
        okc = ~fe.any((0, 1, 2))
        assert fe.mean() <= 1e-3 and okc.mean() >= 0.75
        xh = (P.y.astype(f64) - P.mu) * P.inv
        for relu in (0, 1):
            dz = np.where(z > 0, g16, f32(0)).astype(f64) if relu else g16.astype(f64)
            null_sums = None
            for with_out in (0, 1):
                da_out = Guard(shape, O.STORAGE, device) if with_out else None
                o = {q: Guard((c,), torch.float32, device) for q in ("dg", "db", "A", "B", "C")}
                part = Guard((T, 2, c), torch.float32, device)
                ws, nb = _ws(L, T, c, device)
                assert _rc(L, "ocr_bn_relu_bwd_reduce_pooled_f16", D.y, D.sc, D.sh, D.mu, D.inv, _dev(dyv, device), amd, *geo, relu, da_out,
                           o["dg"], o["db"], o["A"], o["B"], o["C"], part, ws, nb) == OK
                if with_out:
                    if exact:
                        _eq16(da_out.np(), ref, "reduce_pooled routed gradient")
                    else:
                        worst["bn_relu_bwd_reduce_pooled"] = max(worst.get("bn_relu_bwd_reduce_pooled", 0), _r16(da_out.np(), ref, M))
                        # a gathered sum an f32 rounding away from a 16-bit tie may store the other neighbour: then
                        # the device's own stored gradient is what enters the sums
                        dz = np.where((z > 0) | (relu == 0), da_out.np(), f32(0)).astype(f64)
                rb, rg = dz.sum((0, 1, 2)), (dz * xh).sum((0, 1, 2))
                if exact:
                    _bits_equal(o["db"].np(), rb.astype(f32), "reduce_pooled dbeta")
                    _bits_equal(o["dg"].np(), rg.astype(f32), "reduce_pooled dgamma")
                elif with_out:
                    m = _chain(N, T, lanes)
                    worst["bn_relu_bwd_reduce_pooled_sums"] = max(worst.get("bn_relu_bwd_reduce_pooled_sums", 0),
                                                                  _rsum(o["db"].np(), rb, m, np.abs(dz).sum((0, 1, 2)), okc),
                                                                  _rsum(o["dg"].np(), rg, m, np.abs(dz * xh).sum((0, 1, 2)), okc))
                # da_full_out only adds a store: the sums and coefficients are the same numbers with and without it
                if not with_out:
                    null_sums = {q: o[q].np() for q in o}
                else:
                    for q in o:
                        assert np.array_equal(null_sums[q].view(np.int32), o[q].np().view(np.int32)), q
                cb = _coef_bounds(o["db"].np().astype(f64), o["dg"].np().astype(f64), 0.0, 0.0, float(N), P.sc, P.mu, P.inv)
                assert max(_ratio(np.abs(o[q].np() - cb[q][0]), cb[q][1] + 1e-300) for q in "ABC") <= 1
                assert ws.ok()
                part.np()
    torch.cuda.synchronize()
    for entry, r in worst.items():
        _note(entry, name, r)


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes(device):
    """NULL required pointers: OCR_ERR_INVALID_ARG; a short ws_bytes: OCR_ERR_WORKSPACE; c = 12, c = 4096 and (where
    documented) odd h or w: OCR_ERR_UNSUPPORTED; non-positive n, h, w: OCR_ERR_INVALID_ARG.  Nothing is written."""
    from tensorflow_ocr_amd import _lib as L
    n, h, w, c = 2, 4, 6, 64
    oh, ow = 2, 3
    full = torch.zeros((n, h, w, c), dtype=O.STORAGE, device=device)
    pooled = torch.zeros((n, oh, ow, c), dtype=O.STORAGE, device=device)
    am = torch.zeros((n, oh, ow, c), dtype=torch.uint8, device=device)
    v = torch.ones(c, dtype=torch.float32, device=device)
    T = 16
    partd = torch.zeros((T, 2, c), dtype=torch.float32, device=device)
    G = {k: Guard(s, d, device) for k, (s, d) in {
        "full": ((n, h, w, c), O.STORAGE), "pooled": ((n, oh, ow, c), O.STORAGE), "am": ((n, oh, ow, c), torch.uint8),
        "v0": ((c,), torch.float32), "v1": ((c,), torch.float32), "v2": ((c,), torch.float32), "v3": ((c,), torch.float32),
        "v4": ((c,), torch.float32), "part": ((64, 2, c), torch.float32), "ws": ((4096,), torch.uint8)}.items()}
    nb = SZ(4096)
    geo = (n, h, w, c)
    pg = (n, h, w, c, 2, 2, 0, 0, oh, ow)
    # entry: (arguments, indices of the required pointers, index of c or None, index of ws_bytes or None, index of n or None)
    E = {
        "ocr_bn_finalize": ([partd, T, c, DB(8.0), v, v, FL(1e-5), FL(0.9), None, None, G["v0"], G["v1"], None, None, G["ws"], nb], [0, 10, 11, 14], None, 15, None),
        "ocr_bn_inference_params": ([v, v, v, v, FL(1e-5), c, G["v0"], G["v1"]], [2, 3, 6, 7], None, None, None),
        "ocr_bn_bwd_sums": ([partd, T, c, G["v0"], G["v1"], G["ws"], nb], [0, 3, 4, 5], None, 6, None),
        "ocr_bn_bwd_coefficients": ([partd, T, c, DB(8.0), v, v, v, G["v0"], G["v1"], G["v2"], G["v3"], G["v4"], G["ws"], nb], [0, 4, 5, 6, 7, 8, 9, 10, 11, 12], None, 13, None),
        "ocr_bn_relu_f16": ([full, v, v, *geo, 1, 2, G["full"], G["pooled"]], [0, 1, 2, 10], 6, None, 3),
        "ocr_bn_relu_pool_idx_f16": ([full, v, v, *geo, 1, G["full"], G["pooled"], G["am"], None], [0, 1, 2, 9, 10], 6, None, 3),
        "ocr_bn_relu_bwd_f16": ([full, v, v, v, v, full, pooled, *geo, 1, 2, G["v0"], G["v1"], G["full"], G["part"], G["ws"], nb], [0, 1, 2, 3, 4, 6, 13, 14, 15, 16, 17], 10, 18, 7),
        "ocr_bn_relu_bwd_reduce_f16": ([full, v, v, v, v, full, None, *geo, 1, G["v0"], G["v1"], G["v2"], G["v3"], G["v4"], G["part"], G["ws"], nb], [0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17, 18], 10, 19, 7),
        "ocr_bn_relu_bwd_reduce_pooled_f16": ([full, v, v, v, v, pooled, am, *pg, 1, G["full"], G["v0"], G["v1"], G["v2"], G["v3"], G["v4"], G["part"], G["ws"], nb], [0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 22, 23, 24, 25], 10, 26, 7),
        "ocr_bn_relu_bwd_apply_f16": ([full, v, v, v, v, full, *geo, 1, partd, T, G["v0"], G["v1"], G["full"], G["ws"], nb], [0, 1, 2, 3, 4, 5, 11, 13, 14, 15, 16], 9, 17, 6),
        "ocr_bn_relu_pool_bwd_idx_f16": ([full, v, v, v, None, am, pooled, *geo, 1, G["v0"], G["v1"], G["full"], G["part"], G["ws"], nb], [0, 1, 2, 3, 5, 6, 12, 13, 14, 15, 16], 10, 17, 7),
        "ocr_bn_relu_pool_bwd_idx_apply_f16": ([full, v, v, v, am, pooled, *geo, 1, partd, T, G["v0"], G["v1"], G["full"], G["ws"], nb], [0, 1, 2, 3, 4, 5, 11, 13, 14, 15, 16], 9, 17, 6),
        "ocr_bn_relu_bwd_apply_affine_f16": ([full, full, v, v, v, v, *geo, 1, G["full"], 0], [0, 1, 2, 3, 4, 5, 11], 9, None, 6),
        "ocr_bn_relu_pool_bwd_idx_apply_affine_f16": ([full, am, pooled, v, v, v, *geo, 1, G["full"], 0], [0, 1, 2, 3, 4, 5, 11], 9, None, 6),
        "ocr_bn_relu_poolfull_bwd_apply_affine_f16": ([full, full, pooled, am, v, v, v, v, *geo, 1, G["full"], 0], [0, 1, 2, 3, 4, 5, 6, 7, 13], 11, None, 8),
        "ocr_bn_relu_bwd_reduce_rows_f16": ([full, full, None, None, v, v, v, v, *geo, 1, G["part"], 0], [0, 1, 4, 5, 6, 7, 13], 11, None, 8),
        "ocr_channel_stats_f16": ([full, I64(n * h * w), c, G["part"]], [0, 3], 2, None, None),
        "ocr_bn_add_relu_f16": ([full, v, v, full, None, None, I64(n * h * w), c, G["full"], None], [0, 1, 2, 3, 8], 7, None, None),
        "ocr_relu_bwd_f16": ([full, full, I64(n * h * w * c), G["full"]], [0, 1, 3], None, None, None),
        "ocr_add_inplace_f16": ([G["full"], full, I64(n * h * w * c)], [0, 1], None, None, None),
        "ocr_unpool_f16": ([pooled, n, oh, ow, c, G["full"]], [0, 5], 4, None, 1),
        "ocr_unpool_bwd_f16": ([full, n, oh, ow, c, G["pooled"], 0], [0, 5], 4, None, 1),
        "ocr_unpool_add_stats_f16": ([pooled, n, oh, ow, c, G["full"], G["part"]], [0, 5], 4, None, 1),
        "ocr_bias_relu_bwd_f16": ([full, full, I64(n * h * w), c, 1, G["full"], G["v0"], G["part"]], [0, 1, 5, 6, 7], 3, None, None),
        "ocr_maxpool_f16": ([full, *pg, G["pooled"], G["am"]], [0, 11], 4, None, 1),
        "ocr_bn_relu_maxpool_f16": ([full, v, v, 1, *pg, G["pooled"], G["am"]], [0, 1, 2, 14], 7, None, 4),
        "ocr_maxpool_bwd_f16": ([None, am, pooled, *pg, G["full"], 0], [1, 2, 13], 6, None, 3),
    }
    pow2_only = {"ocr_bn_relu_bwd_f16", "ocr_bn_relu_bwd_reduce_f16", "ocr_bn_relu_bwd_reduce_pooled_f16", "ocr_bn_relu_bwd_apply_f16",
                 "ocr_bn_relu_pool_bwd_idx_f16", "ocr_bn_relu_pool_bwd_idx_apply_f16", "ocr_bn_relu_bwd_apply_affine_f16",
                 "ocr_bn_relu_pool_bwd_idx_apply_affine_f16", "ocr_bn_relu_poolfull_bwd_apply_affine_f16", "ocr_bn_relu_bwd_reduce_rows_f16",
                 "ocr_channel_stats_f16", "ocr_unpool_add_stats_f16", "ocr_bias_relu_bwd_f16"}
    guests = {"ocr_bn_relu_bwd_apply_affine_f16", "ocr_bn_relu_pool_bwd_idx_apply_affine_f16",
              "ocr_bn_relu_poolfull_bwd_apply_affine_f16", "ocr_bn_relu_bwd_reduce_rows_f16"}
    for name, (args, req, ci, wi, ni) in E.items():
        for j in req:
            a = list(args)
            a[j] = None
            assert _rc(L, name, *a) == INVALID_ARG, (name, j)
        if wi is not None:
            a = list(args)
            a[wi] = SZ(7)
            assert _rc(L, name, *a) == WORKSPACE, name
        if ci is not None:
            bads = (12,) if name not in pow2_only else (12, 24, 4096, 2048) if name in guests else (12, 24, 4096)
            for bad in bads:                                             # 24: three chunks, no power of two; 2048: c / 4 > 256
                a = list(args)
                a[ci] = bad
                assert _rc(L, name, *a) == UNSUPPORTED, (name, bad)
        if ni is not None:
            for d in range(3):
                a = list(args)
                a[ni + d] = 0
                assert _rc(L, name, *a) == INVALID_ARG, (name, "nhw"[d])
    # odd h or w where the entry documents it: the pooled guests
    for name in ("ocr_bn_relu_pool_bwd_idx_apply_affine_f16", "ocr_bn_relu_poolfull_bwd_apply_affine_f16"):
        args, _, ci, _, _ = E[name]
        for d in (-2, -1):
            a = list(args)
            a[ci + d] = 5
            assert _rc(L, name, *a) == UNSUPPORTED, name
    a = list(E["ocr_bn_relu_bwd_reduce_rows_f16"][0])
    a[2], a[3], a[9] = pooled, am, 5
    assert _rc(L, "ocr_bn_relu_bwd_reduce_rows_f16", *a) == UNSUPPORTED
    for bad in (12, 24, 4096):
        assert int(L._fn("ocr_bn_bwd_num_partials", ctypes.c_int)(n, h, w, bad, 0)) == UNSUPPORTED
        assert int(L._fn("ocr_channel_stats_num_partials", ctypes.c_int)(I64(48), ctypes.c_int(bad))) == UNSUPPORTED
    torch.cuda.synchronize()
    for k, g in G.items():
        assert g.untouched(), k
    # and the same buffers take a well-formed call
    assert _rc(L, "ocr_bn_relu_f16", *E["ocr_bn_relu_f16"][0]) == OK
    torch.cuda.synchronize()
    assert bool((G["pooled"].t == 1).all()) and G["pooled"].ok()
