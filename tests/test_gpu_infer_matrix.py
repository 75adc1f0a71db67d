"""GPU: every entry of csrc/f32_infer.hip and csrc/f16x2_infer.hip (with the epilogue of csrc/f32_conv_ep.h) — the f32 and
f16x2 inference precisions, Graph(precision="f32" | "f16x2") — against a float64 (or stepwise-f32) restatement in NumPy
written in this file.  No device route is compared with another.  Every entry is called through ctypes on the library
tensorflow_ocr_amd.ops binds, the status of every call is asserted, every output and the split route's workspace sit
between sentinel bands and start NaN-filled (an accumulate row starts from its y_old: it works in place), and the
convolution descriptors are filled field by field (oh, ow, pad_top, pad_left included), so asymmetric pads and kh != kw
are reached.

Kernels and the rows that reach them
  conv_f32_mfma_kernel        test_conv[mfma-*]: MFMA_ROWS x kinds exact | random (| wide on `wide`) x FLAGSETS through
                              ocr_conv2d_f32_mfma (the 8 subsets of BIAS | RELU | ACCUM_F16) and ocr_conv2d_f32_mfma_ep (every
                              flag alone and the layers' combinations); test_conv_nan, test_affine_expression, test_conv_status
  pack_split_kernel, conv_f32_split_kernel<1>, conv_f32_split_kernel<2>
                              test_conv[split-*]: SPLIT_ROWS likewise through ocr_conv2d_f32_split / _split_ep; <1> at cout <=
                              64, <2> above; test_conv_nan, test_affine_expression, test_conv_status.  pack_split_kernel's own
                              capped grid needs 16.7 M packed vectors (134 M weights): larger than any row allowed here.
  prep_images_f32_kernel      test_prep_images (npix 1 | 255 | 256 | 257), test_stream_cap[prep]
  bn_relu_f32_kernel          test_bn_relu (pool 0 | 2 x relu 0 | 1 x a_full given or not; maps 1x1, 5x7, 8x8; c 1 | 3 | 64 |
                              257), test_pool_nan, test_affine_expression, test_stream_cap[bn_relu], [bn_relu_pool]
  bn_add_relu_f32_kernel      test_bn_add_relu (npix * c 1 | 255 | 1025 ..., c 1 | 3 | 64), test_bn_add_relu_nan,
                              test_stream_cap[bn_add_relu]
  maxpool_f32_kernel          test_maxpool (2x2/2, 3x3/2, 3x3/1 SAME, 1x1/2; odd and even maps; c 1 | 24; -inf; signed zeros),
                              test_pool_nan, test_stream_cap[maxpool]
  subsample_f32_kernel<4>     test_subsample c = 64 aligned;  subsample_f32_kernel<1>: c = 64 with x or y at a 4-byte offset,
                              c = 18; test_stream_cap[subsample] (<1>, c = 1)
  unpool_f32_kernel           test_unpool (1x1, 3x5, 4x4 x c 1 | 5), test_stream_cap[unpool]
  channel_stats_f32_kernel    test_channel_stats (npix 1 | 63 | 64 | 65 | 130 | 65537 x c 1 | 3 | 256 | 300) with
                              ocr_channel_stats_f32_num_partials.  It launches T <= 1024 blocks and never goes through vgrid.
  every OCR_CHECK_ARG / OCR_CHECK_SHAPE: test_conv_status, test_elementwise_status, test_maxpool_status_empty_input
  ocr_conv2d_f32_split_workspace: its closed form on every conv row (test_conv), 0 for invalid descriptors (test_conv_status)

Bounds (u = 2^-24, g(m) = m u / (1 - m u); all per element, none tuned)
  MFMA route.  The kernel evaluates sum_k x_k w_k (K = kh kw cin terms, any order, each product and each addition one f32
    rounding at the most) and then s epilogue operations, each one rounding: ACCUM_IN 1, AFFINE 2, BIAS 1, RESIDUAL 1, RELU
    0 (1-Lipschitz, exact), ACCUM_F16 1.  With M the sum of the magnitudes of every term — sum |x w| carried through
    |scale|, plus |shift|, |bias|, |residual|, |y_old| — the standard result for any summation order gives
    |dev - ref| <= g(K + s) M.
  Split route, (a) device against the emulated split sum.  The test forms the planes as split1 does, hi = f16(clamp v),
    lo' = f16(clamp((v - hi) 2^11)) (NumPy's cast rounds to nearest even like v_cvt_f16_f32), and evaluates in float64
    S = sum xhi whi + 2^-11 (xhi wlo' + xlo' whi).  A product of two halves has 22 significant bits and is exact in f32,
    so the device differs from S by the accumulation of 3K terms, the join main + corr 2^-11 (one addition; the product by
    2^-11 is exact) and the epilogue alone: |dev - S'| <= g(3K + 1 + s) M' with M' the magnitudes of the 3K terms carried
    through the epilogue as above.
  Split route, (b) S against the true float64 convolution, from the reference alone.  Write v = hi + lo (lo exact in f32),
    a = u16 / (1 + u16), u16 = 2^-11.  |lo| <= a |v| for |v| >= 2^-14 (round to nearest of a normal half), <= 2^-25 below
    (half subnormal spacing 2^-24).  2^-11 lo' = lo + e with |e| <= a |lo| when lo' is a normal half and <= 2^-36 when it
    is a half subnormal (spacing 2^-24, times 2^-11, halved).  x w - (xhi whi + xhi wlo~ + xlo~ whi) = xlo wlo - xhi e_w -
    e_x whi, so per product |diff| <= XL WL + XH WE + XE WH with XL, XE the bounds on |lo|, |e| just given and XH = |x| +
    XL.  For operands with normal planes that is a^2 (3 + 2a) |x w| < 3 u16^2 |x w| = 3 2^-22 |x w|; an operand whose lo'
    is a half subnormal adds at most 2^-36 (1 + a) times the other factor.  test_conv asserts the sum of these per-product
    bounds, and on every row without such an operand that it is below 3 2^-22 sum |x w|.
  Exact rows.  x = k / 8 (|k| <= 32), w in {0, +-0.5, +-1, +-2}, epilogue operands k / 8 and scales in {0.5, 1, 2}: every
    product is a multiple of 2^-4, every partial sum far below 2^20, lo' = 0 on the split route; both routes must match the
    float64 value bit for bit, a zero's sign apart.
  Step order.  Random rows draw |scale| in [0.5, 0.8] or [1.3, 2] with either sign and the other operands N(0, 1): for every
    pair of adjacent steps taken (two additions commute and are left out) the reference with the two swapped differs
    from the reference by more than 100 bounds somewhere in the map; asserted from the reference alone on rows of >= 64
    outputs.
  Wide rows take the operand distribution of test_gpu_f16x2.py::test_conv_f32_split_dynamic_range (x = N(0,1) 10^U(-6,2),
    w = N(0,1) / sqrt(K) 10^U(-3,0), as drawn and times 2^-10) at K <= 96, held to the bounds above.
  Element-wise kernels.  Stepwise f32 in NumPy, bit for bit.  y * scale + shift may be contracted to one fma or not: the
    reference is evaluated both ways (fused: one rounding, through an error-free float64 sum; unfused: two) and each launch
    must equal ONE of them in every element; which one is printed (`infer affine-expression ...`).  The plain entry and the
    AFFINE epilogue of both routes must pick the same (test_affine_expression).  Maxima are exact; under ties the first
    maximum is kept, which shows only in a zero's sign (test_maxpool pins it with +0 / -0 windows, compared with the sign).
    The unpool's products are by 0.5 or 0: exact, so contraction cannot change a bit; operands stay in [2^-100, 2^100].
  channel_stats: sums in double, rounded once: |partial - ref| <= u |ref| + n_strip 2^-53 sum |term|.
  stream_cap rows: more than 65536 * 256 work items, operands k / 8 from a keyed integer pattern made on the device and
    restated on the host, comparison exact.

Findings
  * bn_add_relu_f32_kernel ended in `v > 0 ? v : 0`: a NaN came out as 0, while the fused form (AFFINE | RESIDUAL | RELU)
    keeps it.  Now `v < 0 -> 0` (test_bn_add_relu_nan).
  * maxpool_f32_kernel and the pooled branch of bn_relu_f32_kernel dropped a NaN in the window (`v > m ? v : m`; an all-NaN
    window gave -inf).  Now a NaN in the window gives NaN (test_pool_nan, each of the four positions).
  * The four conv entries masked unknown bits out of d->flags and ignored d->flip_taps: OCR_CONV_STATS or flip_taps = 1 got
    a plain forward convolution and status 0.  Now OCR_ERR_INVALID_ARG (test_conv_status); no caller in ops.py /
    layers_f32.py set either.
  * ocr_maxpool_f32 did not check h and w: h = 0 returned 0 and filled y with -inf.  Now OCR_ERR_INVALID_ARG
    (test_maxpool_status_empty_input).
  * ocr_conv2d_f32_split[_ep] answered a short workspace with OCR_ERR_INVALID_ARG; every other workspace of the ABI
    answers OCR_ERR_WORKSPACE.  Now OCR_ERR_WORKSPACE (test_conv_status); a misaligned one stays OCR_ERR_INVALID_ARG.

MEASURED (largest |err| / bound over the rows and flag sets, f16 / bf16 library, from the `infer <entry> <row> ratio=` lines)
  conv2d_f32_mfma       random 0.382 / 0.382   wide 0.128 / 0.128      conv2d_f32_split      random 0.116 / 0.116   wide 0.316 / 0.316
  conv2d_f32_mfma_ep    random 0.382 / 0.382   wide 0.092 / 0.092      conv2d_f32_split_ep   random 0.103 / 0.103   wide 0.316 / 0.316
  NaN rows (the elements that stay finite): mfma_ep 0.017 / 0.017, split_ep 0.005 / 0.005
  channel_stats_f32     0.996 / 0.996 (a sum right to the last bit still shows its one rounding, up to u |ref|)
  Exact rows and every element-wise row: bit for bit.  y * scale + shift is evaluated FUSED (one fma) by every launch of
  bn_relu_f32_kernel, bn_add_relu_f32_kernel and the AFFINE epilogue of both routes (96 `infer affine-expression` lines say
  fused, 9 either: one-element rows on which the two evaluations coincide; none unfused).
  These kernels read no 16-bit operand and are compiled from the same source in both libraries: the two columns agree to
  every printed digit.  The largest conv ratios belong to the shortest sums (K = 1, 3: P1, P31), where g(K + s) counts
  few roundings; long sums stay far below their bound (random signs).  The split route's largest is the wide row times
  2^-10 at the 128 x 128 tile.  No row was over its bound.  On the host, test_infer_matrix_host.py: the faithful f32
  emulation in another order reaches 0.13 of bound (a), an emulation without one correction product 49 .. 303 times the
  bound, without the 2^-11 more than 10^5 times; |S - conv| reaches 0.49 of bound (b).
  Time on the MI355X: the file's tests 6 s per library; slowest test_stream_cap[bn_relu_pool] 0.9 s (67 M inputs, most of
  it the host pattern and pooling), [prep] 0.6 s; no stream_cap row had to shrink.
"""
import ctypes
from ctypes import byref
from functools import lru_cache, partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (FL, I64, INVALID_ARG, NAN32, OK, SZ, UNSUPPORTED, WORKSPACE, Guard, _bits_equal, _cdiv, _g,
                            _lib, _ratio, _raw, _rc, _rng, bands_untouched, carve, f32, f64, untouched)

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "infer")
BIAS, RELU, STATS, ACCUM_F16, AFFINE, RESIDUAL, ACCUM_IN = 1, 2, 4, 8, 16, 32, 64
PLAIN_SETS = [0, BIAS, RELU, ACCUM_F16, BIAS | RELU, BIAS | ACCUM_F16, RELU | ACCUM_F16, BIAS | RELU | ACCUM_F16]
EP_SETS = [BIAS, RELU, ACCUM_F16, AFFINE, RESIDUAL, ACCUM_IN, AFFINE | RELU, ACCUM_IN | AFFINE | RELU,
           AFFINE | RESIDUAL | RELU, AFFINE | BIAS | RESIDUAL | RELU | ACCUM_F16]
STEPS = ((ACCUM_IN, 1), (AFFINE, 2), (BIAS, 1), (RESIDUAL, 1), (RELU, 0), (ACCUM_F16, 1))      # (flag, f32 operations)
ADDS = (ACCUM_IN, BIAS, RESIDUAL, ACCUM_F16)
U11 = 2.0 ** -11
BANDF = 128                             # floats on each side of a carved buffer
CONV_ENTRY = {("mfma", False): "ocr_conv2d_f32_mfma", ("mfma", True): "ocr_conv2d_f32_mfma_ep",
              ("split", False): "ocr_conv2d_f32_split", ("split", True): "ocr_conv2d_f32_split_ep"}


# ------------------------------------------------------------------------------------------------ conv rows
def _same(size, k, stride, rate):
    """TF SAME: output extent and the pad before (the smaller half)"""
    o = _cdiv(size, stride)
    return o, max((o - 1) * stride + (k - 1) * rate + 1 - size, 0) // 2


def _row(rid, n, h, w, cin, cout, kh, kw, stride=1, rate=1, geom=None, mis=None):
    oh, pt = _same(h, kh, stride, rate)
    ow, pl = _same(w, kw, stride, rate)
    if geom is not None:
        oh, ow, pt, pl = geom
    return NS(id=rid, n=n, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, rate=rate, oh=oh, ow=ow, pt=pt, pl=pl,
              mis=mis, P=n * oh * ow, K=kh * kw * cin)


GEOMETRY = [            # shared by both routes: (id, n, h, w, kh, kw, stride, rate, geom)
    ("k1x3", 1, 6, 7, 1, 3, 1, 1, None),
    ("k3x1", 1, 7, 6, 3, 1, 1, 1, None),
    ("k7s2_same", 1, 8, 10, 7, 7, 2, 1, None),          # pads 2 | 3 on both axes
    ("k3r6_5x5", 1, 5, 5, 3, 3, 1, 6, None),            # every tap but the centre outside
    ("k3s2_odd", 1, 7, 9, 3, 3, 2, 1, None),
    ("k3x2_asym", 1, 6, 5, 3, 2, 1, 1, (5, 5, 0, 1)),   # pad_top 0, pad_left 1, taps beyond the bottom edge
    ("n2_9x9", 2, 9, 9, 3, 3, 1, 1, None),              # P = 162: the first 128-pixel tile straddles the images
]
MFMA_ROWS = [
    _row("P1", 1, 1, 1, 1, 1, 1, 1),
    _row("P31", 1, 1, 31, 3, 3, 1, 1),
    _row("P127", 1, 1, 127, 15, 63, 1, 1),
    _row("P128", 1, 8, 16, 16, 64, 1, 1),
    _row("P129", 1, 3, 43, 17, 65, 1, 1),
    _row("c18_66", 1, 4, 5, 18, 66, 3, 3),
    _row("c20_68", 1, 5, 7, 20, 68, 3, 3),
] + [_row(g[0], g[1], g[2], g[3], 4 + 4 * (i % 2), 8 + 4 * (i % 3), g[4], g[5], g[6], g[7], g[8]) for i, g in enumerate(GEOMETRY)] + [
    _row("mis_" + m, 1, 6, 6, 8, 8, 3, 3, mis=m) for m in ("x", "w", "y", "r")] + [
    _row("wide", 1, 8, 8, 10, 16, 3, 3)]                # K = 90
SPLIT_ROWS = [
    _row("P1", 1, 1, 1, 1, 1, 1, 1),
    _row("P255", 1, 15, 17, 7, 64, 1, 1),
    _row("P256", 1, 16, 16, 8, 64, 1, 1),
    _row("P257", 1, 1, 257, 9, 33, 1, 1),
    _row("P127", 1, 1, 127, 31, 65, 1, 1),
    _row("P128", 1, 8, 16, 32, 128, 1, 1),
    _row("P129", 1, 3, 43, 33, 129, 1, 1),
    _row("c36_130", 1, 4, 5, 36, 130, 3, 3),
    _row("c40_192", 1, 5, 7, 40, 192, 1, 1),            # second 128-cout tile: its upper wave column has no cout
] + [_row(g[0], g[1], g[2], g[3], 8 + 8 * (i % 2), 8 + 4 * (i % 3), g[4], g[5], g[6], g[7], g[8]) for i, g in enumerate(GEOMETRY)] + [
    _row("mis_" + m, 1, 6, 6, 8, 8, 3, 3, mis=m) for m in ("x", "w", "y", "r")] + [
    _row("wide", 1, 8, 8, 96, 16, 1, 1),                # K = 96
    _row("wide3", 1, 6, 6, 10, 72, 3, 3)]               # K = 90, the 128 x 128 tile
ROWS = {"mfma": {r.id: r for r in MFMA_ROWS}, "split": {r.id: r for r in SPLIT_ROWS}}
CONV_CASES = [(route, rid, kind) for route in ("mfma", "split") for rid in ROWS[route]
              for kind in (("exact", "random", "wide", "wide_2^-10") if rid.startswith("wide") else ("exact", "random"))]


def _desc(L, r, flags=0):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.oh, d.ow, d.cout = r.n, r.h, r.w, r.cin, r.oh, r.ow, r.cout
    d.kh, d.kw, d.stride, d.dilation, d.pad_top, d.pad_left, d.flip_taps, d.flags = r.kh, r.kw, r.stride, r.rate, r.pt, r.pl, 0, flags
    return d


def _operands(route, r, kind):
    """the operands of one (route, row, kind), f32; the key is part of the test"""
    rng = _rng("infer", route, r.id, kind)
    xs, ws, os_ = (r.n, r.h, r.w, r.cin), (r.kh, r.kw, r.cin, r.cout), (r.n, r.oh, r.ow, r.cout)
    if kind == "exact":
        o = NS(x=rng.integers(-32, 33, xs) / 8.0, w=rng.choice([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], ws),
               scale=rng.choice([0.5, 1.0, 2.0], r.cout), shift=rng.integers(-32, 33, r.cout) / 8.0,
               bias=rng.integers(-32, 33, r.cout) / 8.0, res=rng.integers(-32, 33, os_) / 8.0, y0=rng.integers(-32, 33, os_) / 8.0)
    else:
        if kind == "random":
            x, w = rng.standard_normal(xs), rng.standard_normal(ws) / np.sqrt(r.K)
        else:
            fac = 1.0 if kind == "wide" else 2.0 ** -10
            x = rng.standard_normal(xs) * 10.0 ** rng.uniform(-6, 2, xs) * fac
            w = rng.standard_normal(ws) / np.sqrt(r.K) * 10.0 ** rng.uniform(-3, 0, ws) * fac
        mag = np.where(rng.random(r.cout) < 0.5, rng.uniform(0.5, 0.8, r.cout), rng.uniform(1.3, 2.0, r.cout))
        o = NS(x=x, w=w, scale=mag * rng.choice([-1.0, 1.0], r.cout), shift=rng.standard_normal(r.cout),
               bias=rng.standard_normal(r.cout), res=rng.standard_normal(os_), y0=rng.standard_normal(os_))
    for k, v in vars(o).items():
        setattr(o, k, np.ascontiguousarray(v, dtype=f32))
    return o


def _cols(x, r, fill=0.0):
    """[P][kh kw cin]: the taps of every output pixel in the HWIO order, `fill` outside the image"""
    out = np.empty((r.n, r.oh, r.ow, r.kh * r.kw, r.cin), x.dtype)
    oy, ox = np.arange(r.oh) * r.stride - r.pt, np.arange(r.ow) * r.stride - r.pl
    for ky in range(r.kh):
        for kx in range(r.kw):
            iy, ix = oy + ky * r.rate, ox + kx * r.rate
            inside = ((iy >= 0) & (iy < r.h))[:, None] & ((ix >= 0) & (ix < r.w))[None, :]
            g = x[:, np.clip(iy, 0, r.h - 1)][:, :, np.clip(ix, 0, r.w - 1)]
            out[:, :, :, ky * r.kw + kx] = np.where(inside[None, :, :, None], g, fill)
    return out.reshape(r.P, r.K)


def split_planes(v):
    """split1 of f16x2_infer.hip on the host -> (hi, lo') as float64"""
    v = np.asarray(v, f32)
    hi = np.clip(v, f32(-65504), f32(65504)).astype(np.float16)
    lo = np.clip((v - hi.astype(f32)) * f32(2048), f32(-65504), f32(65504)).astype(np.float16)
    return hi.astype(f64), lo.astype(f64)


def split_sum(x, w, r, terms=(1, 1, 1), corr=U11):
    """-> (S, sum of |terms|): the split route's sum in float64; `terms` switches (xhi whi, xhi wlo', xlo' whi) on and off
    and `corr` is the weight of the correction products, so that test_infer_matrix_host.py can break it on purpose"""
    xh, xl = split_planes(x)
    wh, wl = (p.reshape(r.K, r.cout) for p in split_planes(w))
    ch, cl = _cols(xh, r), _cols(xl, r)
    S = terms[0] * (ch @ wh) + corr * (terms[1] * (ch @ wl) + terms[2] * (cl @ wh))
    return S, np.abs(ch) @ np.abs(wh) + U11 * (np.abs(ch) @ np.abs(wl) + np.abs(cl) @ np.abs(wh))


def split_truncation_bound(x, w, r):
    """bound (b) of the docstring -> (bound, True when no operand has a subnormal plane)"""
    a = U11 / (1 + U11)

    def parts(v):
        v64 = np.abs(np.asarray(v, f64))
        assert v64.max() < 65504
        lo = np.abs(split_planes(v)[1])
        VL = np.where(v64 >= 2.0 ** -14, a * v64, np.where(v64 > 0, 2.0 ** -25, 0.0))
        sub = (lo < 2.0 ** -14) & (VL > 0)
        VE = np.where(sub, np.where(np.asarray(v, f32).astype(np.float16).astype(f64) == np.asarray(v, f64), 0.0, 2.0 ** -36), a * VL)
        return VL, v64 + VL, VE, bool(((v64 < 2.0 ** -14) & (v64 > 0)).any() or (sub & (VE > 0)).any())
    XL, XH, XE, xs = parts(x)
    WL, WH, WE, ws = (p.reshape(r.K, r.cout) if isinstance(p, np.ndarray) else p for p in parts(w))
    return _cols(XL, r) @ WL + _cols(XH, r) @ WE + _cols(XE, r) @ WH, not (xs or ws)


def _epilogue(v, m, flags, o, order=STEPS):
    """the steps of f32_conv_ep.h on the float64 sum v and its magnitude m -> (value, magnitude, f32 operations)"""
    s = 0
    for flag, ops_ in order:
        if not flags & flag:
            continue
        s += ops_
        if flag in (ACCUM_IN, ACCUM_F16):
            v, m = v + o.y0, m + np.abs(o.y0)
        elif flag == AFFINE:
            v, m = v * o.scale + o.shift, m * np.abs(o.scale) + np.abs(o.shift)
        elif flag == BIAS:
            v, m = v + o.bias, m + np.abs(o.bias)
        elif flag == RESIDUAL:
            v, m = v + o.res, m + np.abs(o.res)
        else:
            v = np.where(v < 0, 0.0, v)                  # a NaN stays NaN
    return v, m, s


def _swaps(flags):
    """STEPS with two adjacent taken steps swapped, for every such pair but two additions, which commute"""
    taken = [i for i, (f, _) in enumerate(STEPS) if flags & f]
    for a, b in zip(taken, taken[1:]):
        if STEPS[a][0] in ADDS and STEPS[b][0] in ADDS:
            continue
        order = list(STEPS)
        order[a], order[b] = order[b], order[a]
        yield order


@lru_cache(maxsize=None)
def _case(route, rid, kind):
    """operands and the float64 references of one row, computed once: conv (value, magnitudes), f32 operations of the sum"""
    r = ROWS[route][rid]
    o = _operands(route, r, kind)
    o64 = NS(**{k: v.astype(f64) for k, v in vars(o).items()})
    o64.res, o64.y0 = o64.res.reshape(r.P, r.cout), o64.y0.reshape(r.P, r.cout)
    cx, w2 = _cols(o64.x, r), o64.w.reshape(r.K, r.cout)
    true, mag = cx @ w2, np.abs(cx) @ np.abs(w2)
    if route == "mfma":
        return r, o, o64, true, mag, r.K
    S, Smag = split_sum(o.x, o.w, r)
    bound_b, ordinary = split_truncation_bound(o.x, o.w, r)
    assert (np.abs(S - true) <= bound_b).all(), "bound (b): the split sum against the float64 convolution"
    if ordinary:
        assert (bound_b <= 3 * 2.0 ** -22 * mag).all()
    if kind == "exact":
        assert np.array_equal(S, true)
    return r, o, o64, S, Smag, 3 * r.K + 1


class Box:
    """an f32 device buffer carved between sentinel bands, NaN-filled or holding `fill`; off = 1 puts it at a 4-byte
    offset from 16-byte alignment inside four spare NaN words that must stay NaN"""

    def __init__(self, shape, device, fill=None, off=0):
        numel = int(np.prod(shape))
        self.guard, T = carve((numel + (4 if off else 0),), torch.float32, BANDF, device)
        self.t = T[off:off + numel].view(*shape)
        self.spare = (T[:off], T[off + numel:])
        assert self.t.data_ptr() % 16 == 4 * off
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=f32)).view(*shape))

    def intact(self):
        return bands_untouched(self.guard) and all(untouched(s) for s in self.spare)

    def untouched(self):
        return self.intact() and untouched(self.t)

    def get(self):
        assert self.intact(), "written outside the buffer"
        return self.t.cpu().numpy()


def _workspace(L, d, device):
    nbytes = int(L._fn("ocr_conv2d_f32_split_workspace", SZ)(byref(d)))
    guard, t = carve((max(nbytes, 16) // 2,), torch.float16, 256, device)
    return nbytes, guard, t


def _launch(L, ops, route, d, x, w, y, o_dev, ws, use_ep):
    """one conv call -> status; o_dev: device tensors of the epilogue operands (None where absent)"""
    name = CONV_ENTRY[route, bool(use_ep)]
    if use_ep:
        ep = ops.ConvF32Epilogue(*[None if t is None else t.data_ptr() for t in (o_dev.bias, o_dev.scale, o_dev.shift, o_dev.res)])
        mid = (byref(ep),)
    else:
        mid = (o_dev.bias,)
    tail = () if route == "mfma" else (ws[2], SZ(ws[0]))
    return _rc(L, name, byref(d), x, w, *mid, y, *tail)


@pytest.mark.parametrize("route,rid,kind", CONV_CASES, ids=["%s-%s-%s" % c for c in CONV_CASES])
def test_conv(device, route, rid, kind):
    L, ops = _lib()
    r, o, o64, conv, mag, m_sum = _case(route, rid, kind)
    x = Box(o.x.shape, device, o.x, off=int(r.mis == "x"))
    w = Box(o.w.shape, device, o.w, off=int(r.mis == "w"))
    res = Box(o.res.shape, device, o.res, off=int(r.mis == "r"))
    dev = NS(scale=torch.from_numpy(o.scale).to(device), shift=torch.from_numpy(o.shift).to(device),
             bias=torch.from_numpy(o.bias).to(device))
    d0 = _desc(L, r)
    ws = _workspace(L, d0, device) if route == "split" else None
    if ws:
        tc = 64 if r.cout <= 64 else 128
        assert ws[0] == 2 * 2 * r.kh * r.kw * _cdiv(r.cout, tc) * _cdiv(r.cin, 32) * 4 * tc * 8, "workspace closed form"
    for use_ep, sets in ((False, PLAIN_SETS), (True, EP_SETS)):
        worst = 0.0
        for flags in sets:
            ref, M, s = _epilogue(conv, mag, flags, o64)
            bound = _g(m_sum + s) * M
            accum = bool(flags & (ACCUM_F16 | ACCUM_IN))
            y = Box(o.y0.shape, device, o.y0 if accum else None, off=int(r.mis == "y"))
            od = NS(bias=dev.bias if flags & BIAS else None, scale=dev.scale if flags & AFFINE else None,
                    shift=dev.shift if flags & AFFINE else None, res=res.t if flags & RESIDUAL else None)
            assert _launch(L, ops, route, _desc(L, r, flags), x.t, w.t, y.t, od, ws, use_ep) == OK, flags
            got = y.get().reshape(r.P, r.cout)
            assert not np.isnan(got).any(), "elements the kernel did not write (flags %d)" % flags
            assert ws is None or bands_untouched(ws[1]), "written outside the workspace"
            if kind == "exact":
                _bits_equal(got, ref.astype(f32), "%s flags %d" % (rid, flags))
            else:
                worst = max(worst, _ratio(np.abs(got.astype(f64) - ref), bound))
                if kind == "random" and r.P * r.cout >= 64:
                    for order in _swaps(flags):
                        alt = _epilogue(conv, mag, flags, o64, order)[0]
                        assert (np.abs(alt - ref) > 100 * bound).any(), "flags %d: a swap of two steps would not show" % flags
        _note(CONV_ENTRY[route, use_ep][4:], "%s/%s" % (rid, kind), worst)
    assert x.intact() and w.intact() and res.intact()


# ------------------------------------------------------------------------------------------------ NaN rows of the convs
def _nan32(n=1):
    return np.full(n, NAN32, np.uint32).view(f32)


@pytest.mark.parametrize("where", ["x", "w", "bias", "scale", "shift", "res", "y0"])
@pytest.mark.parametrize("route", ["mfma", "split"])
def test_conv_nan(device, route, where):
    """One payload NaN in one operand: exactly the outputs the float64 expression makes NaN are NaN, the others keep
    their bound.  A NaN weight reaches every pixel of its cout, padded taps included (0 * NaN), on the device as in the
    expression."""
    L, ops = _lib()
    r = _row("nan", 1, 6, 7, 8, 12, 3, 3)
    flags = AFFINE | BIAS | RESIDUAL | RELU | ACCUM_F16
    o = _operands(route, r, "random")
    at = {"x": (0, 2, 3, 5), "w": (1, 2, 3, 7), "bias": (4,), "scale": (9,), "shift": (0,), "res": (0, 5, 6, 11), "y0": (0, 0, 0, 0)}[where]
    clean = NS(**{k: v.astype(f64) for k, v in vars(o).items()})
    getattr(o, where)[at] = _nan32()[0]
    o64 = NS(**{k: v.astype(f64) for k, v in vars(o).items()})
    for q in (o64, clean):
        q.res, q.y0 = q.res.reshape(r.P, r.cout), q.y0.reshape(r.P, r.cout)
    if route == "mfma":
        conv, mag, m_sum = _cols(clean.x, r) @ clean.w.reshape(r.K, -1), np.abs(_cols(clean.x, r)) @ np.abs(clean.w.reshape(r.K, -1)), r.K
    else:
        (conv, mag), m_sum = split_sum(clean.x.astype(f32), clean.w.astype(f32), r), 3 * r.K + 1
    hit = np.isnan(_cols(o64.x, r)).any(1)[:, None] | np.isnan(o64.w.reshape(r.K, -1)).any(0)[None, :]
    ref, M, s = _epilogue(np.where(hit, np.nan, conv), mag, flags, o64)
    want = np.isnan(ref)
    assert want.any() and not want.all()
    dev = {k: torch.from_numpy(getattr(o, k)).to(device) for k in ("x", "w", "bias", "scale", "shift", "res")}
    y = Box(o.y0.shape, device, o.y0)
    d = _desc(L, r, flags)
    ws = _workspace(L, d, device) if route == "split" else None
    od = NS(bias=dev["bias"], scale=dev["scale"], shift=dev["shift"], res=dev["res"])
    assert _launch(L, ops, route, d, dev["x"], dev["w"], y.t, od, ws, True) == OK
    got = y.get().reshape(r.P, r.cout)
    assert np.array_equal(np.isnan(got), want), "NaN outputs: %d, expected %d" % (np.isnan(got).sum(), want.sum())
    with np.errstate(invalid="ignore"):
        _note(CONV_ENTRY[route, True][4:], "nan_in_" + where, _ratio(np.abs(got.astype(f64) - ref), _g(m_sum + s) * M, skip=want))


# ------------------------------------------------------------------------------------------------ element-wise references
def _fma32(a, b, c):
    """f32(a * b + c), rounded ONCE: the float64 product of two f32 is exact, TwoSum gives the error of the float64 sum,
    and where that sum sits exactly half way between two f32 the error decides the direction"""
    a, b, c = np.broadcast_arrays(*[np.asarray(v, f32).astype(f64) for v in (a, b, c)])
    with np.errstate(invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(f32)
        d = s - r.astype(f64)
        nb = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(f32))
        tie = (d != 0) & (np.abs(d) * 2 == np.abs(nb.astype(f64) - r.astype(f64)))
        return np.where(tie & (err != 0) & (np.sign(err) == np.sign(d)), nb, r)


def _affine2(y, scale, shift):
    """y * scale + shift in f32, both ways -> {"fused": ..., "unfused": ...}"""
    y, scale, shift = (np.asarray(v, f32) for v in (y, scale, shift))
    return {"fused": _fma32(y, scale, shift), "unfused": y * scale + shift}


def _relu32(v):
    return np.where(v < 0, f32(0), v)


def _pool2(a):
    """2x2/2 SAME maximum of [n][h][w][c]; a NaN in the window gives NaN"""
    n, h, w, c = a.shape
    p = np.full((n, 2 * _cdiv(h, 2), 2 * _cdiv(w, 2), c), -np.inf, f32)
    p[:, :h, :w] = a
    q = p.reshape(n, _cdiv(h, 2), 2, _cdiv(w, 2), 2, c)
    return q.max(axis=(2, 4))                            # np.max propagates NaN


def _which(got, refs, what):
    """the name of the ONE reference `got` equals in every element ("either" where the references coincide)"""
    hits = [k for k, v in refs.items() if np.array_equal(matrix_support._z(got), matrix_support._z(v))]
    assert hits, "%s: equals neither the fused nor the unfused evaluation in every element" % what
    mode = "either" if len(hits) == 2 else hits[0]
    print("infer affine-expression %s: %s" % (what, mode))
    return mode


def _maxpool_ref(x, k, stride, pt, pl, oh, ow):
    n, h, w, c = x.shape
    out = np.full((n, oh, ow, c), -np.inf, f32)
    seen_nan = np.zeros((n, oh, ow, c), bool)
    oy, ox = np.arange(oh) * stride - pt, np.arange(ow) * stride - pl
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy + ky, ox + kx
            inside = ((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < w))[None, :]
            g = np.where(inside[None, :, :, None], x[:, np.clip(iy, 0, h - 1)][:, :, np.clip(ix, 0, w - 1)], f32(-np.inf))
            seen_nan |= np.isnan(g)
            with np.errstate(invalid="ignore"):
                out = np.where(g > out, g, out)          # the first maximum stays
    return np.where(seen_nan, f32(np.nan), out)


def _unpool_ref(x):
    """tf.image.resize_bilinear x2 with the legacy sampling, stepwise f32 as the kernel writes it"""
    n, lh, lw, c = x.shape
    oy, ox = np.arange(2 * lh), np.arange(2 * lw)
    y0, x0 = oy >> 1, ox >> 1
    y1, x1 = np.where(oy & 1, np.minimum(y0 + 1, lh - 1), y0), np.where(ox & 1, np.minimum(x0 + 1, lw - 1), x0)
    wy, wx = np.where(oy & 1, f32(0.5), f32(0))[None, :, None, None], np.where(ox & 1, f32(0.5), f32(0))[None, None, :, None]
    v00, v01, v10, v11 = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top, bot = v00 + (v01 - v00) * wx, v10 + (v11 - v10) * wx
    return (top + (bot - top) * wy).astype(f32)


def _d(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(device)


# ------------------------------------------------------------------------------------------------ element-wise rows
@pytest.mark.parametrize("npix", [1, 255, 256, 257])
def test_prep_images(device, npix):
    L, _ = _lib()
    rng = _rng("infer", "prep", npix)
    im = rng.uniform(0, 255, (npix, 3)).astype(f32)
    mean = np.array([123.68, 116.78, 103.94], f32)
    out = Guard((npix, 3), torch.float32, device)
    assert _rc(L, "ocr_prep_images_f32", _d(im, device), I64(npix), FL(mean[0]), FL(mean[1]), FL(mean[2]), out) == OK
    _bits_equal(out.np(), im - mean[None, :], "prep_images npix %d" % npix)


@pytest.mark.parametrize("c", [1, 3, 64, 257])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (8, 8)], ids=["1x1", "5x7", "8x8"])
def test_bn_relu(device, hw, c):
    """Odd edges give windows of one (corner) and two (edge) elements at 5x7 and 1x1."""
    L, _ = _lib()
    n, (h, w) = 2, hw
    rng = _rng("infer", "bn_relu", hw, c)
    y, scale, shift = (rng.standard_normal(s).astype(f32) for s in ((n, h, w, c), (c,), (c,)))
    yd, sd, hd = _d(y, device), _d(scale, device), _d(shift, device)
    modes = set()
    for relu in (0, 1):
        refs = {k: (_relu32(v) if relu else v) for k, v in _affine2(y, scale, shift).items()}
        full = Guard((n, h, w, c), torch.float32, device)
        assert _rc(L, "ocr_bn_relu_f32", yd, sd, hd, n, h, w, c, relu, 0, full, None) == OK
        modes.add(_which(full.np(), refs, "bn_relu %dx%d c%d relu%d pool0" % (h, w, c, relu)))
        for with_full in (True, False):
            full = Guard((n, h, w, c), torch.float32, device)
            pool = Guard((n, _cdiv(h, 2), _cdiv(w, 2), c), torch.float32, device)
            assert _rc(L, "ocr_bn_relu_f32", yd, sd, hd, n, h, w, c, relu, 2, full if with_full else None, pool) == OK
            what = "bn_relu %dx%d c%d relu%d pool2 a_full %d" % (h, w, c, relu, with_full)
            modes.add(_which(pool.np(), {k: _pool2(v) for k, v in refs.items()}, what))
            if with_full:
                modes.add(_which(full.np(), refs, what + " (a_full)"))
            else:
                assert full.untouched()
    assert len(modes - {"either"}) <= 1, "launches of one kernel disagree on the contraction: %s" % modes


@pytest.mark.parametrize("npix,c", [(1, 1), (255, 1), (85, 3), (1025, 1), (17, 64), (7, 3)])
def test_bn_add_relu(device, npix, c):
    L, _ = _lib()
    rng = _rng("infer", "bn_add_relu", npix, c)
    y, sc, scale, shift = (rng.standard_normal(s).astype(f32) for s in ((npix, c), (npix, c), (c,), (c,)))
    out = Guard((npix, c), torch.float32, device)
    assert _rc(L, "ocr_bn_add_relu_f32", _d(y, device), _d(scale, device), _d(shift, device), _d(sc, device), I64(npix), c, out) == OK
    _which(out.np(), {k: _relu32(v + sc) for k, v in _affine2(y, scale, shift).items()}, "bn_add_relu npix %d c %d" % (npix, c))


def test_bn_add_relu_nan(device):
    """A NaN in y, in the shortcut, in scale or in shift comes out as NaN (the ReLU is `v < 0 -> 0`, as in the epilogue),
    and nowhere else."""
    L, _ = _lib()
    rng = _rng("infer", "bn_add_relu_nan")
    npix, c = 9, 5
    y, sc, scale, shift = (rng.standard_normal(s).astype(f32) for s in ((npix, c), (npix, c), (c,), (c,)))
    y[2, 1], sc[4, 0], scale[3], shift[4] = _nan32(4)
    out = Guard((npix, c), torch.float32, device)
    assert _rc(L, "ocr_bn_add_relu_f32", _d(y, device), _d(scale, device), _d(shift, device), _d(sc, device), I64(npix), c, out) == OK
    got = out.raw()
    want = np.zeros((npix, c), bool)
    want[2, 1] = want[4, 0] = True
    want[:, 3] = want[:, 4] = True
    assert np.array_equal(np.isnan(got), want)
    refs = {k: _relu32(v + sc) for k, v in _affine2(y, scale, shift).items()}
    assert any(np.array_equal(matrix_support._z(got)[~want], matrix_support._z(v)[~want]) for v in refs.values())


POOLS = [(2, 2, "2x2/2"), (3, 2, "3x3/2"), (3, 1, "3x3/1"), (1, 2, "1x1/2")]


@pytest.mark.parametrize("c", [1, 24])
@pytest.mark.parametrize("hw", [(7, 5), (8, 6)], ids=["7x5", "8x6"])
@pytest.mark.parametrize("k,stride,pid", POOLS, ids=[p[2] for p in POOLS])
def test_maxpool(device, k, stride, pid, hw, c):
    L, _ = _lib()
    n, (h, w) = 2, hw
    rng = _rng("infer", "maxpool", pid, hw, c)
    x = np.round(rng.standard_normal((n, h, w, c)) * 4).astype(f32) / f32(4)       # a coarse grid: ties in most windows
    x[rng.random(x.shape) < 0.1] = -np.inf
    x[0, :3, :3, 0] = -np.inf                             # a whole window of -inf
    x[1, 0, 0, 0], x[1, 0, 1, 0], x[1, 1, 0, 0], x[1, 1, 1, 0] = -0.0, 0.0, -np.inf, -0.0     # first maximum: -0
    x[1, 2, 2, 0], x[1, 2, 3, 0], x[1, 3, 2, 0], x[1, 3, 3, 0] = 0.0, -0.0, -0.0, -np.inf     # first maximum: +0
    (oh, pt), (ow, pl) = _same(h, k, stride, 1), _same(w, k, stride, 1)
    y = Guard((n, oh, ow, c), torch.float32, device)
    assert _rc(L, "ocr_maxpool_f32", _d(x, device), n, h, w, c, k, stride, pt, pl, oh, ow, y) == OK
    got, ref = y.np(finite=False), _maxpool_ref(x, k, stride, pt, pl, oh, ow)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), "maxpool %s: values or the sign of a tied zero" % pid
    assert np.isneginf(got).any()


@pytest.mark.parametrize("pos", [0, 1, 2, 3])
def test_pool_nan(device, pos):
    """One NaN in a 2x2 window, in each of its four positions: the pooled value is NaN, in ocr_maxpool_f32 and in the
    pooled branch of ocr_bn_relu_f32 (with and without the ReLU), and the other windows are exact.  An all-NaN window too."""
    L, _ = _lib()
    rng = _rng("infer", "pool_nan", pos)
    n, h, w, c = 1, 6, 6, 3
    x = rng.standard_normal((n, h, w, c)).astype(f32)
    x[0, 2 + pos // 2, 2 + pos % 2, 1] = _nan32()[0]
    x[0, 4:6, 0:2, 2] = _nan32()[0]
    want = np.zeros((n, 3, 3, c), bool)
    want[0, 1, 1, 1] = want[0, 2, 0, 2] = True
    y = Guard((n, 3, 3, c), torch.float32, device)
    assert _rc(L, "ocr_maxpool_f32", _d(x, device), n, h, w, c, 2, 2, 0, 0, 3, 3, y) == OK
    got, ref = y.raw(), _maxpool_ref(x, 2, 2, 0, 0, 3, 3)
    assert np.array_equal(np.isnan(got), want) and np.array_equal(np.isnan(ref), want)
    _bits_equal(got, ref, "maxpool", skip=want)
    scale, shift = rng.uniform(0.5, 2, c).astype(f32), rng.standard_normal(c).astype(f32)
    for relu in (0, 1):
        full, pool = Guard((n, h, w, c), torch.float32, device), Guard((n, 3, 3, c), torch.float32, device)
        assert _rc(L, "ocr_bn_relu_f32", _d(x, device), _d(scale, device), _d(shift, device), n, h, w, c, relu, 2, full, pool) == OK
        got = pool.raw()
        assert np.array_equal(np.isnan(got), want), "bn_relu pool 2, relu %d" % relu
        assert np.array_equal(np.isnan(full.raw()), np.isnan(x))
        refs = {k: _pool2(_relu32(v) if relu else v) for k, v in _affine2(x, scale, shift).items()}
        assert any(np.array_equal(matrix_support._z(got)[~want], matrix_support._z(v)[~want]) for v in refs.values())


SUBS = [("c64", 64, 0, 0), ("c64_x_off", 64, 1, 0), ("c64_y_off", 64, 0, 1), ("c18", 18, 0, 0)]


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("sid,c,xoff,yoff", SUBS, ids=[s[0] for s in SUBS])
def test_subsample(device, sid, c, xoff, yoff, stride):
    L, _ = _lib()
    n, h, w = 2, 7, 5
    x = _rng("infer", "subsample", sid, stride).standard_normal((n, h, w, c)).astype(f32)
    xb = Box(x.shape, device, x, off=xoff)
    y = Box((n, _cdiv(h, stride), _cdiv(w, stride), c), device, off=yoff)
    assert _rc(L, "ocr_subsample_f32", xb.t, n, h, w, c, stride, y.t) == OK
    got = y.get()
    assert np.array_equal(got.view(np.int32), x[:, ::stride, ::stride].view(np.int32)) and xb.intact()


@pytest.mark.parametrize("c", [1, 5])
@pytest.mark.parametrize("lhw", [(1, 1), (3, 5), (4, 4)], ids=["1x1", "3x5", "4x4"])
def test_unpool(device, lhw, c):
    L, _ = _lib()
    n, (lh, lw) = 2, lhw
    rng = _rng("infer", "unpool", lhw, c)
    x = (rng.standard_normal((n, lh, lw, c)) * 2.0 ** rng.integers(-90, 91, (n, lh, lw, c))).astype(f32)
    assert (np.abs(x) < 2.0 ** 100).all() and (np.abs(x[x != 0]) > 2.0 ** -110).all()
    y = Guard((n, 2 * lh, 2 * lw, c), torch.float32, device)
    assert _rc(L, "ocr_unpool_f32", _d(x, device), n, lh, lw, c, y) == OK
    _bits_equal(y.np(), _unpool_ref(x), "unpool %dx%d c %d" % (lh, lw, c))


STATS_ROWS = [(1, 1), (63, 3), (64, 256), (65, 300), (130, 300), (130, 1), (65537, 3)]


@pytest.mark.parametrize("npix,c", STATS_ROWS)
def test_channel_stats(device, npix, c):
    L, _ = _lib()
    T = _raw(L, "ocr_channel_stats_f32_num_partials", I64(npix), ctypes.c_int(c))
    assert T == min(1024, _cdiv(npix, 64))
    strip = _cdiv(npix, T)
    x = (_rng("infer", "stats", npix, c).standard_normal((npix, c)) * 3 + 0.5).astype(f32)
    part = Guard((T, 2, c), torch.float32, device)
    assert _rc(L, "ocr_channel_stats_f32", _d(x, device), I64(npix), c, part) == OK
    got = part.np().astype(f64)
    x64 = np.zeros((T * strip, c), f64)
    x64[:npix] = x
    x64 = x64.reshape(T, strip, c)
    ref = np.stack([x64.sum(1), (x64 * x64).sum(1)], 1)
    S = np.stack([np.abs(x64).sum(1), (x64 * x64).sum(1)], 1)
    if npix == 65537:
        assert (T, strip) == (1024, 65) and not got[1009:].any() and got[1008].all(), "the empty strips hold zeros"
    _note("channel_stats_f32", "npix%d_c%d" % (npix, c), _ratio(np.abs(got - ref), 2.0 ** -24 * np.abs(ref) + strip * 2.0 ** -53 * S))


# ------------------------------------------------------------------------------------------------ the capped grid
CAP = 65536 * 256


def _pattern(count, key, device=None):
    """k / 8, k = ((29 i + key) & 4095) - 2048: on the device from torch integers, on the host from NumPy's"""
    assert count * 29 + key < 2 ** 31
    if device is not None:
        i = torch.arange(count, dtype=torch.int32, device=device)
        return ((((i * 29 + key) & 4095) - 2048).to(torch.float32) / 8).contiguous()
    i = np.arange(count, dtype=np.int32)
    return (((i * 29 + key) & 4095) - 2048).astype(f32) / f32(8)


def _same_bits(out, ref):
    got = out.raw()
    assert got.shape == ref.shape and np.array_equal((got + f32(0)).view(np.int32), (ref + f32(0)).view(np.int32))


@pytest.mark.parametrize("kernel", ["prep", "bn_relu", "bn_relu_pool", "bn_add_relu", "maxpool", "subsample", "unpool"])
def test_stream_cap(device, kernel):
    """More than 65536 * 256 work items: the grid of vgrid is capped and every thread takes a second element.  Operands
    are k / 8 with scales in {0.5, 1, 2}, so every result is exact and the comparison is bit for bit."""
    L, _ = _lib()
    if kernel == "prep":
        npix = CAP + 257
        out = Guard((npix, 3), torch.float32, device)
        assert _rc(L, "ocr_prep_images_f32", _pattern(3 * npix, 5, device), I64(npix), FL(123.5), FL(116.75), FL(103.875), out) == OK
        _same_bits(out, _pattern(3 * npix, 5).reshape(npix, 3) - np.array([123.5, 116.75, 103.875], f32))
    elif kernel in ("bn_relu", "bn_add_relu"):
        n, h, w, c = 1, 2049, 2731, 3
        assert h * w * c > CAP
        scale, shift = np.array([0.5, 1.0, 2.0], f32), np.array([-3.125, 0.25, 100.0], f32)
        y = _pattern(h * w * c, 11).reshape(n, h, w, c)
        out = Guard((n, h, w, c), torch.float32, device)
        if kernel == "bn_relu":
            assert _rc(L, "ocr_bn_relu_f32", _pattern(h * w * c, 11, device), _d(scale, device), _d(shift, device), n, h, w, c, 1, 0, out, None) == OK
            _same_bits(out, _relu32(y * scale + shift))
        else:
            assert _rc(L, "ocr_bn_add_relu_f32", _pattern(h * w * c, 11, device), _d(scale, device), _d(shift, device),
                       _pattern(h * w * c, 77, device), I64(h * w), c, out) == OK
            _same_bits(out, _relu32(y * scale + shift + _pattern(h * w * c, 77).reshape(n, h, w, c)))
    elif kernel == "bn_relu_pool":
        n, h, w, c = 1, 4097, 4097, 4
        assert 2049 * 2049 * c > CAP
        scale, shift = np.array([0.5, 1.0, 2.0, 1.0], f32), np.array([-3.125, 0.25, 100.0, -1000.0], f32)
        pool = Guard((n, 2049, 2049, c), torch.float32, device)
        assert _rc(L, "ocr_bn_relu_f32", _pattern(h * w * c, 3, device), _d(scale, device), _d(shift, device), n, h, w, c, 1, 2, None, pool) == OK
        _same_bits(pool, _pool2(_relu32(_pattern(h * w * c, 3).reshape(n, h, w, c) * scale + shift)))
    elif kernel == "maxpool":
        n, h, w, c = 1, 2049, 2049, 4
        assert h * w * c > CAP
        y = Guard((n, h, w, c), torch.float32, device)
        assert _rc(L, "ocr_maxpool_f32", _pattern(h * w * c, 9, device), n, h, w, c, 3, 1, 1, 1, h, w, y) == OK
        pad = np.full((n, h + 2, w + 2, c), -np.inf, f32)
        pad[:, 1:-1, 1:-1] = _pattern(h * w * c, 9).reshape(n, h, w, c)
        ref = pad[:, 1:-1, 1:-1].copy()
        for ky in range(3):
            for kx in range(3):
                np.maximum(ref, pad[:, ky:ky + h, kx:kx + w], out=ref)       # no NaN, and a zero's sign is not compared
        _same_bits(y, ref)
    elif kernel == "subsample":
        n, h, w, c = 1, 8194, 8194, 1                     # the scalar kernel: one item per element
        assert 4097 * 4097 > CAP
        y = Guard((n, 4097, 4097, c), torch.float32, device)
        assert _rc(L, "ocr_subsample_f32", _pattern(h * w, 21, device), n, h, w, c, 2, y) == OK
        _same_bits(y, _pattern(h * w, 21).reshape(n, h, w, c)[:, ::2, ::2])
    else:
        n, lh, lw, c = 1, 2049, 2049, 1
        assert 4 * lh * lw > CAP
        y = Guard((n, 2 * lh, 2 * lw, c), torch.float32, device)
        assert _rc(L, "ocr_unpool_f32", _pattern(lh * lw, 13, device), n, lh, lw, c, y) == OK
        _same_bits(y, _unpool_ref(_pattern(lh * lw, 13).reshape(n, lh, lw, c)))


# ------------------------------------------------------------------------------------------------ one expression
def test_affine_expression(device):
    """f32_conv_ep.h: OCR_CONV_AFFINE is "the expression of bn_relu_f32_kernel".  A 1x1 convolution of one channel with
    weight 1 on operands of the half grid leaves x itself in the accumulator on both routes (K = 1; hi = x, lo' = 0), so
    its AFFINE epilogue and ocr_bn_relu_f32 evaluate y * scale + shift on the same numbers: fused or not, they must agree."""
    L, ops = _lib()
    rng = _rng("infer", "affine_expression")
    n, h, w = 1, 9, 15
    x = rng.standard_normal((n, h, w, 1)).astype(np.float16).astype(f32)
    scale, shift = rng.uniform(0.5, 2, 1).astype(f32), rng.standard_normal(1).astype(f32)
    refs = _affine2(x, scale, shift)
    assert not np.array_equal(refs["fused"], refs["unfused"]), "operands on which the two evaluations differ"
    xd, sd, hd = _d(x, device), _d(scale, device), _d(shift, device)
    out = Guard(x.shape, torch.float32, device)
    assert _rc(L, "ocr_bn_relu_f32", xd, sd, hd, n, h, w, 1, 0, 0, out, None) == OK
    modes = {"bn_relu": _which(out.np(), refs, "plain ocr_bn_relu_f32")}
    r = _row("affine", n, h, w, 1, 1, 1, 1)
    d = _desc(L, r, AFFINE)
    one = _d(np.ones((1, 1, 1, 1), f32), device)
    for route in ("mfma", "split"):
        y = Box(x.shape, device)
        ws = _workspace(L, d, device) if route == "split" else None
        assert _launch(L, ops, route, d, xd, one, y.t, NS(bias=None, scale=sd, shift=hd, res=None), ws, True) == OK
        modes[route] = _which(y.get(), refs, "AFFINE epilogue, %s route" % route)
    assert len(set(modes.values())) == 1, modes


# ------------------------------------------------------------------------------------------------ status rows
@pytest.mark.parametrize("route", ["mfma", "split"])
def test_conv_status(device, route):
    """Every refusal of the four conv entries; the guarded output and the workspace are untouched after each."""
    L, ops = _lib()
    r = _row("status", 1, 6, 6, 8, 8, 3, 3)
    o = _operands(route, r, "random")
    t = {k: _d(getattr(o, k), device) for k in ("x", "w", "bias", "scale", "shift", "res")}
    y = Box(o.y0.shape, device)
    good = _desc(L, r)

    def wsz(d):
        return int(L._fn("ocr_conv2d_f32_split_workspace", SZ)(None if d is None else byref(d)))
    nbytes, wguard, wt = _workspace(L, good, device)
    wfull = (nbytes, wguard, wt)
    checked = [0]

    def call(want, use_ep, d, x="x", w="w", yy=True, od=None, ws=wfull, dnull=False):
        od = od or NS(bias=None, scale=None, shift=None, res=None)
        name = CONV_ENTRY[route, bool(use_ep)]
        if use_ep == "null_ep":
            mid = (None,)
        elif use_ep:
            mid = (byref(ops.ConvF32Epilogue(*[None if v is None else v.data_ptr() for v in (od.bias, od.scale, od.shift, od.res)])),)
        else:
            mid = (od.bias,)
        tail = () if route == "mfma" else (ws[2], SZ(ws[0]))
        rc = _rc(L, name, None if dnull else byref(d), t[x] if x else None, t[w] if w else None, *mid, y.t if yy else None, *tail)
        assert rc == want, (name, rc, want)
        assert y.untouched() and bands_untouched(wguard) and untouched(wt), name
        checked[0] += 1

    def variant(**kw):
        d = _desc(L, r)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for use_ep in (False, True):
        call(INVALID_ARG, use_ep, good, dnull=True)
        call(INVALID_ARG, use_ep, good, x=None)
        call(INVALID_ARG, use_ep, good, w=None)
        call(INVALID_ARG, use_ep, good, yy=False)
        for field in ("n", "h", "w", "cin", "cout", "oh", "ow", "kh", "kw", "stride", "dilation"):
            for bad in (0, -1):
                call(INVALID_ARG, use_ep, variant(**{field: bad}))
                assert wsz(variant(**{field: bad})) == 0
        call(INVALID_ARG, use_ep, variant(flags=BIAS))                       # BIAS without a bias
        call(INVALID_ARG, use_ep, variant(flip_taps=1))
        call(INVALID_ARG, use_ep, variant(flip_taps=-1))
        for stray in (STATS, 128, 1 << 20, RELU | STATS, -(1 << 31)):
            call(INVALID_ARG, use_ep, variant(flags=stray), od=NS(bias=t["bias"], scale=t["scale"], shift=t["shift"], res=t["res"]))
    for ep_only in (AFFINE, RESIDUAL, ACCUM_IN):                              # the plain entries document three flags
        call(INVALID_ARG, False, variant(flags=ep_only))
    call(INVALID_ARG, "null_ep", variant(flags=BIAS))
    call(INVALID_ARG, True, variant(flags=AFFINE), od=NS(bias=None, scale=t["scale"], shift=None, res=None))
    call(INVALID_ARG, True, variant(flags=AFFINE), od=NS(bias=None, scale=None, shift=t["shift"], res=None))
    call(INVALID_ARG, True, variant(flags=RESIDUAL))
    call(INVALID_ARG, True, variant(flags=ACCUM_IN | ACCUM_F16))
    call(UNSUPPORTED, False, variant(n=1 << 16, oh=1 << 8, ow=1 << 8))         # n oh ow = 2^32: refused before any launch
    assert wsz(None) == 0 and wsz(good) == nbytes > 0
    if route == "split":
        for use_ep in (False, True):
            call(INVALID_ARG, use_ep, good, ws=(nbytes, wguard, None))
            call(WORKSPACE, use_ep, good, ws=(nbytes - 1, wguard, wt))
            call(WORKSPACE, use_ep, good, ws=(0, wguard, wt))
            call(INVALID_ARG, use_ep, good, ws=(nbytes, wguard, wt[2:]))        # 4 bytes off 16-byte alignment
    # and the good call still works on the same buffers
    assert _launch(L, ops, route, good, t["x"], t["w"], y.t, NS(bias=None, scale=None, shift=None, res=None), wfull, True) == OK
    assert not np.isnan(y.get()).any() and bands_untouched(wguard)
    assert checked[0] > 60


def test_elementwise_status(device):
    """NULL pointers, zero and negative extents, pool = 1 and a missing output: OCR_ERR_INVALID_ARG, nothing written."""
    L, _ = _lib()
    x = _d(np.ones(4096, f32), device)
    out, out2 = Guard((4096,), torch.float32, device), Guard((4096,), torch.float32, device)
    i32 = ctypes.c_int
    rows = []

    def sweep(name, args, pointers, extents):
        """`args` is a good argument list; every pointer in turn becomes NULL, every extent 0 and -1"""
        for j in pointers:
            rows.append((name, [None if i == j else a for i, a in enumerate(args)]))
        for j in extents:
            for bad in (0, -1):
                rows.append((name, [(I64(bad) if isinstance(a, I64) else bad) if i == j else a for i, a in enumerate(args)]))

    sweep("ocr_channel_stats_f32", [x, I64(8), 2, out], (0, 3), (1, 2))
    sweep("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, 0, out, out2], (0, 1, 2), (3, 4, 5, 6))
    rows.append(("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, 1, out, out2]))          # pool = 1
    rows.append(("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, 3, out, out2]))
    rows.append(("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, -2, out, out2]))
    rows.append(("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, 0, None, out2]))         # pool 0 writes a_full
    rows.append(("ocr_bn_relu_f32", [x, x, x, 1, 4, 4, 2, 1, 2, out, None]))          # pool 2 writes a_pool
    sweep("ocr_maxpool_f32", [x, 1, 4, 4, 2, 2, 2, 0, 0, 2, 2, out], (0, 11), (1, 4, 5, 6, 9, 10))
    sweep("ocr_subsample_f32", [x, 1, 4, 4, 2, 2, out], (0, 6), (1, 2, 3, 4, 5))
    sweep("ocr_prep_images_f32", [x, I64(8), FL(1.0), FL(2.0), FL(3.0), out], (0, 5), (1,))
    sweep("ocr_bn_add_relu_f32", [x, x, x, x, I64(8), 2, out], (0, 1, 2, 3, 6), (4, 5))
    sweep("ocr_unpool_f32", [x, 1, 2, 2, 2, out], (0, 5), (1, 2, 3, 4))
    for name, args in rows:
        assert _rc(L, name, *args) == INVALID_ARG, (name, args)
        assert out.untouched() and out2.untouched(), name
    for npix, c in ((0, 4), (-1, 4), (8, 0), (8, -1)):
        assert _raw(L, "ocr_channel_stats_f32_num_partials", I64(npix), i32(c)) == INVALID_ARG
    assert len(rows) > 70


def test_maxpool_status_empty_input(device):
    """h = 0 or w = 0 (and negative): there is no input to take a maximum of; the entry once returned 0 and stored -inf."""
    L, _ = _lib()
    x = _d(np.ones(64, f32), device)
    out = Guard((64,), torch.float32, device)
    for h, w in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert _rc(L, "ocr_maxpool_f32", x, 1, h, w, 2, 2, 2, 0, 0, 2, 2, out) == INVALID_ARG
        assert out.untouched()
