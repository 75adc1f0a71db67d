"""GPU: the fused launch entries of csrc/conv_igemm.hip that the epilogue matrix (test_gpu_conv_epilogues.py) does not
reach — the operand-transforming pointwise kernel's forward and backward loaders, the bottleneck tail on every kernel
that carries it, and the pooled epilogue of the persistent 64-channel kernel — each against a float64 restatement on
16-bit-exact operands, called through the C ABI (a refusal is a status, not an exception).  No device route is
compared with another.  The stages are decoupled so that a failure names the stage: the loader output (x_out /
dy_out) is checked against float64 of the inputs; the convolution against the float64 convolution of THE LOADER OUTPUT
THE DEVICE STORED; the partial sums against float64 sums of THE y / dx THE DEVICE STORED.

Rows (the family asserted through ocr_conv2d_variant, the partial-row count through ocr_conv2d_num_mtiles):

  Part A, forward loaders, (n, h, w, cin, cout), 1x1 SAME — ocr_conv2d_pw_bnaddrelu_f16 (with / without the
  projection BN, with mask_bits / NULL, with / without OCR_CONV_STATS) and ocr_conv2d_pw_bnrelu_f16 on every row:
    a64     2,16,24,256,64    conv_pwx_kernel<64,1>: four K stages, exactly three flat tiles
    a128r   1,20,32,512,128   conv_pwx_kernel<128,2>: 2.5 flat tiles (ragged)
    a480    3,5,32,128,64     conv_pwx_kernel<64,1>: 480 pixels (a multiple of 32, not of 64), two K stages
    a256sw  2,16,32,128,512   conv_pwx_kernel<256,4>: grid 4 x 2 = 8, XCD swizzle on; only cout tile 0 writes x_out / bits
    a256    2,8,20,1024,256   conv_pwx_kernel<256,4>: one cout tile, no swizzle, ragged
    amax    1,8,8,2048,256    conv_pwx_kernel<256,4>: two stages + coefficient rows = exactly 160 KB of LDS, a quarter tile
  Refused (OCR_ERR_UNSUPPORTED, outputs untouched): cin = 64; cin = 2112 with cout = 256 (LDS); 1,5,5,128,128 (25
  pixels); a 3x3 descriptor.  BIAS, RELU or ACCUM_F16 in d->flags: OCR_ERR_INVALID_ARG.

  Part B, backward loader, input-gradient form (cin = c4 the operand's channels, cout = c the gradient's) —
  ocr_conv2d_pw_bnbwd_bnred_f16 (bn_relu 0 | 1) and ocr_conv2d_pw_bnbwd_tail_f16 (relu_shift NULL | given x the
  epilogues plain, accum, tail_out, tail_bits, tail_sub, tail_accum_sub_bits; the sub_grad ones on b256o only):
    b128    2,16,24  256 -> 128   conv_pwx_kernel<128,2>: three flat tiles
    b128r   1,20,32  512 -> 128   ragged
    b256o   4,7,24   512 -> 256   conv_pwx_kernel<256,4>: odd h, h*w = 168 and w = 24 no powers of two, sub_grad [4][4][12][256]
    b256sw  2,16,32  128 -> 512   swizzle on, two cout tiles
    cout = 64 (2,16,24, 256 -> 64, conv_pwx_kernel<64,1>): COUT64_SUPPORTED below.

  Part C, ocr_conv2d_bnred_tail_f16 on the plain kernels, (n, h, w, cin, cout, k), input-gradient form:
    t_pw    2,12,40,64,256,1   conv_pw_kernel<256,4> (256-cout tile kept: the epilogue loads)
    t_pw64  2,12,24,128,192,1  conv_pw_kernel<64,1>, three cout tiles
    t_ig1   2,9,37,128,512,1   conv_igemm_kernel<256,64,4,0,8>: generic 1x1, odd h and w
    t_w4    2,12,40,128,256,3  named conv3x3_w4_kernel, launched on conv_igemm_kernel
    t_w4s   2,13,40,128,128,3  named conv3x3_w4s_kernel<128>, launched on conv_igemm_kernel
    t_16row 2,24,33,96,384,3   conv_igemm_kernel<128,32,2,1,16>: 16-row tiles, two partial rows per tile
    t_c64   2,100,130,64,64,3  conv_c64_persist_kernel<64>: OCR_ERR_UNSUPPORTED, outputs untouched
  1x1 rows: {tail_out, bits} x {plain, ACCUM} x {no sub, sub}; 3x3 rows: (tail_out, plain, no sub) and (bits, ACCUM,
  sub).  BIAS / RELU in flags or both masks NULL: OCR_ERR_INVALID_ARG.

  Part D, ocr_conv2d_relu_pool_f16 (conv_c64_persist_kernel<64, true>), 64 -> 64, (2,100,130) even / even and
  (2,101,131) odd / odd (130 pixel tiles each; the kernel needs >= 128), flags BIAS|RELU | BIAS | 0, argmax given and
  NULL: POOL_SUPPORTED below.  (2,12,24) and shapes outside 64 -> 64: OCR_ERR_UNSUPPORTED; STATS / ACCUM_F16:
  OCR_ERR_INVALID_ARG.

Where the kernels round.
  conv_pwx_kernel MODE 1 (pw_bnaddrelu): z = r16(fma(prev_y, scale, shift)); r = shortcut, or r16(fma(shortcut,
    sc_scale, sc_shift)) with the projection; f = z + r in f32; x_out = r16(max(f, 0)); bit e = the stored value > 0.
  MODE 3 (pw_bnrelu): x_out = r16(max(fma(prev_y, scale, shift), 0)).
  MODE 2 (pw_bnbwd_*): dy_out = r16(fma(A, dz * [fma(y, A, relu_shift) > tie], fma(B, y, C))), the mask dropped without
    relu_shift (tie = OCR_RELU_TIE, half the smallest subnormal).
  Epilogue (conv_epilogue.h; the header of ocr_conv2d_bnred_tail_f16): r16(f32 accumulator); under ACCUM_F16
    r16(that + old); with sub_grad r16(that + sub) at the pixels with y and x even, sub index (image, y / 2, x / 2),
    extents ceil(h / 2), ceil(w / 2); zero where tail_out <= 0 (or the bit is clear); the partial sums are taken of the
    stored 16-bit values in f32.
  Pooled epilogue: r16(max(acc + bias, 0)) per pixel, then the first maximum in (dy, dx) order of the window's existing
    pixels; a 16-bit maximum is exact.

Bounds (u = U16 the storage half-ulp, e = U32 = 2^-24, tiny = the smallest subnormal; M = the sum of |terms|).
  pw_bnrelu x_out   one f32 fma (<= e |z|) and one 16-bit rounding:  u |ref| + 4 e M + tiny  (the form of
                    test_gpu_bn_pool_matrix._r16), M = |y scale| + |shift|.
  pw_bnaddrelu x_out  E1 = u (|z| + [proj] |sv|) + 4 e M + 2 tiny covers the two inner 16-bit roundings and the three
                    f32 roundings (two fmas, one add; M = |y scale| + |shift| + |short sc| + |sc_shift|).  The ReLU is
                    1-Lipschitz, the final rounding is taken of a value within E1 of ref:
                    bound = E1 + u (|ref| + E1) + tiny.  No element is skipped: at the threshold the value is inside.
  dy_out            two nested f32 fmas and one rounding: u |ref| + 4 e M + tiny, M = |A dz| + |B y| + |C|.  With
                    relu_shift the elements with |A y + shift| <= 4 e (|A y| + |shift|) are skipped (share <= 1e-3,
                    asserted by the builder from the operands alone).
  y / dx            the reference carries the kernel's 16-bit roundings, so what is left is the f32 accumulation and the
                    1-ulp flips it causes: one rounding 1e-3 (f16) / 8e-3 (bf16) of max|ref|, two roundings 1.5e-3 /
                    8e-3 (the project's bars); k >= 3 roundings the one-rounding bar + (k - 1) u max|stored total|.
                    The two pixels whose sub_grad entry is 64 x larger are barred by their own maximum, everything
                    else by the maximum without them (stricter than one maximum over all).  Masked elements: exactly 0.
  stats / partial   the epilogue matrix's: (sum, sum of squares) rtol 1e-4, atol 1e-2 / 1e-8; (sum dz, sum dz xhat) rtol
                    1e-3, atol 5e-2, an element whose mask an f32 evaluation may see differently counted on either side.
  pooled            one-rounding bar of the reference maximum; the float64 value at the argmax position within twice
                    that bound of the window's maximum; under RELU windows whose float64 values are all below -bound
                    store exactly 0 with argmax 0.

Findings (no kernel was found wrong; two statements of the header were, and are corrected there).
  * cout = 64 under ocr_conv2d_pw_bnbwd_tail_f16: the header asked for cout >= 128, conv_plan does not check it, and
    the device serves all six epilogues correctly on conv_pwx_kernel<64,1> (COUT64_SUPPORTED: all True).
  * ocr_conv2d_relu_pool_f16 with flags BIAS and 0: the header named BIAS|RELU only; the generic instantiation of the
    pooled kernel gives the correct maximum of conv [+ bias] and its first-max positions (POOL_SUPPORTED: all True).
  * Rerouted tails (t_w4, t_w4s) fill exactly ocr_conv2d_num_mtiles rows although the named and the launched family
    differ; conv_c64_persist_kernel refuses the tail and writes nothing.

MEASURED (largest |err| / bound per entry over its rows on the MI355X, f16 / bf16 library, from the `conv_fused <entry>
<row> ratio=` lines; records, not thresholds — the threshold is ratio <= 1.  A stored 16-bit output that is right to the
last bit still shows its final rounding, up to 0.999 of u |ref|.)
  pw_bnaddrelu   x_out 0.990 / 0.989   y 0.329 / 0.326   stats 0.003 / 0.004
  pw_bnrelu      x_out 0.997 / 0.996   y 0.402 / 0.396   stats 0.003 / 0.003
  pw_bnbwd_bnred dy_out 0.998 / 0.996  dx 0.357 / 0.357  partial 0.000 / 0.000
  pw_bnbwd_tail  dy_out 0.998 / 0.996  dx 0.445 / 0.446  partial 0.000 / 0.000   (cout = 64 rows included)
  bnred_tail     dx 0.324 / 0.279      partial 0.000 / 0.000
  relu_pool      pooled 0.298 / 0.299  argmax 0.111 / 0.137
  (partial: below 0.0005 of the epilogue matrix's rtol 1e-3 / atol 5e-2, which is wide for sums of a few hundred
  stored values; the bars are the project's and are kept as they are.)
"""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (F16, INVALID_ARG, OK, TINY, U16, U32, UNSUPPORTED, _d32, _dev, _h, _ratio, _rc, _rng,
                            bands_untouched, carve, f32, f64, untouched)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "conv_fused")

BIAS, RELU, STATS, ACCUM = 1, 2, 4, 8
Y_BAND = 16 * 32 * 256          # elements: the largest tile (16 rows x 32 columns x 256 couts)
P_BAND = 2 * 512 * 4            # floats: four partial rows of the widest layer
T1 = 1e-3 if F16 else 8e-3      # one output rounding
T2 = 1.5e-3 if F16 else 8e-3    # two

A_ROWS = {  # name: (variant, (n, h, w, cin, cout))
    "a64": ("conv_pw_kernel<64,1>", (2, 16, 24, 256, 64)),
    "a128r": ("conv_pw_kernel<128,2>", (1, 20, 32, 512, 128)),
    "a480": ("conv_pw_kernel<64,1>", (3, 5, 32, 128, 64)),
    "a256sw": ("conv_pw_kernel<256,4>", (2, 16, 32, 128, 512)),
    "a256": ("conv_pw_kernel<256,4>", (2, 8, 20, 1024, 256)),
    "amax": ("conv_pw_kernel<256,4>", (1, 8, 8, 2048, 256)),
}
A_MTILES = {"a64": 3, "a128r": 3, "a480": 2, "a256sw": 4, "a256": 2, "amax": 1}
# (entry, projection BN, mask_bits given, OCR_CONV_STATS)
A_VARIANTS = [("add", p, b, s) for p in (0, 1) for b in (1, 0) for s in (1, 0)] + [("relu", 0, 0, 1), ("relu", 0, 0, 0)]

B_ROWS = {  # name: (variant, (n, h, w, c4, c))
    "b128": ("conv_pw_kernel<128,2>", (2, 16, 24, 256, 128)),
    "b128r": ("conv_pw_kernel<128,2>", (1, 20, 32, 512, 128)),
    "b256o": ("conv_pw_kernel<256,4>", (4, 7, 24, 512, 256)),
    "b256sw": ("conv_pw_kernel<256,4>", (2, 16, 32, 128, 512)),
    "b64": ("conv_pw_kernel<64,1>", (2, 16, 24, 256, 64)),       # the cout = 64 row (COUT64_SUPPORTED)
}
# epilogue: (ACCUM_F16, tail mask form, sub_grad)
EPILOGUES = {"plain": (0, None, 0), "accum": (1, None, 0), "tail_out": (0, "out", 0), "tail_bits": (0, "bits", 0),
             "tail_sub": (0, "out", 1), "tail_accum_sub_bits": (1, "bits", 1)}
B_TAIL_CASES = [(r, s, e) for r in ("b128", "b128r", "b256o", "b256sw") for s in (0, 1) for e in EPILOGUES
                if not EPILOGUES[e][2] or r == "b256o"]
# cout = 64 under ocr_conv2d_pw_bnbwd_tail_f16 (the header asks for cout >= 128, conv_plan does not check it): per
# epilogue True = the correct result, False = OCR_ERR_UNSUPPORTED, as the device returned.  Anything else is a bug.
COUT64_SUPPORTED = {e: True for e in EPILOGUES}

C_ROWS = {  # name: (variant, (n, h, w, cin, cout, k))
    "t_pw": ("conv_pw_kernel<256,4>", (2, 12, 40, 64, 256, 1)),
    "t_pw64": ("conv_pw_kernel<64,1>", (2, 12, 24, 128, 192, 1)),
    "t_ig1": ("conv_igemm_kernel<256,64,4,0,8>", (2, 9, 37, 128, 512, 1)),
    "t_w4": ("conv3x3_w4_kernel", (2, 12, 40, 128, 256, 3)),
    "t_w4s": ("conv3x3_w4s_kernel<128>", (2, 13, 40, 128, 128, 3)),
    "t_16row": ("conv_igemm_kernel<128,32,2,1,16>", (2, 24, 33, 96, 384, 3)),
    "t_c64": ("conv_c64_persist_kernel<64>", (2, 100, 130, 64, 64, 3)),
}
# (mask form, ACCUM_F16, sub_grad)
C_CASES = [(r, m, a, s) for r in ("t_pw", "t_pw64", "t_ig1") for m in ("out", "bits") for a in (0, 1) for s in (0, 1)] + \
          [(r, m, a, s) for r in ("t_w4", "t_w4s", "t_16row") for (m, a, s) in (("out", 0, 0), ("bits", 1, 1))]

D_SHAPES = {"even": (2, 100, 130), "odd": (2, 101, 131)}
# flag set under ocr_conv2d_relu_pool_f16 (the header documents BIAS|RELU; the others run the generic instantiation of
# the pooled kernel): True = the correct result, False = OCR_ERR_UNSUPPORTED, as the device returned
POOL_SUPPORTED = {BIAS | RELU: True, BIAS: True, 0: True}

N_TESTS = (len(A_ROWS) * len(A_VARIANTS) + 2 * 4 + 2 * 3 + len(B_TAIL_CASES) + len(EPILOGUES) + 2 * len(B_ROWS) + 1
           + len(C_CASES) + 2 + 1 + 2 * len(POOL_SUPPORTED) * len(D_SHAPES) + 1)

_OPS = {}                       # operands (and, where the operand is not device-made, the float64 convolution), per row


# ------------------------------------------------------------------------------------------------ helpers
def _lib():
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd import ops
    return L, ops


def _desc(ops, n, h, w, cin, cout, k, form, flags):
    """SAME padding; the input-gradient form flips the taps and takes the pads layers._conv_dgrad computes"""
    d = ops.conv_desc((n, h, w, cin), cout, k, k, 1, 1)
    if form == "dgrad":
        d.pad_top = (k - 1) - d.pad_top
        d.pad_left = (k - 1) - d.pad_left
        d.flip_taps = 1
    d.flags = flags
    return d


def _np(t):
    return t.float().cpu().numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.cpu().numpy()


class Bytes:
    """a byte buffer (mask bits, argmax) inside a larger allocation: 0xEE between two 0x5E bands"""

    def __init__(self, numel, band, device):
        assert band % 16 == 0
        self.flat = torch.full((2 * band + numel,), 0x5E, dtype=torch.uint8, device=device)
        self.t = self.flat[band:band + numel]
        self.t.fill_(0xEE)
        self.band = band
        assert self.t.data_ptr() % 16 == 0

    def bands(self):
        return bool((self.flat[:self.band] == 0x5E).all()) and bool((self.flat[self.band + self.t.numel():] == 0x5E).all())

    def untouched(self):
        return self.bands() and bool((self.t == 0xEE).all())


def _packbits(mask):
    return np.packbits(np.asarray(mask).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _conv64(x, wk, d):
    """float64 convolution of x [n,h,w,cin] with wk [k*k][cout][cin] under descriptor d (stride 1, dilation 1)"""
    k = d.kh
    n, h, w, cin = x.shape
    cout = wk.shape[1]
    if k == 1:
        return (x.reshape(-1, cin).astype(f64) @ wk[0].astype(f64).T).reshape(n, h, w, cout)
    wt = torch.from_numpy(wk).double().reshape(k, k, cout, cin)
    if d.flip_taps:
        wt = wt.flip(0, 1)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    pad = (d.pad_left, k - 1 - d.pad_left, d.pad_top, k - 1 - d.pad_top)
    ref = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, pad), wt.permute(2, 3, 0, 1).contiguous())
    return ref.permute(0, 2, 3, 1).contiguous().numpy()


def _r16(got, ref, M, skip=None):
    """a stored 16-bit output of one f32 expression against float64 (test_gpu_bn_pool_matrix._r16's bound)"""
    ref = np.asarray(ref, f64)
    return _ratio(np.abs(got.astype(f64) - ref), U16 * np.abs(ref) + 4 * U32 * np.asarray(M, f64) + TINY, skip)


def _check_y(got, ref):
    """one output rounding: the project's bar of max|ref|"""
    return _ratio(np.abs(got.astype(f64) - ref), T1 * np.abs(ref).max())


def _check_stats(part, got):
    """(sum, sum of squares) of the STORED values, per column after summing the rows: the epilogue matrix's rtol / atol"""
    sums = part.astype(f64).sum(0)
    g = got.astype(f64).reshape(-1, got.shape[-1])
    want = [g.sum(0), (g * g).sum(0)]
    bars = [(1e-4, 1e-2), (1e-4, 1e-8)]
    return max(_ratio(np.abs(sums[i] - want[i]), bars[i][1] + bars[i][0] * np.abs(want[i])) for i in range(2))


def _check_partial(part, dz, by, mean, invstd, unsure=None):
    """(sum dz, sum dz xhat(bn_y)) of the STORED gradient, dz already masked: the epilogue matrix's rtol / atol; an
    undecided element counts on either side"""
    sums = part.astype(f64).sum(0)
    c = dz.shape[-1]
    dz = dz.astype(f64).reshape(-1, c)
    xh = ((by.astype(f64) - mean) * invstd).reshape(-1, c)
    want = [dz.sum(0), (dz * xh).sum(0)]
    slack = [0.0, 0.0]
    if unsure is not None:
        slack = [np.where(unsure, np.abs(dz), 0.0).sum(0), np.where(unsure, np.abs(dz * xh), 0.0).sum(0)]
    return max(_ratio(np.abs(sums[i] - want[i]), 5e-2 + 1e-3 * np.abs(want[i]) + slack[i]) for i in range(2))


def _expect_dx(conv, old, sub, tail_out):
    """the epilogue in float64 with roundings where the kernel rounds -> (reference, roundings, the total before the
    mask)"""
    r, k = _h(conv).astype(f64), 1
    if old is not None:
        r, k = _h(r + old).astype(f64), k + 1
    if sub is not None:
        r = r.copy()
        r[:, ::2, ::2] = _h(r[:, ::2, ::2] + sub)
        k += 1
    return (r if tail_out is None else np.where(tail_out > 0, r, 0.0)), k, r


def _check_dx(got, ref, k, total, tail_out, big):
    """`big`: the pixels whose sub_grad entry is 64 x larger, barred by their own maximum"""
    bar = np.zeros(ref.shape)
    for sel in (~big, big):
        if sel.any():
            m, mt = np.abs(ref[sel]).max(), np.abs(total[sel]).max()
            bar[sel] = T1 * m if k == 1 else T2 * m if k == 2 else T1 * m + (k - 1) * U16 * mt
    if tail_out is not None:
        assert (got[tail_out <= 0] == 0).all(), "non-zero values where the tail mask is false"
    return _ratio(np.abs(got.astype(f64) - ref), bar)


def _big_sub(rng, n, h, w, c):
    """sub_grad [n][ceil(h/2)][ceil(w/2)][c] with one entry 64 x larger at the last even / even pixel of the last
    image and one at pixel (0, 0) of image 1 -> (sub, the full-resolution pixels they land on)"""
    sh, sw = (h + 1) // 2, (w + 1) // 2
    sub = rng.standard_normal((n, sh, sw, c)) * 0.3
    sub[n - 1, sh - 1, sw - 1] *= 64
    sub[min(1, n - 1), 0, 0] *= 64
    big = np.zeros((n, h, w, c), bool)
    big[n - 1, 2 * (sh - 1), 2 * (sw - 1)] = True
    big[min(1, n - 1), 0, 0] = True
    return _h(sub), big


def _tail_operands(rng, n, h, w, c):
    """what the tail epilogue reads, on the output's geometry"""
    T = {"old": _h(rng.standard_normal((n, h, w, c)) * 0.5), "out": _h(rng.standard_normal((n, h, w, c))),
         "by": _h(rng.standard_normal((n, h, w, c))), "mean": rng.normal(0, 0.2, c).astype(f32),
         "invstd": rng.uniform(0.7, 1.3, c).astype(f32)}
    T["sub"], T["big"] = _big_sub(rng, n, h, w, c)
    T["bits"] = _packbits(T["out"] > 0)
    return T


def _tail_args(T, form, use_sub, device):
    """(bn_y, bn_mean, bn_invstd, tail_out, tail_mask_bits, sub_grad) of a tail call; the bits form gets no tail_out"""
    return (_dev(T["by"], device), _d32(T["mean"], device), _d32(T["invstd"], device),
            _dev(T["out"], device) if form == "out" else None,
            torch.from_numpy(T["bits"]).to(device) if form == "bits" else None,
            _dev(T["sub"], device) if use_sub else None)


# ------------------------------------------------------------------------------------------------ part A
def a_operands(row):
    if row not in _OPS:
        n, h, w, cin, cout = A_ROWS[row][1]
        rng = _rng("A", row)
        P = {"y": _h(rng.standard_normal((n, h, w, cin))), "short": _h(rng.standard_normal((n, h, w, cin))),
             "sc": rng.uniform(0.5, 1.5, cin).astype(f32), "sh": rng.normal(0, 0.3, cin).astype(f32),
             "ssc": rng.uniform(0.5, 1.5, cin).astype(f32), "ssh": rng.normal(0, 0.3, cin).astype(f32),
             "w": _h(rng.standard_normal((1, cout, cin)) * np.sqrt(2.0 / cin))}
        P["sc"][5] = -0.8                                                  # a negative scale
        P["ssc"][cin - 3] = -1.1
        _OPS[row] = P
    return _OPS[row]


def _a_launch(L, ops, device, shape, k, P, entry, proj, bits, flags, stats_given=None):
    """one forward-loader call on carved outputs -> (status, outputs)"""
    n, h, w, cin, cout = shape
    d = _desc(ops, n, h, w, cin, cout, k, "fwd", flags)
    T = ops.conv2d_num_mtiles(d)
    xg, x_out = carve((n, h, w, cin), O.STORAGE, Y_BAND, device)
    yg, y = carve((n, d.oh, d.ow, cout), O.STORAGE, Y_BAND, device)
    pg, part = carve((T, 2, cout), torch.float32, P_BAND, device)
    mb = Bytes(n * h * w * cin // 8, 256 * cin // 8, device) if bits else None
    stats = part if (flags & STATS if stats_given is None else stats_given) else None
    a = [_dev(P["y"], device), _d32(P["sc"], device), _d32(P["sh"], device)]
    if entry == "add":
        rc = _rc(L, "ocr_conv2d_pw_bnaddrelu_f16", ctypes.byref(d), *a, _dev(P["short"], device),
                 _d32(P["ssc"], device) if proj else None, _d32(P["ssh"], device) if proj else None, x_out,
                 mb.t if bits else None, _dev(P["w"], device), y, stats)
    else:
        rc = _rc(L, "ocr_conv2d_pw_bnrelu_f16", ctypes.byref(d), *a, x_out, _dev(P["w"], device), y, stats)
    torch.cuda.synchronize()
    return rc, dict(d=d, T=T, xg=xg, x_out=x_out, yg=yg, y=y, pg=pg, part=part, mb=mb)


def _a_untouched(R):
    return (untouched(R["x_out"]) and untouched(R["y"]) and untouched(R["part"]) and bands_untouched(R["xg"]) and
            bands_untouched(R["yg"]) and bands_untouched(R["pg"]) and (R["mb"] is None or R["mb"].untouched()))


@pytest.mark.parametrize("entry,proj,bits,stats", A_VARIANTS)
@pytest.mark.parametrize("row", list(A_ROWS))
def test_forward_loaders(device, row, entry, proj, bits, stats):
    L, ops = _lib()
    variant, shape = A_ROWS[row]
    n, h, w, cin, cout = shape
    P = a_operands(row)
    rc, R = _a_launch(L, ops, device, shape, 1, P, entry, proj, bits, STATS if stats else 0)
    assert ops.conv2d_variant(R["d"]) == variant and R["T"] == A_MTILES[row]
    assert rc == OK, rc
    assert bands_untouched(R["xg"]) and bands_untouched(R["yg"]) and bands_untouched(R["pg"])
    name = "pw_bnaddrelu" if entry == "add" else "pw_bnrelu"
    tag = "%s/p%db%ds%d" % (row, proj, bits, stats)
    # the loader output against float64 of the inputs
    got = _np(R["x_out"])
    assert not np.isnan(got).any(), "x_out: elements not written"
    y64, sc, sh = P["y"].astype(f64), P["sc"].astype(f64), P["sh"].astype(f64)
    z = y64 * sc + sh
    Mz = np.abs(y64 * sc) + np.abs(sh)
    if entry == "relu":
        _note(name + "_x_out", tag, _r16(got, np.maximum(z, 0.0), Mz))
    else:
        s64 = P["short"].astype(f64)
        sv = s64 * P["ssc"] + P["ssh"] if proj else s64
        M = Mz + (np.abs(s64 * P["ssc"]) + np.abs(P["ssh"].astype(f64)) if proj else np.abs(s64))
        ref = np.maximum(z + sv, 0.0)
        E1 = U16 * (np.abs(z) + (np.abs(sv) if proj else 0.0)) + 4 * U32 * M + 2 * TINY
        _note(name + "_x_out", tag, _ratio(np.abs(got - ref), E1 + U16 * (ref + E1) + TINY))
        if bits:
            assert R["mb"].bands(), "stores outside mask_bits"
            assert np.array_equal(R["mb"].t.cpu().numpy(), _packbits(got > 0)), "mask_bits is not the mask of the stored x_out"
    # the convolution of the stored loader output
    gy = _np(R["y"])
    assert not np.isnan(gy).any(), "y: elements not written"
    _note(name + "_y", tag, _check_y(gy, _conv64(got, P["w"], R["d"])))
    if stats:
        pr = _np(R["part"])
        assert not np.isnan(pr).any(), "partial rows not written"
        _note(name + "_stats", tag, _check_stats(pr, gy))
    else:
        assert untouched(R["part"])


A_REFUSED = {"cin64": ((2, 16, 24, 64, 64), 1), "lds": ((1, 8, 8, 2112, 256), 1), "pix25": ((1, 5, 5, 128, 128), 1),
             "k3": ((2, 16, 24, 128, 128), 3)}


@pytest.mark.parametrize("entry", ["add", "relu"])
@pytest.mark.parametrize("case", list(A_REFUSED))
def test_forward_loaders_refuse(device, case, entry):
    L, ops = _lib()
    shape, k = A_REFUSED[case]
    n, h, w, cin, cout = shape
    rng = _rng("A-refused", case)
    P = {"y": _h(rng.standard_normal((n, h, w, cin))), "short": _h(rng.standard_normal((n, h, w, cin))),
         "sc": np.ones(cin, f32), "sh": np.zeros(cin, f32), "ssc": np.ones(cin, f32), "ssh": np.zeros(cin, f32),
         "w": _h(rng.standard_normal((k * k, cout, cin)) * 0.05)}
    rc, R = _a_launch(L, ops, device, shape, k, P, entry, 1, 1, STATS)
    assert rc == UNSUPPORTED, rc
    assert _a_untouched(R)


@pytest.mark.parametrize("entry", ["add", "relu"])
@pytest.mark.parametrize("flag", [BIAS, RELU, ACCUM])
def test_forward_loaders_flags(device, flag, entry):
    L, ops = _lib()
    rc, R = _a_launch(L, ops, device, A_ROWS["a480"][1], 1, a_operands("a480"), entry, 0, 1, flag | STATS)
    assert rc == INVALID_ARG, rc
    assert _a_untouched(R)
    rc, R = _a_launch(L, ops, device, A_ROWS["a480"][1], 1, a_operands("a480"), entry, 0, 1, STATS, stats_given=False)
    assert rc == INVALID_ARG, rc                                           # STATS without a stats buffer
    assert _a_untouched(R)


# ------------------------------------------------------------------------------------------------ part B
def b_operands(row):
    """operands of a backward-loader row; asserts from the operands alone that the elements whose ReLU mask an f32
    evaluation may see differently are at most 1e-3 of the tensor"""
    if row not in _OPS:
        n, h, w, c4, c = B_ROWS[row][1]
        rng = _rng("B", row)
        P = {"dz": _h(rng.standard_normal((n, h, w, c4)) * 0.3), "ya": _h(rng.standard_normal((n, h, w, c4))),
             "A": rng.uniform(0.5, 1.5, c4).astype(f32), "B": rng.normal(0, 0.3, c4).astype(f32),
             "C": rng.normal(0, 0.1, c4).astype(f32), "shift": rng.normal(0, 0.3, c4).astype(f32),
             "w": _h(rng.standard_normal((1, c, c4)) * np.sqrt(2.0 / c4))}
        ay = P["ya"].astype(f64) * P["A"]
        pre = ay + P["shift"]
        P["skip"] = np.abs(pre) <= 4 * U32 * (np.abs(ay) + np.abs(P["shift"].astype(f64)))
        share = float(P["skip"].mean())
        assert share <= 1e-3, (row, share)
        P["mask"] = pre > 0
        P["tail"] = _tail_operands(rng, n, h, w, c)
        # the layer below, for ocr_conv2d_pw_bnbwd_bnred_f16 (general BN parameters, two negative scales)
        bsc = rng.uniform(0.5, 1.5, c).astype(f32)
        bsc[5], bsc[c - 3] = -0.8, -1.1
        P["bsc"], P["bsh"] = bsc, rng.normal(0, 0.3, c).astype(f32)
        a = P["tail"]["by"].astype(f64) * bsc
        zz = a + P["bsh"]
        P["bn_mask"] = zz > 0
        P["bn_unsure"] = np.abs(zz) < 2e-5 * (np.abs(a) + np.abs(P["bsh"].astype(f64)))
        assert float(P["bn_unsure"].mean()) <= 1e-4
        _OPS[row] = P
    return _OPS[row]


def _b_loader_args(P, relu_shift, device):
    return (_dev(P["dz"], device), _dev(P["ya"], device), _d32(P["A"], device), _d32(P["B"], device), _d32(P["C"], device),
            _d32(P["shift"], device) if relu_shift else None)


def _b_check_dy(P, got, relu_shift):
    assert not np.isnan(got).any(), "dy_out: elements not written"
    dz, ya = P["dz"].astype(f64), P["ya"].astype(f64)
    A, B, C = (P[k].astype(f64) for k in "ABC")
    dzm = np.where(P["mask"], dz, 0.0) if relu_shift else dz
    ref = A * dzm + B * ya + C
    M = np.abs(A * dzm) + np.abs(B * ya) + np.abs(C)
    return _r16(got, ref, M, P["skip"] if relu_shift else None)


def _b_tail_launch(L, ops, device, row, relu_shift, epi, flags=None, tail_override=None):
    shape = B_ROWS[row][1]
    n, h, w, c4, c = shape
    accum, form, use_sub = EPILOGUES[epi]
    P = b_operands(row)
    T = P["tail"]
    d = _desc(ops, n, h, w, c4, c, 1, "dgrad", (ACCUM if accum else 0) if flags is None else flags)
    rows = ops.conv2d_num_mtiles(d)
    dyg, dy = carve((n, h, w, c4), O.STORAGE, Y_BAND, device)
    dxg, dx = carve((n, h, w, c), O.STORAGE, Y_BAND, device, _dev(T["old"], device) if accum else None)
    pg, part = carve((rows, 2, c), torch.float32, P_BAND, device)
    targs = _tail_args(T, form, use_sub, device) if form else (None,) * 6
    if tail_override is not None:
        targs = tail_override(targs)
    la = _b_loader_args(P, relu_shift, device)
    rc = _rc(L, "ocr_conv2d_pw_bnbwd_tail_f16", ctypes.byref(d), *la, dy, _dev(P["w"], device), dx, part, *targs)
    torch.cuda.synchronize()
    return rc, dict(d=d, rows=rows, dyg=dyg, dy=dy, dxg=dxg, dx=dx, pg=pg, part=part, accum=accum, old=T["old"])


def _b_untouched(R, device):
    same = torch.equal(R["dx"], _dev(R["old"], device)) if R["accum"] else untouched(R["dx"])
    return (same and untouched(R["dy"]) and untouched(R["part"]) and bands_untouched(R["dyg"]) and
            bands_untouched(R["dxg"]) and bands_untouched(R["pg"]))


_B_STORED = {}                  # (row, relu_shift, epilogue) -> (dx, partial) bits, for the tail_out / bits comparison


def _b_tail_check(device, row, relu_shift, epi, R):
    """everything a successful ocr_conv2d_pw_bnbwd_tail_f16 call must have left"""
    n, h, w, c4, c = B_ROWS[row][1]
    accum, form, use_sub = EPILOGUES[epi]
    P = b_operands(row)
    T = P["tail"]
    tag = "%s/s%d/%s" % (row, relu_shift, epi)
    assert bands_untouched(R["dyg"]) and bands_untouched(R["dxg"]) and bands_untouched(R["pg"])
    gdy = _np(R["dy"])
    _note("pw_bnbwd_tail_dy_out", tag, _b_check_dy(P, gdy, relu_shift))
    gdx = _np(R["dx"])
    assert not np.isnan(gdx).any(), "dx: elements not written"
    tail_out = T["out"] if form else None
    ref, k, total = _expect_dx(_conv64(gdy, P["w"], R["d"]), T["old"] if accum else None, T["sub"] if use_sub else None, tail_out)
    big = T["big"] if use_sub else np.zeros(ref.shape, bool)
    _note("pw_bnbwd_tail_dx", tag, _check_dx(gdx, ref, k, total, tail_out, big))
    if form:
        pr = _np(R["part"])
        assert not np.isnan(pr).any(), "partial rows not written"
        _note("pw_bnbwd_tail_partial", tag, _check_partial(pr, gdx, T["by"], T["mean"], T["invstd"]))
        _B_STORED[(row, relu_shift, epi)] = (R["dx"].clone(), R["part"].clone())
    else:
        assert untouched(R["part"]), "`partial` written without a tail"


@pytest.mark.parametrize("row,relu_shift,epi", B_TAIL_CASES)
def test_backward_loader_tail(device, row, relu_shift, epi):
    L, ops = _lib()
    rc, R = _b_tail_launch(L, ops, device, row, relu_shift, epi)
    assert ops.conv2d_variant(R["d"]) == B_ROWS[row][0]
    n, h, w, c4, c = B_ROWS[row][1]
    assert R["rows"] == -(-n * h * w // 256)
    assert rc == OK, rc
    _b_tail_check(device, row, relu_shift, epi, R)
    if epi == "tail_bits":
        # the same mask under the other operand encoding: bit-identical stores (one call against itself, no other route)
        if (row, relu_shift, "tail_out") not in _B_STORED:
            rc2, R2 = _b_tail_launch(L, ops, device, row, relu_shift, "tail_out")
            assert rc2 == OK
            _B_STORED[(row, relu_shift, "tail_out")] = (R2["dx"].clone(), R2["part"].clone())
        dx_o, part_o = _B_STORED[(row, relu_shift, "tail_out")]
        assert torch.equal(R["dx"].view(torch.int16), dx_o.view(torch.int16)), "dx differs between tail_out and bits"
        assert torch.equal(R["part"].view(torch.int32), part_o.view(torch.int32)), "partial differs between tail_out and bits"


@pytest.mark.parametrize("epi", list(EPILOGUES))
def test_backward_loader_tail_cout64(device, epi):
    L, ops = _lib()
    rc, R = _b_tail_launch(L, ops, device, "b64", 1, epi)
    assert ops.conv2d_variant(R["d"]) == B_ROWS["b64"][0] and R["rows"] == 3
    print("conv_fused pw_bnbwd_tail cout64 %s: status %d" % (epi, rc))
    if COUT64_SUPPORTED[epi]:
        assert rc == OK, rc
        _b_tail_check(device, "b64", 1, epi, R)
    else:
        assert rc == UNSUPPORTED, rc
        assert _b_untouched(R, device)


@pytest.mark.parametrize("bn_relu", [0, 1])
@pytest.mark.parametrize("row", list(B_ROWS))
def test_backward_loader_bnred(device, row, bn_relu):
    L, ops = _lib()
    variant, (n, h, w, c4, c) = B_ROWS[row]
    P = b_operands(row)
    T = P["tail"]
    d = _desc(ops, n, h, w, c4, c, 1, "dgrad", 0)
    assert ops.conv2d_variant(d) == variant
    rows = ops.conv2d_num_mtiles(d)
    assert rows == -(-n * h * w // 256)
    dyg, dy = carve((n, h, w, c4), O.STORAGE, Y_BAND, device)
    dxg, dx = carve((n, h, w, c), O.STORAGE, Y_BAND, device)
    pg, part = carve((rows, 2, c), torch.float32, P_BAND, device)
    rc = _rc(L, "ocr_conv2d_pw_bnbwd_bnred_f16", ctypes.byref(d), *_b_loader_args(P, 0, device)[:5], dy, _dev(P["w"], device),
             dx, part, _dev(T["by"], device), _d32(P["bsc"], device), _d32(P["bsh"], device), _d32(T["mean"], device),
             _d32(T["invstd"], device), bn_relu)
    torch.cuda.synchronize()
    assert rc == OK, rc
    assert bands_untouched(dyg) and bands_untouched(dxg) and bands_untouched(pg)
    tag = "%s/r%d" % (row, bn_relu)
    gdy = _np(dy)
    _note("pw_bnbwd_bnred_dy_out", tag, _b_check_dy(P, gdy, 0))
    gdx = _np(dx)
    assert not np.isnan(gdx).any(), "dx: elements not written"
    _note("pw_bnbwd_bnred_dx", tag, _check_y(gdx, _h(_conv64(gdy, P["w"], d)).astype(f64)))
    pr = _np(part)
    assert not np.isnan(pr).any(), "partial rows not written"
    dzm = np.where(P["bn_mask"], gdx, 0.0) if bn_relu else gdx
    unsure = P["bn_unsure"].reshape(-1, c) if bn_relu else None
    _note("pw_bnbwd_bnred_partial", tag, _check_partial(pr, dzm, T["by"], T["mean"], T["invstd"], unsure))


def test_backward_loader_argument_rules(device):
    L, ops = _lib()
    n, h, w, c4, c = B_ROWS["b128"][1]
    # tail pointers partly given
    rc, R = _b_tail_launch(L, ops, device, "b128", 1, "tail_out", tail_override=lambda t: (None,) + t[1:])
    assert rc == INVALID_ARG and _b_untouched(R, device), rc                # bn_y NULL but tail_out set
    rc, R = _b_tail_launch(L, ops, device, "b128", 1, "tail_out", tail_override=lambda t: t[:3] + (None, None, None))
    assert rc == INVALID_ARG and _b_untouched(R, device), rc                # bn_y set but both masks NULL
    for flag in (STATS, BIAS, RELU):
        rc, R = _b_tail_launch(L, ops, device, "b128", 1, "plain", flags=flag)
        assert rc == INVALID_ARG and _b_untouched(R, device), (flag, rc)
    # the shapes the transforming kernel does not take
    P = b_operands("b128")
    for shape, k in (((2, 16, 24, 64, 128), 1), ((1, 5, 5, 128, 128), 1), ((2, 16, 24, 128, 128), 3)):
        nn, hh, ww, ci, co = shape
        d = _desc(ops, nn, hh, ww, ci, co, k, "dgrad", 0)
        rows = ops.conv2d_num_mtiles(d)
        z = torch.zeros((nn, hh, ww, ci), dtype=O.STORAGE, device=device)
        v = torch.ones(ci, device=device)
        dyg, dy = carve((nn, hh, ww, ci), O.STORAGE, Y_BAND, device)
        dxg, dx = carve((nn, hh, ww, co), O.STORAGE, Y_BAND, device)
        pg, part = carve((rows, 2, co), torch.float32, P_BAND, device)
        wk = torch.zeros((k * k, co, ci), dtype=O.STORAGE, device=device)
        rc = _rc(L, "ocr_conv2d_pw_bnbwd_tail_f16", ctypes.byref(d), z, z, v, v, v, None, dy, wk, dx, part, *(None,) * 6)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (shape, rc)
        assert untouched(dy) and untouched(dx) and untouched(part) and bands_untouched(dyg) and bands_untouched(dxg) and bands_untouched(pg)


# ------------------------------------------------------------------------------------------------ part C
def c_operands(ops, row):
    if row not in _OPS:
        n, h, w, cin, cout, k = C_ROWS[row][1]
        rng = _rng("C", row)
        P = {"x": _h(rng.standard_normal((n, h, w, cin))),
             "w": _h(rng.standard_normal((k * k, cout, cin)) * np.sqrt(2.0 / (k * k * cin)))}
        P["tail"] = _tail_operands(rng, n, h, w, cout)
        if row != "t_c64":
            P["conv"] = _conv64(P["x"], P["w"], _desc(ops, n, h, w, cin, cout, k, "dgrad", 0))
        _OPS[row] = P
    return _OPS[row]


def _c_launch(L, ops, device, row, form, accum, use_sub, flags=None, tail_override=None):
    n, h, w, cin, cout, k = C_ROWS[row][1]
    P = c_operands(ops, row)
    T = P["tail"]
    d = _desc(ops, n, h, w, cin, cout, k, "dgrad", (ACCUM if accum else 0) if flags is None else flags)
    rows = ops.conv2d_num_mtiles(d)
    yg, y = carve((n, h, w, cout), O.STORAGE, Y_BAND, device, _dev(T["old"], device) if accum else None)
    pg, part = carve((rows, 2, cout), torch.float32, P_BAND, device)
    targs = _tail_args(T, form, use_sub, device)
    if tail_override is not None:
        targs = tail_override(targs)
    rc = _rc(L, "ocr_conv2d_bnred_tail_f16", ctypes.byref(d), _dev(P["x"], device), _dev(P["w"], device), y, part, *targs)
    torch.cuda.synchronize()
    return rc, dict(d=d, rows=rows, yg=yg, y=y, pg=pg, part=part, accum=accum, old=T["old"])


def _c_untouched(R, device):
    same = torch.equal(R["y"], _dev(R["old"], device)) if R["accum"] else untouched(R["y"])
    return same and untouched(R["part"]) and bands_untouched(R["yg"]) and bands_untouched(R["pg"])


_C_STORED = {}


@pytest.mark.parametrize("row,form,accum,use_sub", C_CASES)
def test_tail_on_plain_kernels(device, row, form, accum, use_sub):
    L, ops = _lib()
    variant, (n, h, w, cin, cout, k) = C_ROWS[row]
    P = c_operands(ops, row)
    T = P["tail"]
    rc, R = _c_launch(L, ops, device, row, form, accum, use_sub)
    assert ops.conv2d_variant(R["d"]) == variant
    assert rc == OK, rc
    assert bands_untouched(R["yg"]) and bands_untouched(R["pg"])
    tag = "%s/%s/a%ds%d" % (row, form, accum, use_sub)
    got = _np(R["y"])
    assert not np.isnan(got).any(), "dx: elements not written"
    ref, kk, total = _expect_dx(P["conv"], T["old"] if accum else None, T["sub"] if use_sub else None, T["out"])
    big = T["big"] if use_sub else np.zeros(ref.shape, bool)
    _note("bnred_tail_dx", tag, _check_dx(got, ref, kk, total, T["out"], big))
    pr = _np(R["part"])
    assert pr.shape[0] == ops.conv2d_num_mtiles(R["d"])
    assert not np.isnan(pr).any(), "partial rows not written: %s" % sorted(set(np.nonzero(np.isnan(pr))[0].tolist()))[:16]
    _note("bnred_tail_partial", tag, _check_partial(pr, got, T["by"], T["mean"], T["invstd"]))
    # the two encodings of the same mask store the same bits (1x1 rows: both forms are in the cross)
    other = _C_STORED.get((row, "out" if form == "bits" else "bits", accum, use_sub))
    if other is not None:
        assert torch.equal(R["y"].view(torch.int16), other[0].view(torch.int16)), "dx differs between tail_out and bits"
        assert torch.equal(R["part"].view(torch.int32), other[1].view(torch.int32)), "partial differs between tail_out and bits"
    _C_STORED[(row, form, accum, use_sub)] = (R["y"].clone(), R["part"].clone())


@pytest.mark.parametrize("form,accum,use_sub", [("out", 0, 0), ("bits", 1, 1)])
def test_tail_refused_on_the_persistent_kernel(device, form, accum, use_sub):
    L, ops = _lib()
    rc, R = _c_launch(L, ops, device, "t_c64", form, accum, use_sub)
    assert ops.conv2d_variant(R["d"]) == C_ROWS["t_c64"][0]
    assert rc == UNSUPPORTED, rc
    assert _c_untouched(R, device)


def test_tail_argument_rules(device):
    L, ops = _lib()
    for flag in (BIAS, RELU):
        rc, R = _c_launch(L, ops, device, "t_pw64", "out", 0, 0, flags=flag)
        assert rc == INVALID_ARG and _c_untouched(R, device), (flag, rc)
    rc, R = _c_launch(L, ops, device, "t_pw64", "out", 0, 0, tail_override=lambda t: t[:3] + (None, None) + t[5:])
    assert rc == INVALID_ARG and _c_untouched(R, device), rc               # both masks NULL


# ------------------------------------------------------------------------------------------------ part D
def d_operands(ops, name):
    if ("D", name) not in _OPS:
        n, h, w = D_SHAPES[name]
        rng = _rng("D", name)
        P = {"x": _h(rng.standard_normal((n, h, w, 64))), "w": _h(rng.standard_normal((9, 64, 64)) * np.sqrt(2.0 / (9 * 64))),
             "bias": (0.5 * rng.standard_normal(64)).astype(f32)}
        P["conv"] = _conv64(P["x"], P["w"], _desc(ops, n, h, w, 64, 64, 3, "fwd", 0))
        _OPS[("D", name)] = P
    return _OPS[("D", name)]


def _d_launch(L, ops, device, shape, cin, cout, P, flags, with_argmax):
    n, h, w = shape
    d = _desc(ops, n, h, w, cin, cout, 3, "fwd", flags)
    ph, pw = (h + 1) // 2, (w + 1) // 2
    pg, pooled = carve((n, ph, pw, cout), O.STORAGE, Y_BAND, device)
    am = Bytes(n * ph * pw * cout, 2048, device)
    rc = _rc(L, "ocr_conv2d_relu_pool_f16", ctypes.byref(d), _dev(P["x"], device), _dev(P["w"], device),
             _d32(P["bias"], device) if flags & BIAS else None, pooled, am.t if with_argmax else None)
    torch.cuda.synchronize()
    return rc, dict(d=d, pg=pg, pooled=pooled, am=am)


@pytest.mark.parametrize("with_argmax", [1, 0])
@pytest.mark.parametrize("flags", list(POOL_SUPPORTED))
@pytest.mark.parametrize("name", list(D_SHAPES))
def test_pooled_conv(device, name, flags, with_argmax):
    L, ops = _lib()
    n, h, w = D_SHAPES[name]
    P = d_operands(ops, name)
    rc, R = _d_launch(L, ops, device, D_SHAPES[name], 64, 64, P, flags, with_argmax)
    assert ops.conv2d_variant(R["d"]) == "conv_c64_persist_kernel<64>"
    print("conv_fused relu_pool %s flags %d: status %d" % (name, flags, rc))
    if not POOL_SUPPORTED[flags]:
        assert rc == UNSUPPORTED, rc
        assert untouched(R["pooled"]) and bands_untouched(R["pg"]) and R["am"].untouched()
        return
    assert rc == OK, rc
    assert bands_untouched(R["pg"]) and R["am"].bands()
    tag = "%s/f%d/i%d" % (name, flags, with_argmax)
    pre = P["conv"] + (P["bias"].astype(f64) if flags & BIAS else 0.0)
    act = np.maximum(pre, 0.0) if flags & RELU else pre
    ph, pw = (h + 1) // 2, (w + 1) // 2
    full = np.full((n, 2 * ph, 2 * pw, 64), -np.inf)
    full[:, :h, :w] = act
    cand = np.stack([full[:, 0::2, 0::2], full[:, 0::2, 1::2], full[:, 1::2, 0::2], full[:, 1::2, 1::2]], 0)
    ref = cand.max(0)
    bound = T1 * np.abs(ref).max()
    got = _np(R["pooled"])
    assert not np.isnan(got).any(), "pooled: elements not written"
    _note("relu_pool_pooled", tag, _ratio(np.abs(got - ref), bound))
    dead = None
    if flags & RELU:
        fpre = np.full((n, 2 * ph, 2 * pw, 64), -np.inf)
        fpre[:, :h, :w] = pre
        dead = np.stack([fpre[:, 0::2, 0::2], fpre[:, 0::2, 1::2], fpre[:, 1::2, 0::2], fpre[:, 1::2, 1::2]], 0).max(0) < -bound
        assert (got[dead] == 0).all(), "a window with nothing positive does not store 0"
    if with_argmax:
        idx = R["am"].t.cpu().numpy().reshape(n, ph, pw, 64)
        assert (idx < 4).all(), "argmax bytes not written or out of range"
        at = np.take_along_axis(cand, idx[None].astype(np.int64), 0)[0]
        assert np.isfinite(at).all(), "argmax names a position that does not exist"
        _note("relu_pool_argmax", tag, _ratio(ref - at, 2 * bound))
        if dead is not None:
            assert (idx[dead] == 0).all(), "first maximum of an all-zero window is position 0"
    else:
        assert R["am"].untouched()


def test_pooled_conv_refusals(device):
    L, ops = _lib()
    rng = _rng("D-refused")
    for shape, cin, cout in (((2, 12, 24), 64, 64), ((2, 100, 130), 64, 128), ((2, 100, 130), 128, 64)):
        n, h, w = shape
        P = {"x": _h(rng.standard_normal((n, h, w, cin))), "w": _h(rng.standard_normal((9, cout, cin)) * 0.05),
             "bias": np.zeros(cout, f32)}
        rc, R = _d_launch(L, ops, device, shape, cin, cout, P, BIAS | RELU, 1)
        assert rc == UNSUPPORTED, (shape, cin, cout, rc)
        assert untouched(R["pooled"]) and bands_untouched(R["pg"]) and R["am"].untouched()
    P = d_operands(ops, "even")
    for flag in (STATS, ACCUM):
        rc, R = _d_launch(L, ops, device, D_SHAPES["even"], 64, 64, P, BIAS | RELU | flag, 1)
        assert rc == INVALID_ARG, (flag, rc)
        assert untouched(R["pooled"]) and bands_untouched(R["pg"]) and R["am"].untouched()
