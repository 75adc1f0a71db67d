"""GPU: every convolution kernel family x every epilogue setting the C ABI accepts, each against a float64
restatement on the same 16-bit-exact operands (torch / numpy on the CPU; no device route is compared with another).

Families (asserted through ocr_conv2d_variant, so a change of the selection rules cannot move the matrix):
conv3x3_w4_kernel (one and two cout tiles), conv3x3_w4s_kernel<128> / <64> (even and odd chunk pairs),
conv_c64_persist_kernel<64>, conv_pw_kernel<256,4> (ragged last flat tile; and the cin = 64 shape whose tile the
dispatcher switches between 128 and 256 couts with the epilogue's global operands), conv_pw_kernel<64,1>, and the
generic conv_igemm_kernel tiles (1x1 on a pixel count that is no multiple of 32, dilation 6, 32-wide tiles on
32-channel chunks, 16-row tiles, stride 2 with SAME padding).

Modes: A STATS, B BIAS|RELU, C BIAS, D BIAS|RELU|STATS (forward form); E ACCUM_F16, F ACCUM_F16|STATS (input-gradient
form: flip_taps = 1, pads as layers._conv_dgrad computes them); G / H / I the fused BN-backward reduction
(ocr_conv2d_bnred_f16: raw store, masked store, no ReLU) and J the same entry with ACCUM_F16, which the product never
issues: per family either the correct result or OCR_ERR_UNSUPPORTED.  The launch descriptor of a family is the same in
both forms (its weights are drawn directly in the [tap][cout][cin] operand layout), so every mode of a row runs the
row's kernel.

Where the kernels round (conv_epilogue.h and the three wave-private epilogues agree): the f32 accumulator + bias,
after the ReLU, is rounded to the storage type ONCE; under ACCUM_F16 that rounded value + the value that was there is
rounded again; the masked store zeroes afterwards; the partial sums are taken of the STORED 16-bit values in f32.

Bars: one output rounding 1e-3 (f16) / 8e-3 (bf16) of max|ref| as in test_conv_fwd_dgrad_wgrad; two roundings
1.5e-3 / 8e-3 as in test_bottleneck_tail_conv_vs_numpy.  Partial sums: rtol / atol of
test_special_kernels_are_selected_and_emit_stats.

Every output and partial buffer is carved out of a larger allocation with sentinel guard bands of one tile's worth of
elements on each side (what ragged tiles write outside the tensor would show there), and is pre-filled with NaN where
the launch does not read it: the product hands these kernels uninitialised buffers, so every element and every
partial row must be written."""
import numpy as np
import pytest
import torch

from matrix_support import _h, _rng, bands_untouched, carve
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

# name: (expected variant, (n, h, w, cin, cout, k, dilation, stride)) — the LAUNCH descriptor's channels
FAMILIES = {
    "w4_256": ("conv3x3_w4_kernel", (2, 33, 70, 128, 256, 3, 1, 1)),            # ragged rows and columns, 2 chunks
    "w4_512": ("conv3x3_w4_kernel", (2, 12, 40, 128, 512, 3, 1, 1)),            # two cout tiles
    "w4s_128": ("conv3x3_w4s_kernel<128>", (2, 21, 45, 128, 384, 3, 1, 1)),     # two chunk pairs, three cout tiles
    "w4s_64": ("conv3x3_w4s_kernel<64>", (2, 19, 40, 128, 192, 3, 1, 1)),       # two chunk pairs, three cout tiles
    "w4s_64_odd": ("conv3x3_w4s_kernel<64>", (2, 13, 40, 192, 64, 3, 1, 1)),    # three chunk pairs (odd)
    "c64": ("conv_c64_persist_kernel<64>", (2, 100, 130, 64, 64, 3, 1, 1)),     # 130 ragged pixel tiles (needs >= 128)
    "pw_256": ("conv_pw_kernel<256,4>", (2, 24, 40, 256, 512, 1, 1, 1)),        # 7.5 flat tiles, 4 K stages, 2 cout tiles
    "pw_256_cin64": ("conv_pw_kernel<256,4>", (2, 12, 40, 64, 256, 1, 1, 1)),   # 128-cout tiles unless the epilogue loads
    "pw_64": ("conv_pw_kernel<64,1>", (2, 12, 24, 128, 192, 1, 1, 1)),          # 2.25 flat tiles, three cout tiles
    "ig_1x1": ("conv_igemm_kernel<256,64,4,0,8>", (2, 9, 37, 128, 512, 1, 1, 1)),     # 666 pixels: not the GEMM kernel
    "ig_dil6": ("conv_igemm_kernel<128,32,2,1,16>", (2, 12, 20, 128, 384, 3, 6, 1)),  # fc6-style dilation (28 x 44 halo), 3 cout tiles
    "ig_32": ("conv_igemm_kernel<32,32,1,1,8>", (2, 17, 19, 96, 160, 3, 1, 1)),       # 32-wide tiles, 32-channel chunks
    "ig_16row": ("conv_igemm_kernel<128,32,2,1,16>", (2, 24, 33, 96, 384, 3, 1, 1)),   # 16-row tile, second tile half empty
    "ig_stride2": ("conv_igemm_kernel<256,32,4,1,8>", (2, 18, 36, 64, 256, 3, 1, 2)), # SAME padding 0 before / 1 after
}

BIAS, RELU, STATS, ACCUM = 1, 2, 4, 8
# mode: (entry, form, flags, store_masked, bn_relu)
MODES = {
    "A": ("conv2d", "fwd", STATS, 0, 0),
    "B": ("conv2d", "fwd", BIAS | RELU, 0, 0),
    "C": ("conv2d", "fwd", BIAS, 0, 0),
    "D": ("conv2d", "fwd", BIAS | RELU | STATS, 0, 0),
    "E": ("conv2d", "dgrad", ACCUM, 0, 0),
    "F": ("conv2d", "dgrad", ACCUM | STATS, 0, 0),
    "G": ("bnred", "dgrad", 0, 0, 1),
    "H": ("bnred", "dgrad", 0, 1, 1),
    "I": ("bnred", "dgrad", 0, 0, 0),
    "J": ("bnred", "dgrad", ACCUM, 0, 1),
}
# mode H in the bias-net form (the activation itself as bn_y, scale 1, shift 0, mean 0, invstd 1: PixelLink's
# conv1_2 -> conv1_1 gradient runs on exactly this kernel); general BN parameters on every other family
BIAS_NET_FAMILY = "c64"
# mode J: what each family does with ACCUM_F16 under the fused reduction — True: the correct result (two roundings,
# sums of the stored values under the mask); False: OCR_ERR_UNSUPPORTED.  Anything else is a bug.
J_SUPPORTED = {f: True for f in FAMILIES}

# stride-2 shapes take the forward modes only (layers._conv_dgrad refuses strided input gradients)
CASES = [(f, m) for f in FAMILIES for m in MODES if not (FAMILIES[f][1][7] != 1 and MODES[m][1] == "dgrad")]

Y_BAND = 16 * 32 * 256          # elements: the largest tile (16 rows x 32 columns x 256 couts)
P_BAND = 2 * 512 * 4            # floats: four partial rows of the widest layer

_REF = {}                       # (family, form) -> (x, w_kc, float64 convolution), computed once per shape


def _desc(ops, shape, form, flags):
    """The launch descriptor: SAME padding from ops.conv_desc; the input-gradient form flips the taps and takes the
    pads layers._conv_dgrad computes."""
    n, h, w, cin, cout, k, dil, stride = shape
    d = ops.conv_desc((n, h, w, cin), cout, k, k, stride, dil)
    if form == "dgrad":
        assert stride == 1
        d.pad_top = dil * (k - 1) - d.pad_top
        d.pad_left = dil * (k - 1) - d.pad_left
        d.flip_taps = 1
    d.flags = flags
    return d


def _reference(ops, family, form):
    """16-bit-exact operands of the shape and their float64 convolution (torch on the CPU, explicit padding):
    y[n, oy, ox, co] = sum x[n, oy*s + ky*dil - pt, ox*s + kx*dil - pl, ci] * w_kc[tap(ky, kx)][co][ci], the tap
    index mirrored under flip_taps."""
    key = (family, form)
    if key not in _REF:
        shape = FAMILIES[family][1]
        n, h, w, cin, cout, k, dil, stride = shape
        d = _desc(ops, shape, form, 0)
        rng = _rng(shape, form)
        x = _h(rng.standard_normal((n, h, w, cin)))
        wk = _h(rng.standard_normal((k * k, cout, cin)) * np.sqrt(2.0 / (k * k * cin)))
        wt = torch.from_numpy(wk).double().reshape(k, k, cout, cin)
        if d.flip_taps:
            wt = wt.flip(0, 1)
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        pad = (d.pad_left, max(0, (d.ow - 1) * stride + (k - 1) * dil + 1 - w - d.pad_left),
               d.pad_top, max(0, (d.oh - 1) * stride + (k - 1) * dil + 1 - h - d.pad_top))
        ref = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, pad), wt.permute(2, 3, 0, 1).contiguous(),
                                         stride=stride, dilation=dil).permute(0, 2, 3, 1).contiguous().numpy()
        assert ref.shape == (n, d.oh, d.ow, cout)
        _REF[key] = (x, wk, ref)
    return _REF[key]


def _bn_inputs(rng, shape_out, cout, bias_net):
    """bn_y and the producing layer's BN parameters; the float64 pre-activation z and the set of elements whose sign
    an f32 evaluation may see differently (within 2e-5 of the terms' magnitudes of the threshold)."""
    if bias_net:
        by = _h(np.maximum(rng.standard_normal(shape_out), 0.0))         # the activation itself: half of it exact zeros
        scale, shift = np.ones(cout, np.float32), np.zeros(cout, np.float32)
        mean, invstd = np.zeros(cout, np.float32), np.ones(cout, np.float32)
    else:
        by = _h(rng.standard_normal(shape_out))
        scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        scale[5] = -0.8                                                   # negative scales: the mask is NOT by > const
        scale[cout - 3] = -1.1                                            # ... one in the last cout tile as well
        shift = rng.normal(0, 0.3, cout).astype(np.float32)
        mean = rng.normal(0, 0.2, cout).astype(np.float32)
        invstd = rng.uniform(0.7, 1.3, cout).astype(np.float32)
    a = by.astype(np.float64) * scale.astype(np.float64)
    z = a + shift.astype(np.float64)
    unsure = np.abs(z) < 2e-5 * (np.abs(a) + np.abs(shift.astype(np.float64)))
    return by, scale, shift, mean, invstd, z, unsure


def bn_unsure_share(family, mode):
    """CPU only: the share of elements excluded from the exact mask comparison for the case's seed."""
    n, h, w, cin, cout, k, dil, stride = FAMILIES[family][1]
    rng = _rng(FAMILIES[family][1], mode)
    rng.standard_normal((n, h, w, cout))                                  # (`old` is drawn first in every case)
    unsure = _bn_inputs(rng, (n, h, w, cout), cout, mode == "H" and family == BIAS_NET_FAMILY)[6]
    return float(unsure.mean())


@pytest.mark.parametrize("family,mode", CASES)
def test_conv_epilogue_vs_float64(device, family, mode):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd._lib import OcrHipError
    variant, shape = FAMILIES[family]
    entry, form, flags, store_masked, bn_relu = MODES[mode]
    n, h, w, cin, cout, k, dil, stride = shape
    d = _desc(ops, shape, form, flags)
    assert ops.conv2d_variant(d) == variant
    x, wk, conv = _reference(ops, family, form)
    oshape = (n, d.oh, d.ow, cout)
    bf16 = O.STORAGE == torch.bfloat16
    accum = bool(flags & ACCUM)
    tol = 8e-3 if bf16 else (1.5e-3 if accum else 1e-3)

    rng = _rng(shape, mode)
    old = _h(rng.standard_normal(oshape) * 0.5)
    dev16 = lambda a: torch.from_numpy(a).to(O.STORAGE).to(device)
    f32 = lambda a: torch.from_numpy(a).to(device)
    xd, wd = dev16(x), dev16(wk)
    yg, y = carve(oshape, O.STORAGE, Y_BAND, device, dev16(old) if accum else float("nan"))
    want_partial = entry == "bnred" or bool(flags & STATS)
    T = ops.conv2d_num_mtiles(d)
    pg, part = carve((T, 2, cout), torch.float32, P_BAND, device, float("nan"))

    pre = conv                                                            # float64 value in front of the ReLU
    bias = None
    if flags & BIAS:
        # N(0,1), the scale of the outputs themselves: a bias vector shifted by a few channels or swapped between
        # the halves of a cout tile moves the output by O(1), three orders above the bar of assertion 1
        bias = rng.standard_normal(cout).astype(np.float32)
        pre = conv + bias.astype(np.float64)
    ref = np.maximum(pre, 0.0) if flags & RELU else pre
    if accum:
        ref = _h(_h(ref).astype(np.float64) + old).astype(np.float64)     # round the convolution, add, round again

    unsure = np.zeros(oshape, bool)
    if entry == "conv2d":
        ops.conv2d(d, xd, wd, y, f32(bias) if bias is not None else None, part if want_partial else None)
    else:
        by, scale, shift, mean, invstd, z, unsure = _bn_inputs(rng, oshape, cout,
                                                               mode == "H" and family == BIAS_NET_FAMILY)
        share = float(unsure.mean())
        assert share <= 1e-4, share
        mask = (z > 0) if bn_relu else np.ones(oshape, bool)
        if not bn_relu:
            unsure = np.zeros(oshape, bool)
        ctx = (dev16(by), f32(scale), f32(shift), f32(mean), f32(invstd), bool(bn_relu))
        if mode == "J" and not J_SUPPORTED[family]:
            with pytest.raises(OcrHipError, match=r"\(-2\)"):
                ops.conv2d_bnred(d, xd, wd, y, part, ctx, store_masked=bool(store_masked))
            torch.cuda.synchronize()
            assert torch.equal(y, dev16(old)) and bands_untouched(yg) and bands_untouched(pg)
            print("%s %s variant %s: refused (OCR_ERR_UNSUPPORTED)" % (family, mode, variant))
            return
        ops.conv2d_bnred(d, xd, wd, y, part, ctx, store_masked=bool(store_masked))
    torch.cuda.synchronize()

    got = y.float().cpu().numpy().astype(np.float64)
    if store_masked:
        # 5. outside the undecided set: exactly 0 where the mask is false, the reference value where it is true;
        # inside it either of the two
        err_t = np.abs(got - ref)
        ref = np.where(mask, ref, 0.0)
    m = np.abs(ref).max()
    if store_masked:
        sure_f = ~mask & ~unsure
        masked_exact = bool((got[sure_f] == 0).all())
        err = np.where(mask & ~unsure, err_t, 0.0)
        err = np.maximum(err, np.where(unsure, np.minimum(err_t, np.abs(got)), 0.0))
        e_y = float(np.nanmax(err) / m) if np.isfinite(got).all() else float("nan")
    else:
        masked_exact = True
        e_y = float(np.abs(got - ref).max() / m)

    e_s = [0.0, 0.0]
    stats_ok = True
    if want_partial:
        sums = part.cpu().numpy().astype(np.float64).sum(0)
        if entry == "conv2d":
            # 4. the sums are of the STORED values (held to the reference by assertion 1)
            want = [got.sum((0, 1, 2)), (got * got).sum((0, 1, 2))]
            bars = [(1e-4, 1e-2), (1e-4, 1e-8)]
            slack = [0.0, 0.0]
        else:
            dz = np.where(mask, got, 0.0)
            xh = (by.astype(np.float64) - mean) * invstd
            want = [dz.sum((0, 1, 2)), (dz * xh).sum((0, 1, 2))]
            bars = [(1e-3, 5e-2), (1e-3, 5e-2)]
            # an undecided element counts on either side: at most its own magnitude per channel
            slack = [np.where(unsure, np.abs(got), 0.0).sum((0, 1, 2)), np.where(unsure, np.abs(got * xh), 0.0).sum((0, 1, 2))]
        for i in range(2):
            diff = np.abs(sums[i] - want[i])
            e_s[i] = float(np.nanmax(diff / (np.abs(want[i]) + 1.0))) if np.isfinite(sums).all() else float("nan")
            stats_ok = stats_ok and bool((diff <= bars[i][1] + bars[i][0] * np.abs(want[i]) + slack[i]).all())
    print("%s %s variant %s: y %.2e s0 %.2e s1 %.2e" % (family, mode, variant, e_y, e_s[0], e_s[1]))

    # 6. every element and every partial row written
    assert np.isfinite(got).all(), "%d elements of y not written" % int((~np.isfinite(got)).sum())
    if want_partial:
        pr = part.cpu().numpy()
        assert np.isfinite(pr).all(), "partial rows not written: %s" % sorted(set(np.nonzero(~np.isfinite(pr))[0].tolist()))[:16]
    else:
        assert bool(torch.isnan(part).all())                              # ... and not touched without STATS
    # 7. nothing written outside the tensors
    assert bands_untouched(yg), "stores outside y"
    assert bands_untouched(pg), "stores outside the partial rows"
    # 1. the stored tensor
    assert e_y < tol, (e_y, tol)
    assert masked_exact, "masked store: non-zero values where the ReLU mask is false"
    # 2. the ReLU is exact away from the rounding of its argument
    if flags & RELU:
        assert (got[pre < -tol * m] == 0).all() and (got[pre > tol * m] > 0).all()
        assert (got >= 0).all()
    # 4.
    assert stats_ok, (e_s, sums, want)
