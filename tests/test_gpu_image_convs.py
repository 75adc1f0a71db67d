"""GPU: the two convolutions that read the image itself — conv1_1 of VGG / PixelLink (csrc/conv_first.hip: 3x3, cin 3)
and the ResNet root (csrc/conv_stem.hip: 7x7, stride 2, explicit (3,3) padding) — every entry of the C ABI against a
float64 restatement on the same 16-bit-exact operands (numpy on the CPU: the image padded explicitly, one einsum per
tap, no autograd).  No device route is compared with another except where bit identity is the documented contract:
the statistics-only forward == the storing one, ocr_conv2d_first_bn_relu_f16 == ocr_bn_relu_f16 on the stored y, the
`w_first` (recomputing) fused weight gradient == the `bn_y` form on the forward's y.

Rows (n, h, w, cout); tiles are 8 rows x 32 columns of OUTPUT, the counts asserted against ocr_conv2d_*_num_mtiles:
  row       first 3x3          stem 7x7/2          tiles  what it reaches
  one       (1, 1, 1, 64)      (1, 1, 1, 64)         1    one output; the halo is padding but for one pixel
  tile      (1, 8, 32, 64)     (1, 16, 64, 64)       1    exactly one full tile (stem: even input extents)
  tile_odd  -                  (1, 15, 63, 64)       1    ... on odd input extents
  four      (1, 9, 33, 64)     (1, 17, 65, 64)       4    four tiles, three holding one row / column
  layer     (2, 20, 45, 64)    (2, 38, 70, 64)      12    the shapes of the layer tests, at matrix bars
  cout128   (2, 20, 45, 128)   (2, 38, 70, 128)     12    two cout tiles
  cap       (2, 4117, 5, 64)   (2, 8233, 9, 64)   1030    > 512: the weight-gradient workgroups take 2 or 3 tiles, the
                                                          image index changing between trips (first layer: the next
                                                          tile's dy prefetched into registers; the stem loads dy at
                                                          the top of each trip); > 1024: the first layer's moments
                                                          take a second trip
Forms per row: the forward under flags 0, BIAS, BIAS|RELU, STATS, BIAS|RELU|STATS (first layer: also y = NULL);
ocr_conv2d_first_bn_relu_f16 (relu on / off, a tenth of the scales negative); the plain weight gradients; the fused
ones (bn_y, w_first, stem; relu on / off, general A, B, C, shift); the moments on `layer` and `cap`; the packers on
general f32 weights, bit for bit against the documented [3][cout][16] / [7][2][cout][16] layouts, zero slots included.
One more row feeds ocr_prep_images_f16's own output through the forward check.  Impulse rows (a dozen single-channel
small integers in the image: its four corners, the middle of its last row and column on an even- and an odd-sized
stem map, the four pixels around a tile corner; weights / dy dense multiples of 1/64 below 2) are exact in f32 in any
order, so y and dw must equal the float64 result BIT FOR BIT: they pin the tap order, the stride-2 origin, the pad
offsets and the cout-block mapping, which the random rows can only bound.

Where the kernels round (conv_epilogue.h): f32 accumulator + bias, after the ReLU, rounded ONCE; the partial sums are
taken of the stored 16-bit values.  The fused weight gradients: dz = da * [fma(y, A, shift) > OCR_RELU_TIE],
dy16 = round16(fma(A, dz, fma(B, y, C))), restated with a correctly rounded f32 fma (the exact product, the exact
error of the float64 sum, one rounding) — the float64 dw of dy16 is then the reference.  Conditions on the inputs,
asserted on the CPU from the reference alone: no mask argument within one f32 ulp of the threshold (every row); no
float64 intermediate of an fma on an f32 rounding midpoint with a non-zero residual (every row: the only way the
restated fma can differ from the hardware's); no pre-rounding dy within one f32 ulp of a 16-bit rounding boundary on
the rows of at most 20 000 elements, whose seed is searched for it.  On the larger rows no seed can satisfy the last
one — the share of f32 values that close to a boundary is 2 * 2^-13 (f16) / 2 * 2^-16 (bf16), 28 / 3.5 expected
elements on `layer` already — and the midpoint condition, which is sharp, stands alone.

Bars (the project's own): forward 1e-3 (f16) / 8e-3 (bf16) of max|ref|; two roundings (first_bn_relu) 1.5e-3 / 8e-3;
partial sums rtol 1e-4, atol 1e-2 (sums) / 1e-8 (squares) as test_special_kernels_are_selected_and_emit_stats; weight
gradients 5e-6 of max|ref| in both builds (on the cap rows the test first confirms on the CPU that a sequential f32 sum
of the same terms stays inside it); moments' statistics row as test_first_conv_statistics_from_the_image_moments
(mean 1e-5 of a standard deviation, variance 1e-5 relative); moments_f64 element-wise within
(64 * trips + 3) * 2^-24 * sum|terms| — the f32 chain of one element: a wave adds its 64 pixels of every tile (four
MFMAs of 16, each product counted as one addition), the four waves meet in 3 more; f64 across workgroups — and the pixel
count exact.

Measured, largest per kernel over its rows (f16 / bf16 library):
  conv_first_kernel<false> y            4.3e-04 / 3.5e-03      conv_stem_kernel y                  4.8e-04 / 3.5e-03
  conv_first_kernel<true> a             3.8e-04 / 3.0e-03      conv_stem_wgrad_kernel<false>       1.7e-07 / 1.2e-07
  conv_first_wgrad_kernel<false>        1.4e-07 / 1.1e-07      conv_stem_wgrad_kernel<true>        1.1e-07 / 1.1e-07
  conv_first_wgrad_kernel<true,false>   1.1e-07 / 9.7e-08      first_moments: mean 1.8e-08 / 1.4e-08 sd, variance
  conv_first_wgrad_kernel<true,true>    bit-identical to <true,false>    5.8e-08 / 6.3e-08, M 0.007 / 0.018 of its bound
The fused kernels round every dy element to f32 and then to 16 bits (an empty asm on the f32 value keeps the compiler
from fusing the fma and the conversion of part of the elements into v_fma_mixlo/hi_f16, which rounds once); the stem's
`layer` and `cout128` rows are the ones that tell the two apart at this bar.

What the rows catch, each break tried once on a scratch build of the f16 library (never committed):
  * the stem halo origin shifted by one pixel: every stem row of the forward, the plain and the fused weight gradient,
    and the stem impulse rows (forward and weight gradient) — 25 cases;
  * kx / c swapped in the first layer's packer: the packer layout test, every first-layer forward, bn_relu, fused
    (y differs) and moments row, and the first-layer forward impulse row — 24 cases;
  * the kw = 1 partial row dropped from the first layer's row sum: every first-layer plain and fused row but `one`
    (whose single pixel lies in the kw = 0 half) and the first-layer weight-gradient impulse row — 11 cases;
  * the barrier at the top of the persistent loop removed (first layer, stem; one build each): NOTHING fails, the cap
    rows included.  The only hazard it guards is a wave that finished its MFMAs overwriting `dyt` while another still
    reads it, and the fast wave has a global-memory round trip (the halo, in the stem the dy rows) to wait out first,
    against eight MFMAs of the slow one: the race does not show.  The cap rows do test the accumulation across trips,
    the prefetch and the change of image between trips (a wrong value there is caught as any other); the barrier itself
    stays UNTESTED by this file, and no row is known that would make its absence observable.

Every output, workspace and partial buffer is NaN-filled and carved out of a larger allocation with sentinel bands on
both sides; every element must be written and the bands left alone.  Error returns (one test for both files) must
leave the NaN-filled outputs untouched: nothing is launched on an argument error.

Out of scope: ocr_conv2d_bnred_first_f16, ocr_conv2d_bnred_first_wgrad_f16 and ocr_conv2d_first_wgrad_sums_f32 run on
the 64-channel persistent igemm kernel, not in these two files (their tests: test_gpu_layers.py); ocr_conv2d_stem_f16
requires y — it has no statistics-only form (asserted: INVALID_ARG)."""
import ctypes

import numpy as np
import pytest
import torch

from matrix_support import (BF16, INVALID_ARG, OK, UNSUPPORTED, WORKSPACE, _h, _rng, _seed, bands_untouched, carve, untouched,
                            written)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

BIAS, RELU, STATS = 1, 2, 4
FLAG_MODES = (0, BIAS, BIAS | RELU, STATS, BIAS | RELU | STATS)
RELU_TIE = 2.0 ** -134 if BF16 else 2.0 ** -25          # OCR_RELU_TIE (csrc/common.h)
GEOM = {"first": (3, 1, 1), "stem": (7, 2, 3)}          # kernel extent, stride, padding
# kind -> row -> ((n, h, w, cout), tiles)
ROWS = {
    "first": {"one": ((1, 1, 1, 64), 1), "tile": ((1, 8, 32, 64), 1), "four": ((1, 9, 33, 64), 4),
              "layer": ((2, 20, 45, 64), 12), "cout128": ((2, 20, 45, 128), 12), "cap": ((2, 4117, 5, 64), 1030)},
    "stem": {"one": ((1, 1, 1, 64), 1), "tile": ((1, 16, 64, 64), 1), "tile_odd": ((1, 15, 63, 64), 1),
             "four": ((1, 17, 65, 64), 4), "layer": ((2, 38, 70, 64), 12), "cout128": ((2, 38, 70, 128), 12),
             "cap": ((2, 8233, 9, 64), 1030)},
}
CASES = [(k, r) for k in ROWS for r in ROWS[k]]
IMPULSE = [("first", (2, 9, 33, 128)), ("stem", (2, 38, 70, 128)), ("stem", (1, 17, 65, 128))]
MOMENT_ROWS = ("layer", "cap")
SEED_SEARCHED = 20000           # elements: the fused rows whose seed is searched for the one-ulp condition
N_TESTS = 3 * len(CASES) + len(ROWS["first"]) + len(MOMENT_ROWS) + 2 * len(IMPULSE) + 4 + 2

WG_CAP, MOMENT_CAP = 512, 1024  # wgrad_blocks / stem_blocks, FM_WGS
WGRAD_BAR = 5e-6
# the cap rows' dy: chosen on the CPU per storage type (see _operands); sequential f32 sum / bar with these seeds:
# first 0.91 (f16) 0.62 (bf16), stem 0.99 (f16) 0.84 (bf16)
CAP_DY_SEED = {"first": 1, "stem": 5 if BF16 else 2}
Y_TOL = 8e-3 if BF16 else 1e-3
A_TOL = 8e-3 if BF16 else 1.5e-3

_REF = {}


def _out(kind, h, w):
    k, s, pad = GEOM[kind]
    return (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1


def _taps(kind, x):
    """(ky, kx, x[n, oy*s + ky - pad, ox*s + kx - pad, :] as [n, oh, ow, 3] float64) per tap, from an explicitly
    zero-padded copy of the image."""
    k, s, pad = GEOM[kind]
    n, h, w, _ = x.shape
    oh, ow = _out(kind, h, w)
    xp = np.zeros((n, max((oh - 1) * s + k, pad + h), max((ow - 1) * s + k, pad + w), 3), np.float64)
    xp[:, pad:pad + h, pad:pad + w] = x
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, np.ascontiguousarray(xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s])


def _conv_float64(kind, x, w_hwio):
    n, h, w, _ = x.shape
    y = np.zeros((n,) + _out(kind, h, w) + (w_hwio.shape[-1],), np.float64)
    for ky, kx, xs in _taps(kind, x):
        y += np.einsum("nyxc,co->nyxo", xs, w_hwio[ky, kx].astype(np.float64))
    return y


def _dw_float64(kind, x, dy):
    k = GEOM[kind][0]
    dw = np.empty((k, k, 3, dy.shape[-1]), np.float64)
    dy64 = dy.astype(np.float64)
    for ky, kx, xs in _taps(kind, x):
        dw[ky, kx] = np.einsum("nyxc,nyxo->co", xs, dy64)
    return dw


def _operands(kind, row):
    """x [n,h,w,3] like mean-subtracted pixels rounded to storage, w [k,k,3,cout] 16-bit exact, their float64
    convolution, dy for the plain weight gradient and its float64 dw: drawn and computed once per row."""
    key = (kind, row)
    if key not in _REF:
        (n, h, w, cout), _ = ROWS[kind][row]
        k = GEOM[kind][0]
        rng = _rng(kind, row)
        x = _h(rng.integers(0, 256, (n, h, w, 3)) - np.array([123.68, 116.78, 103.94]))
        wt = _h(rng.standard_normal((k, k, 3, cout)) * np.sqrt(2.0 / (k * k * 3)) / 64.0)
        conv = _conv_float64(kind, x, wt)
        dy = rng.standard_normal(conv.shape) * 0.25
        if row == "cap":
            # a sequential f32 sum of 41 170 terms fits the weight-gradient bar for some draws only (3e-6 .. 1e-5 of
            # max|ref| over seeds, whatever the distribution; the kernels, which sum by tiles, are at 1e-7): dy has
            # zero mean per channel and a seed chosen on the CPU so that it does (asserted in
            # test_plain_wgrad_vs_float64)
            dy = _rng(kind, "cap", "dy", CAP_DY_SEED[kind]).standard_normal(conv.shape) * 0.25
            dy -= dy.mean((0, 1, 2))
        dy = _h(dy)
        _REF[key] = dict(x=x, w=wt, conv=conv, dy=dy, dw=_dw_float64(kind, x, dy))
        for a in _REF[key].values():
            a.setflags(write=False)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- device side
def _dev16(a, device):
    return torch.from_numpy(np.array(a, np.float32)).to(O.STORAGE).to(device)


def _x4(x, device):
    n, h, w, _ = x.shape
    x4 = np.zeros((n, h, w, 4), np.float32)
    x4[..., :3] = x
    return _dev16(x4, device)


INTS = ("n", "h", "w", "cout", "flags", "relu")
SIZES = ("ws_bytes",)
SIG = {
    "ocr_conv2d_first_f16": "n h w cout x4 wp bias flags y stats",
    "ocr_conv2d_stem_f16": "n h w cout x4 wp bias flags y stats",
    "ocr_conv2d_first_bn_relu_f16": "n h w cout x4 wp scale shift relu y",
    "ocr_conv2d_first_wgrad_f16": "n h w cout x4 dy dw ws ws_bytes",
    "ocr_conv2d_stem_wgrad_f16": "n h w cout x4 dy dw ws ws_bytes",
    "ocr_conv2d_first_wgrad_bn_f16": "n h w cout x4 dy bn_y wp_re shift A B C relu dw ws ws_bytes",
    "ocr_conv2d_stem_wgrad_bn_f16": "n h w cout x4 dy bn_y shift A B C relu dw ws ws_bytes",
    "ocr_conv2d_first_moments_keep_f16": "n h w cout x4 wp row mom ws ws_bytes",
    "ocr_conv2d_first_moments_f16": "n h w cout x4 wp row ws ws_bytes",
}


def _call(name, v, **over):
    """The status (not raised) of a C-ABI entry with its arguments taken by name from `v`, then `over`; a tensor is
    passed as its device pointer, None as NULL, an int in a pointer slot as that address."""
    from tensorflow_ocr_amd import _lib as L
    v = dict(v, **over)
    args = []
    for a in SIG[name].split():
        if a in INTS:
            args.append(ctypes.c_int(int(v[a])))
        elif a in SIZES:
            args.append(ctypes.c_size_t(int(v[a])))
        elif isinstance(v.get(a), int):
            args.append(ctypes.c_void_p(v[a]))
        else:
            args.append(L.ptr(v.get(a)))
    return int(L._fn(name, ctypes.c_int)(*args, L.stream_ptr()))


def _tiles(kind, n, h, w):
    from tensorflow_ocr_amd import _lib as L
    return L.call_int("ocr_conv2d_%s_num_mtiles" % kind, ctypes.c_int(n), ctypes.c_int(h), ctypes.c_int(w))


def _pack(kind, wt, device):
    """the packed operand of the forward, guarded; -> (guard, packed)"""
    from tensorflow_ocr_amd import _lib as L
    cout = wt.shape[-1]
    shape = (3, cout, 16) if kind == "first" else (7, 2, cout, 16)
    guard, wp = carve(shape, O.STORAGE, 1024, device)
    wd = torch.from_numpy(np.array(wt, np.float32)).to(device)
    rc = L._fn("ocr_pack_weights_%s_f16" % kind, ctypes.c_int)(L.ptr(wd), ctypes.c_int(cout), L.ptr(wp), L.stream_ptr())
    assert rc == OK
    return guard, wp


def _row_setup(kind, row, device):
    (n, h, w, cout), tiles = ROWS[kind][row]
    assert _tiles(kind, n, h, w) == tiles, "the tiling changed: row %s no longer reaches what its name says" % row
    if row == "cap":
        assert tiles == 1030 and tiles > 2 * WG_CAP and tiles > MOMENT_CAP
    ref = _operands(kind, row)
    oh, ow = _out(kind, h, w)
    _, wp = _pack(kind, ref["w"], device)
    v = dict(n=n, h=h, w=w, cout=cout, x4=_x4(ref["x"], device), wp=wp, flags=0, relu=0)
    return v, ref, (n, oh, ow, cout), tiles


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------- packers
def _packed_numpy(kind, wt):
    """The documented layouts restated: first [3][cout][16], k = kx*4 + c; stem [7][2][cout][16],
    k = (kx - 4*khalf)*4 + c; zero for kx past the filter or c = 3."""
    k = GEOM[kind][0]
    cout = wt.shape[-1]
    w16 = _h(wt)
    if kind == "first":
        out = np.zeros((3, cout, 16), np.float32)
        for ky in range(3):
            for kx in range(3):
                for c in range(3):
                    out[ky, :, kx * 4 + c] = w16[ky, kx, c]
        return out
    out = np.zeros((7, 2, cout, 16), np.float32)
    for ky in range(k):
        for kx in range(k):
            for c in range(3):
                out[ky, kx // 4, :, (kx % 4) * 4 + c] = w16[ky, kx, c]
    return out


@pytest.mark.parametrize("kind,cout", [("first", 64), ("first", 128), ("stem", 64), ("stem", 128)])
def test_packers_exact_layout(device, kind, cout):
    k = GEOM[kind][0]
    wt = _rng("pack", kind, cout).standard_normal((k, k, 3, cout)).astype(np.float32)
    guard, wp = _pack(kind, wt, device)
    torch.cuda.synchronize()
    want = torch.from_numpy(_packed_numpy(kind, wt)).to(O.STORAGE)
    assert written(wp) and bands_untouched(guard)
    assert torch.equal(wp.cpu().view(torch.int16), want.view(torch.int16))          # +0 in every zero slot as well


# ---------------------------------------------------------------------------------------------------- forward
def _check_forward(kind, v, x, wt, conv, oshape, tiles, device, tag):
    """Every flag mode of the forward entry on one shape; returns the largest error of y."""
    n, oh, ow, cout = oshape
    name = "ocr_conv2d_%s_f16" % kind
    rng = _rng("bias", tag)
    bias = rng.standard_normal(cout).astype(np.float32)
    bd = torch.from_numpy(bias).to(device)
    worst = 0.0
    for flags in FLAG_MODES:
        yg, y = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
        pg, part = carve((tiles, 2, cout), torch.float32, 2 * cout, device)
        assert _call(name, v, flags=flags, bias=bd if flags & BIAS else None, y=y,
                     stats=part if flags & STATS else None) == OK
        torch.cuda.synchronize()
        assert written(y), "%s flags %d: elements of y not written" % (tag, flags)
        assert bands_untouched(yg) and bands_untouched(pg), "%s flags %d: stores outside a buffer" % (tag, flags)
        pre = conv + bias.astype(np.float64) if flags & BIAS else conv
        ref = np.maximum(pre, 0.0) if flags & RELU else pre
        got = y.float().cpu().numpy().astype(np.float64)
        m = np.abs(ref).max()
        e = float(np.abs(got - ref).max() / m)
        worst = max(worst, e)
        assert e < Y_TOL, (tag, flags, e)
        if flags & RELU:
            assert (got >= 0).all() and (got[pre < -Y_TOL * m] == 0).all() and (got[pre > Y_TOL * m] > 0).all()
        if not flags & STATS:
            assert untouched(part)
            continue
        assert written(part), "%s flags %d: partial rows not written" % (tag, flags)
        sums = part.double().sum(0).cpu().numpy()
        assert np.allclose(sums[0], got.sum((0, 1, 2)), rtol=1e-4, atol=1e-2), (tag, flags)
        assert np.allclose(sums[1], (got * got).sum((0, 1, 2)), rtol=1e-4), (tag, flags)
        if kind == "first":                               # y = NULL: the same partial rows, bit for bit, nothing stored
            p2g, part2 = carve((tiles, 2, cout), torch.float32, 2 * cout, device)
            assert _call(name, v, flags=flags, bias=bd if flags & BIAS else None, y=None, stats=part2) == OK
            torch.cuda.synchronize()
            assert torch.equal(part2.view(torch.int32), part.view(torch.int32)) and bands_untouched(p2g)
    return worst


@pytest.mark.parametrize("kind,row", CASES)
def test_forward_vs_float64(device, kind, row):
    v, ref, oshape, tiles = _row_setup(kind, row, device)
    e = _check_forward(kind, v, ref["x"], ref["w"], ref["conv"], oshape, tiles, device, (kind, row))
    print("image conv %-5s %-8s forward: y %.2e" % (kind, row, e))


def test_first_forward_on_prepared_images(device):
    """ocr_prep_images_f16's own output ([n,h,w,4], channel 3 zero) through the same forward check."""
    from tensorflow_ocr_amd import _lib as L
    n, h, w, cout = 2, 20, 45, 64
    rng = _rng("prep")
    img = torch.from_numpy(rng.uniform(0, 255, (n, h, w, 3)).astype(np.float32)).to(device)
    xg, x4 = carve((n, h, w, 4), O.STORAGE, 1024, device)
    L.call("ocr_prep_images_f16", L.ptr(img), ctypes.c_int64(n * h * w), ctypes.c_float(123.68), ctypes.c_float(116.78),
           ctypes.c_float(103.94), L.ptr(x4), L.stream_ptr())
    torch.cuda.synchronize()
    assert written(x4) and bands_untouched(xg)
    xh = x4.float().cpu().numpy()
    assert (xh[..., 3] == 0).all()
    want = img.cpu().numpy().astype(np.float64) - np.array([123.68, 116.78, 103.94], np.float32).astype(np.float64)
    assert np.abs(xh[..., :3] - want).max() <= (0.5 if BF16 else 0.0625) + 1e-4   # half a 16-bit ulp in [128, 256) + the f32 subtraction's
    x = np.ascontiguousarray(xh[..., :3])
    wt = _h(rng.standard_normal((3, 3, 3, cout)) * np.sqrt(2.0 / 27) / 64.0)
    _, wp = _pack("first", wt, device)
    v = dict(n=n, h=h, w=w, cout=cout, x4=x4, wp=wp)
    tiles = _tiles("first", n, h, w)
    e = _check_forward("first", v, x, wt, _conv_float64("first", x, wt), (n, h, w, cout), tiles, device, "prepared")
    print("image conv first prepared forward: y %.2e" % e)


@pytest.mark.parametrize("row", list(ROWS["first"]))
def test_first_bn_relu_vs_float64_and_the_elementwise_pass(device, row):
    from tensorflow_ocr_amd import ops
    v, ref, oshape, tiles = _row_setup("first", row, device)
    cout = oshape[-1]
    rng = _rng("bnrelu", row)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout, p=[0.1, 0.9])).astype(np.float32)
    shift = rng.normal(0, 0.3, cout).astype(np.float32)
    assert (scale < 0).any()
    sd, hd = torch.from_numpy(scale).to(device), torch.from_numpy(shift).to(device)
    yg, y = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
    assert _call("ocr_conv2d_first_f16", v, y=y, bias=None, stats=None) == OK
    y16 = _h(ref["conv"]).astype(np.float64)               # the value the first pass stores, from the reference
    for relu in (1, 0):
        ag, a = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
        assert _call("ocr_conv2d_first_bn_relu_f16", v, scale=sd, shift=hd, relu=relu, y=a) == OK
        eg, a_el = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
        ops.bn_relu(y, sd, hd, bool(relu), 0, a_full=a_el)
        torch.cuda.synchronize()
        assert written(a) and bands_untouched(ag) and bands_untouched(yg) and bands_untouched(eg)
        want = y16 * scale.astype(np.float64) + shift.astype(np.float64)
        if relu:
            want = np.maximum(want, 0.0)
        e = _rel(a.float().cpu().numpy(), want)
        print("image conv first %-8s bn_relu relu=%d: a %.2e" % (row, relu, e))
        assert e < A_TOL, e
        assert torch.equal(a.view(torch.int16), a_el.view(torch.int16)), "not the values ocr_bn_relu_f16 gives on the stored y"


# ---------------------------------------------------------------------------------------------------- weight gradients
def _wgrad_buffers(kind, v, device):
    from tensorflow_ocr_amd import _lib as L
    k = GEOM[kind][0]
    elems = k * k * 3 * v["cout"]
    nbytes = L.call_size("ocr_conv2d_%s_wgrad_workspace" % kind, *(ctypes.c_int(v[a]) for a in ("n", "h", "w", "cout")))
    blocks = min(_tiles(kind, v["n"], v["h"], v["w"]), WG_CAP)
    # one partial row per workgroup and K half: the layout is restated because `every workspace element is written`
    # (_run_wgrad) holds only if the workspace is exactly the rows the kernel stores; a change of the partial layout
    # has to change this line with it
    assert nbytes == blocks * 2 * elems * 4
    wg, ws = carve((nbytes // 4,), torch.float32, elems, device)
    dg, dw = carve((k, k, 3, v["cout"]), torch.float32, elems, device)
    return wg, ws, dg, dw, nbytes


def _run_wgrad(name, kind, v, device, **operands):
    wg, ws, dg, dw, nbytes = _wgrad_buffers(kind, v, device)
    assert _call(name, v, dw=dw, ws=ws, ws_bytes=nbytes, **operands) == OK
    torch.cuda.synchronize()
    assert written(ws), "%s: workspace elements the kernel did not write" % name
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(dw).all())
    assert bands_untouched(wg) and bands_untouched(dg), "%s: written outside a buffer" % name
    return dw.cpu().numpy()


def _sequential_f32_error(kind, x, dy, ref):
    """CPU only: max error / max|ref| of a SEQUENTIAL float32 sum of the very terms of dw (pixel after pixel)."""
    worst = 0.0
    dy32 = dy.reshape(-1, 1, dy.shape[-1]).astype(np.float32)
    for ky, kx, xs in _taps(kind, x):
        terms = xs.reshape(-1, 3, 1).astype(np.float32) * dy32
        seq = np.cumsum(terms, axis=0, dtype=np.float32)[-1]
        worst = max(worst, float(np.abs(seq.astype(np.float64) - ref[ky, kx]).max()))
    return worst / float(np.abs(ref).max())


@pytest.mark.parametrize("kind,row", CASES)
def test_plain_wgrad_vs_float64(device, kind, row):
    v, ref, oshape, tiles = _row_setup(kind, row, device)
    if row == "cap":
        seq = _sequential_f32_error(kind, ref["x"], ref["dy"], ref["dw"])
        print("image conv %-5s cap: sequential f32 sum on the CPU %.2e" % (kind, seq))
        assert seq <= WGRAD_BAR, "the reference's own terms do not fit the bar in f32: %.2e" % seq
    got = _run_wgrad("ocr_conv2d_%s_wgrad_f16" % kind, kind, v, device, dy=_dev16(ref["dy"], device))
    e = _rel(got, ref["dw"])
    print("image conv %-5s %-8s plain wgrad: dw %.2e" % (kind, row, e))
    assert e <= WGRAD_BAR, e


def _fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, as the hardware's fma: a * b is exact in float64 (24 + 11 bits at most),
    s + e == a * b + c exactly (two-sum).  round32(s) differs from the single rounding only where s is exactly an
    f32 midpoint and e != 0 -> (result, number of such elements)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    nxt = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (d != 0) & (np.abs(d) * 2 == np.abs(nxt.astype(np.float64) - r.astype(np.float64)))
    return r, int((mid & (e != 0)).sum())


def _bn_operands(seed, y16, relu):
    """da and the per-channel A, B, C, shift drawn from `seed`; the restated dy16 and how far the draw is from the
    conditions: (mask arguments within an f32 ulp of the threshold, fma midpoints, dy within an ulp of a boundary)."""
    cout = y16.shape[-1]
    rng = np.random.default_rng(seed)
    da = _h(rng.standard_normal(y16.shape) * 0.25)
    A = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout, p=[0.1, 0.9])).astype(np.float32)
    B = rng.normal(0, 0.1, cout).astype(np.float32)
    C = rng.normal(0, 0.05, cout).astype(np.float32)
    shift = rng.normal(0, 0.3, cout).astype(np.float32)
    z = y16.astype(np.float64) * A.astype(np.float64) + shift.astype(np.float64)
    near_mask = int((np.abs(z - RELU_TIE) <= 2.0 ** -23 * np.maximum(np.abs(z), RELU_TIE)).sum()) if relu else 0
    dz = np.where(z > RELU_TIE, da, np.float32(0)) if relu else da
    inner, t1 = _fma32(np.broadcast_to(B, y16.shape), y16, np.broadcast_to(C, y16.shape))
    outer, t2 = _fma32(np.broadcast_to(A, y16.shape), dz, inner)
    dy16 = _h(outer)
    inf = np.float32(np.inf)
    near16 = int(((_h(np.nextafter(outer, inf)) != dy16) | (_h(np.nextafter(outer, -inf)) != dy16)).sum())
    return dict(da=da, A=A, B=B, C=C, shift=shift, dy16=dy16), (near_mask, t1 + t2, near16)


def _bn_case(kind, row, relu, y16):
    """The draw of the row: on rows of at most SEED_SEARCHED elements the first seed that meets all three conditions,
    on the larger ones (no seed can meet the third: see the module docstring) the first that meets the first two."""
    small = y16.size <= SEED_SEARCHED
    for trial in range(4000):
        ops_, (near_mask, mids, near16) = _bn_operands(_seed("bn", kind, row, relu, trial), y16, relu)
        if near_mask == 0 and mids == 0 and (near16 == 0 or not small):
            return ops_, trial, near16
    raise AssertionError("no seed satisfies the conditions on the inputs")


@pytest.mark.parametrize("kind,row", CASES)
def test_fused_wgrad_vs_float64(device, kind, row):
    v, ref, oshape, tiles = _row_setup(kind, row, device)
    cout = oshape[-1]
    yg, y = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
    assert _call("ocr_conv2d_%s_f16" % kind, v, y=y, bias=None, stats=None) == OK     # the y of the forward launch
    torch.cuda.synchronize()
    y16 = y.float().cpu().numpy()
    assert _rel(y16, ref["conv"]) < Y_TOL
    f32 = lambda a: torch.from_numpy(a).to(device)
    for relu in (1, 0):
        o, trial, near16 = _bn_case(kind, row, relu, y16)
        want = _dw_float64(kind, ref["x"], o["dy16"])
        args = dict(dy=_dev16(o["da"], device), shift=f32(o["shift"]), A=f32(o["A"]), B=f32(o["B"]), C=f32(o["C"]), relu=relu)
        name = "ocr_conv2d_%s_wgrad_bn_f16" % kind
        got = _run_wgrad(name, kind, v, device, bn_y=y, wp_re=None, **args)
        e = _rel(got, want)
        print("image conv %-5s %-8s fused wgrad relu=%d (seed %d, %d of %d dy within an ulp of a boundary): dw %.2e" % (
            kind, row, relu, trial, near16, y16.size, e))
        assert e <= WGRAD_BAR, e
        if kind == "first":
            re = _run_wgrad(name, kind, v, device, bn_y=None, wp_re=v["wp"], **args)
            assert np.array_equal(re.view(np.int32), got.view(np.int32)), "the recomputing form is not bit-identical"
    assert bands_untouched(yg)


# ---------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("row", MOMENT_ROWS)
def test_first_moments_vs_float64(device, row):
    from tensorflow_ocr_amd import _lib as L
    v, ref, oshape, tiles = _row_setup("first", row, device)
    n, h, w, cout = oshape
    nbytes = L.call_size("ocr_conv2d_first_moments_workspace")
    conv = ref["conv"]
    N = n * h * w
    s1, s2 = conv.sum((0, 1, 2)), (conv * conv).sum((0, 1, 2))
    mean, var = s1 / N, s2 / N - (s1 / N) ** 2
    V = np.concatenate([xs.reshape(N, 3) for _, _, xs in _taps("first", ref["x"])] + [np.ones((N, 1))], axis=1)
    M = np.zeros((32, 32))
    M[:28, :28] = V.T @ V
    absM = np.zeros((32, 32))
    absM[:28, :28] = np.abs(V).T @ np.abs(V)
    trips = -(-tiles // min(tiles, MOMENT_CAP))
    assert trips == (2 if row == "cap" else 1)
    bound = (64 * trips + 3) * 2.0 ** -24 * absM
    for keep in (True, False):
        wg, ws = carve((nbytes // 4,), torch.float32, 1024, device)
        rg, srow = carve((2, cout), torch.float32, 2 * cout, device)
        mg, mom = carve((32, 32), torch.float64, 1024, device)
        name = "ocr_conv2d_first_moments_keep_f16" if keep else "ocr_conv2d_first_moments_f16"
        assert _call(name, v, row=srow, mom=mom, ws=ws, ws_bytes=nbytes) == OK
        torch.cuda.synchronize()
        assert written(srow) and bands_untouched(wg) and bands_untouched(rg) and bands_untouched(mg)
        got = srow.double().cpu().numpy()
        gmean, gvar = got[0] / N, got[1] / N - (got[0] / N) ** 2
        e_m, e_v = float(np.abs(gmean - mean).max() / np.sqrt(var).max()), float(np.abs(gvar / var - 1).max())
        assert e_m <= 1e-5 and e_v <= 1e-5, (e_m, e_v)
        if not keep:
            assert untouched(mom)
            continue
        assert written(mom)
        gm = mom.cpu().numpy()
        err = np.abs(gm - M)
        print("image conv first %-8s moments: mean %.2e sd, variance %.2e, M %.3f of its bound" % (
            row, e_m, e_v, float((err[:28, :28] / bound[:28, :28]).max())))
        assert (err <= bound).all(), np.argwhere(err > bound)[:4].tolist()
        assert gm[27, 27] == N                                                     # the pixel count is exact


# ---------------------------------------------------------------------------------------------------- impulse rows
def _impulse_image(kind, n, h, w):
    """Fourteen single-channel small integers: the corners of the first image; in the last image the middle of the
    last row and of the last column and the four pixels around the corner where four output tiles meet."""
    s = GEOM[kind][1]
    by, bx = 8 * s, 32 * s                                 # the input pixel under the second tile row / column's origin
    assert h > by and w > bx
    pts = [(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1), (n - 1, h - 1, w // 2), (n - 1, h // 2, w - 1),
           (n - 1, by - 1, bx - 1), (n - 1, by - 1, bx), (n - 1, by, bx - 1), (n - 1, by, bx),
           # (interior pixels of every row / column parity: a stride of 2 shows each to half of the taps)
           (n - 1, by - 3, bx - 3), (n - 1, by - 3, bx - 2), (n - 1, by - 2, bx - 3), (n - 1, by - 2, bx - 2)]
    x = np.zeros((n, h, w, 3), np.float32)
    for j, (img, iy, ix) in enumerate(pts):
        x[img, iy, ix] = 0
        x[img, iy, ix, j % 3] = (1, 2, 3, -1, -2, -3)[j % 6]
    return x


def _dyadic(shape, *strides):
    """dense multiples of 1/64 below 2, a different one along every axis (251 is prime)"""
    idx = np.indices(shape)
    m = sum(i * s for i, s in zip(idx, strides)) % 251 - 125
    return (m / 64.0).astype(np.float32)


@pytest.mark.parametrize("kind,shape", IMPULSE)
def test_impulse_forward_exact(device, kind, shape):
    n, h, w, cout = shape
    k = GEOM[kind][0]
    x = _impulse_image(kind, n, h, w)
    wt = _dyadic((k, k, 3, cout), 37 * 3 * k, 37 * 3, 37, 11)                  # 37 * ((ky*k + kx)*3 + c) + 11 * co
    assert np.array_equal(_h(wt), wt) and np.array_equal(_h(x), x)
    ref = _conv_float64(kind, x, wt)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)       # exact in f32, hence in any order
    oshape = ref.shape
    _, wp = _pack(kind, wt, device)
    yg, y = carve(oshape, O.STORAGE, 8 * 32 * cout, device)
    v = dict(n=n, h=h, w=w, cout=cout, x4=_x4(x, device), wp=wp, flags=0, bias=None, stats=None, y=y)
    assert _call("ocr_conv2d_%s_f16" % kind, v) == OK
    torch.cuda.synchronize()
    assert written(y) and bands_untouched(yg)
    bad = np.argwhere(y.float().cpu().numpy() != _h(ref))
    assert bad.size == 0, "%d elements differ, first (n, oy, ox, co) = %s" % (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("kind,shape", IMPULSE)
def test_impulse_wgrad_exact(device, kind, shape):
    n, h, w, cout = shape
    x = _impulse_image(kind, n, h, w)
    oh, ow = _out(kind, h, w)
    dy = _dyadic((n, oh, ow, cout), 5, 13, 7, 3)
    assert np.array_equal(_h(dy), dy)
    ref = _dw_float64(kind, x, dy)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)
    assert np.abs(ref).max(axis=(2, 3)).min() > 0                               # every tap carries something
    v = dict(n=n, h=h, w=w, cout=cout, x4=_x4(x, device))
    got = _run_wgrad("ocr_conv2d_%s_wgrad_f16" % kind, kind, v, device, dy=_dev16(dy, device))
    bad = np.argwhere(got != ref32)
    assert bad.size == 0, "%d elements differ, first (ky, kx, c, co) = %s" % (len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------------------------------- status codes
def test_status_codes_and_nothing_launched(device):
    """Every entry of both files: a null operand or a non-positive extent is INVALID_ARG, cout = 96 UNSUPPORTED, a
    workspace one byte short (or a misaligned one) WORKSPACE, BIAS / STATS without their pointers INVALID_ARG, a
    misaligned moments_f64 INVALID_ARG — and every NaN-filled output is still NaN afterwards: nothing was launched."""
    from tensorflow_ocr_amd import _lib as L
    outputs, guards = [], []

    def filled(shape, dtype, band=256):
        g, t = carve(shape, dtype, band, device)
        outputs.append(t)
        guards.append(g)
        return t
    mbytes = L.call_size("ocr_conv2d_first_moments_workspace")
    for kind, (n, h, w, cout) in (("first", (1, 9, 33, 64)), ("stem", (1, 17, 65, 64))):
        k = GEOM[kind][0]
        oshape = (n,) + _out(kind, h, w) + (cout,)
        tiles = _tiles(kind, n, h, w)
        z16 = lambda s: torch.zeros(s, dtype=O.STORAGE, device=device)
        z32 = lambda s: torch.zeros(s, dtype=torch.float32, device=device)
        nbytes = L.call_size("ocr_conv2d_%s_wgrad_workspace" % kind, *(ctypes.c_int(a) for a in (n, h, w, cout)))
        base = dict(n=n, h=h, w=w, cout=cout, x4=z16((n, h, w, 4)), wp=z16((3, cout, 16) if kind == "first" else (7, 2, cout, 16)),
                    bias=z32(cout), flags=BIAS | STATS, relu=1, scale=z32(cout), shift=z32(cout), A=z32(cout), B=z32(cout),
                    C=z32(cout), dy=z16(oshape), bn_y=z16(oshape), y=filled(oshape, O.STORAGE),
                    stats=filled((tiles, 2, cout), torch.float32), dw=filled((k, k, 3, cout), torch.float32))
        base["wp_re"] = None
        wgrad = dict(base, ws=filled((nbytes // 4,), torch.float32), ws_bytes=nbytes)
        entries = [("ocr_conv2d_%s_f16" % kind, base, ("x4", "wp", "bias", "stats")),
                   ("ocr_conv2d_%s_wgrad_f16" % kind, wgrad, ("x4", "dy", "dw", "ws")),
                   ("ocr_conv2d_%s_wgrad_bn_f16" % kind, wgrad, ("x4", "dy", "bn_y", "shift", "A", "B", "C", "dw", "ws"))]
        if kind == "first":
            moments = dict(base, row=filled((2, cout), torch.float32), mom=filled((32, 32), torch.float64),
                           ws=filled((mbytes // 4,), torch.float32), ws_bytes=mbytes)
            entries += [("ocr_conv2d_first_bn_relu_f16", base, ("x4", "wp", "scale", "shift", "y")),
                        ("ocr_conv2d_first_moments_keep_f16", moments, ("x4", "wp", "row", "ws")),
                        ("ocr_conv2d_first_moments_f16", moments, ("x4", "wp", "row", "ws"))]
        for name, v, pointers in entries:
            for extent in ("n", "h", "w", "cout"):
                for bad in (0, -1):
                    assert _call(name, v, **{extent: bad}) == INVALID_ARG, (name, extent, bad)
            assert _call(name, v, cout=96) == UNSUPPORTED, name
            for p in pointers:
                assert _call(name, v, **{p: None}) == INVALID_ARG, (name, p)
            if "ws_bytes" in v:
                assert _call(name, v, ws_bytes=v["ws_bytes"] - 1) == WORKSPACE, name
        fwd = "ocr_conv2d_%s_f16" % kind
        assert _call(fwd, base, flags=0, y=None) == INVALID_ARG                  # nothing to store, nothing to sum
        if kind == "stem":
            assert _call(fwd, base, flags=STATS, y=None) == INVALID_ARG          # no statistics-only form
        else:
            assert _call("ocr_conv2d_first_wgrad_bn_f16", wgrad, bn_y=None, wp_re=None) == INVALID_ARG   # neither y nor w_first
            odd = moments["mom"].data_ptr() + 4
            assert _call("ocr_conv2d_first_moments_keep_f16", moments, mom=odd) == INVALID_ARG
            odd = moments["ws"].data_ptr() + 4
            for name in ("ocr_conv2d_first_moments_keep_f16", "ocr_conv2d_first_moments_f16"):
                assert _call(name, moments, ws=odd, ws_bytes=mbytes) == WORKSPACE
    torch.cuda.synchronize()
    assert all(untouched(t) for t in outputs), "an error return launched something"
    assert all(bands_untouched(g) for g in guards)
