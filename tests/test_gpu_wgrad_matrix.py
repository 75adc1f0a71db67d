"""GPU: every weight-gradient kernel family and every edge of its split-K plan (csrc/conv_wgrad.hip, conv_wgrad_pw.hip)
through the public C ABI, each against a float64 restatement on the same 16-bit-exact operands (numpy on the CPU, one
einsum per tap over explicitly padded input; no autograd, no device route compared with another except where
bit-identity is the contract).

What runs is asserted through ocr_conv2d_wgrad_variant (the selection the launch itself reads), so a change of
wgrad_select / fill2 / pw_plan cannot move the matrix onto one family unnoticed.  Instantiations wgrad_slabs and
wgrad_pw_launch can launch, and the rows that reach them:

  wgrad_pw_kernel<256,256,2> <256,128,4> <256,64,4> <128,256,2> <128,128,2> <128,64,4> <64,256,1> <64,128,1> <64,64,2>
                            pw_<cin>_<cout> (1x1 on 2 x 9 x 37: last pixel tile partial), pw_dil6 (nine taps, halo wider
                            than the map), pw_s2 (1x1 stride 2), pw_dil2_s2, pw_xcd_on / pw_short_split (several blocks;
                            grid a multiple of 8 or not; last split one tile short), pw_69_slabs
  wgrad3_kernel<9,128>      t3_128_ragged, t3_128_blocks (XCD order on), t3_128_short_split (9 tiles in splits of 2)
  wgrad3_kernel<9,64>       t3_64_three_co, t3_64_tiny (fewer tiles than wanted splits), t3_64_co160 (ragged third block)
  wgrad2_kernel<128,9>      t2_128_9 (partial ci block)
  wgrad2_kernel<64,9>       t2_64_9 (partial ci and co blocks, slabs doubled in the workgroup), t2_64_2x2 (4 of 9 taps)
  wgrad2_kernel<128,1>      t2_128_1
  wgrad2_kernel<64,1>       t2_64_1
  wgrad_kernel<9>           gen_5x1, gen_4x2 — see below
  wgrad_kernel<1>           UNREACHED: a 1x1 filter misses fill2 only at stride >= 2 (halo 7 x 63 > 7 x 32 pixels), and
                            there fill()'s own halo (15 x 63 pixels x 144 B + the dy tile) exceeds 160 KiB of LDS, so no
                            1x1 shape of any size reaches it; 1x1 shapes run the pointwise GEMM, wgrad2<*,1>, or nothing.
  slab_reduce_kernel<1|4|16|64>  rows of every width, and SLAB_SUM below on its own.

Findings about the selection (neither halo depends on the map size, so they hold for every map):
  * 3x3 at stride 2, dilation 1 — (2, 18, 36, 64, 128, 3, 1, 2) — reaches NO family: fill2 refuses the 9 x 65 halo and
    fill() the 17 x 65 one (196 KB of LDS); the launch answers OCR_ERR_UNSUPPORTED (asserted: UNSUPPORTED_SHAPES).  The
    nets never ask for it (layers._conv_dgrad refuses strided input gradients as well).
  * With square filters the generic wgrad_kernel<9> is reached only by dilated filters on tensors of >= 2^30 elements
    (out of scope); below that the pointwise GEMM takes every dilated shape fill() accepts.  The rows here reach it with
    the smallest non-square filters whose 4-row halo exceeds fill2's 7 x 32 pixels: 5 x 1 (8 x 32) and 4 x 2 (7 x 33).
    No net of the project uses such filters.
  * Neither generic row has a stride: fill()'s 8-row halo is at least 15 x 63 pixels at stride 2 (172 KB with the dy tile,
    over the 160 KiB of LDS), so wgrad_kernel runs at stride 1 only and its stride arithmetic (a_lane, a_half, the halo
    origin) is NOT covered here — no shape can reach it.  The same holds for wgrad2 / wgrad3 (fill2's 7 x 32-pixel limit);
    stride 2 runs on the pointwise GEMM only (pw_s2, pw_dil2_s2).
  * The 3x3 cin % 64 == 0 shapes on wgrad2 (OCR_WGRAD3=0) are run by
    test_gpu_switches.py::test_kernel_family_selectors_in_a_child_interpreter; nothing here sets that variable.

Bar: max|dw - ref| <= 5e-6 max|ref| in both builds (test_conv_fwd_dgrad_wgrad's: operands and products are exact in
f32, only the accumulation order differs).  Measured, largest per family over the one- and two-call forms
(f16 / bf16 library); every row lies between 6.5e-8 and 1.9e-7:
  wgrad_pw_kernel (all tiles)  1.35e-07 / 1.22e-07        wgrad2_kernel<128,9>  1.24e-07 / 9.28e-08
  wgrad3_kernel<9,128>         1.84e-07 / 1.50e-07        wgrad2_kernel<64,9>   1.12e-07 / 1.02e-07
  wgrad3_kernel<9,64>          1.40e-07 / 1.17e-07        wgrad2_kernel<128,1>  1.48e-07 / 7.48e-08
  wgrad_kernel<9>              1.39e-07 / 1.16e-07        wgrad2_kernel<64,1>   7.99e-08 / 6.52e-08
The slab sum alone stays within 0.6 of its derived bound (5 slabs on one lane) and far below it on 16 / 64 lanes.
Impulse rows must match bit for bit (every product and partial sum is a small dyadic rational, exact in f32 in any
order): they pin the tap order, the pad offsets, the stride and the channel-block mapping, which the random rows can
only bound.

Every row gets a workspace of exactly ocr_conv2d_wgrad_workspace bytes and a dw, both NaN-filled and carved out of
larger allocations with sentinel bands of one slab's worth of bytes on each side: the product hands the slab kernel
an uninitialised buffer, and the slab sum adds every slab unconditionally."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from matrix_support import INVALID_ARG, OK, UNSUPPORTED, WORKSPACE, _h, _raw, bands_untouched, carve, untouched
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

# name: (expected slab kernel, (n, h, w, cin, cout, k | (kh, kw), dilation, stride)); SAME padding from ops.conv_desc
ROWS = {
    # pointwise GEMM, one row per instantiation: 666 pixels = 20 stages of 2 x 32, every second one 5 columns wide
    "pw_256_256": ("wgrad_pw_kernel<256,256,2>", (2, 9, 37, 256, 256, 1, 1, 1)),
    "pw_256_128": ("wgrad_pw_kernel<256,128,4>", (2, 9, 37, 256, 128, 1, 1, 1)),
    "pw_256_64": ("wgrad_pw_kernel<256,64,4>", (2, 9, 37, 256, 64, 1, 1, 1)),
    "pw_128_256": ("wgrad_pw_kernel<128,256,2>", (2, 9, 37, 128, 256, 1, 1, 1)),
    "pw_128_128": ("wgrad_pw_kernel<128,128,2>", (2, 9, 37, 128, 128, 1, 1, 1)),
    "pw_128_64": ("wgrad_pw_kernel<128,64,4>", (2, 9, 37, 128, 64, 1, 1, 1)),
    "pw_64_256": ("wgrad_pw_kernel<64,256,1>", (2, 9, 37, 64, 256, 1, 1, 1)),
    "pw_64_128": ("wgrad_pw_kernel<64,128,1>", (2, 9, 37, 64, 128, 1, 1, 1)),
    "pw_64_64": ("wgrad_pw_kernel<64,64,2>", (2, 9, 37, 64, 64, 1, 1, 1)),
    "pw_dil6": ("wgrad_pw_kernel<128,256,2>", (2, 12, 20, 128, 256, 3, 6, 1)),       # 9 taps x 12 splits = 108 workgroups
    "pw_s2": ("wgrad_pw_kernel<128,128,2>", (2, 17, 35, 128, 128, 1, 1, 2)),
    "pw_dil2_s2": ("wgrad_pw_kernel<64,64,2>", (2, 9, 11, 64, 64, 3, 2, 2)),         # strided AND dilated: pads 2, 5 x 6 output
    "pw_xcd_on": ("wgrad_pw_kernel<256,256,2>", (2, 9, 37, 256, 512, 1, 1, 1)),      # 2 blocks x 20 splits
    "pw_short_split": ("wgrad_pw_kernel<256,256,2>", (3, 46, 20, 512, 512, 1, 1, 1)),  # 4 blocks; 69 stages in 35 splits of 2
    "pw_69_slabs": ("wgrad_pw_kernel<64,64,2>", (3, 46, 20, 64, 64, 1, 1, 1)),       # 69 slabs on 64 sum lanes
    "t3_128_ragged": ("wgrad3_kernel<9,128>", (2, 9, 37, 64, 128, 3, 1, 1)),         # 4 x 32-pixel tiles: ragged rows and columns
    "t3_128_blocks": ("wgrad3_kernel<9,128>", (1, 16, 64, 256, 256, 3, 1, 1)),       # 4 ci x 2 co blocks
    "t3_128_short_split": ("wgrad3_kernel<9,128>", (1, 34, 20, 512, 512, 3, 1, 1)),  # 9 tiles, 8 wanted: 5 splits, the last of 1
    "t3_64_three_co": ("wgrad3_kernel<9,64>", (2, 13, 40, 128, 192, 3, 1, 1)),
    "t3_64_tiny": ("wgrad3_kernel<9,64>", (3, 7, 5, 64, 64, 3, 1, 1)),               # map < one tile; 6 tiles, 256 splits wanted
    "t3_64_co160": ("wgrad3_kernel<9,64>", (1, 17, 19, 64, 160, 3, 1, 1)),           # third cout block half full
    "t2_128_9": ("wgrad2_kernel<128,9>", (1, 17, 19, 96, 128, 3, 1, 1)),
    "t2_64_9": ("wgrad2_kernel<64,9>", (1, 17, 19, 96, 160, 3, 1, 1)),
    "t2_64_2x2": ("wgrad2_kernel<64,9>", (1, 9, 11, 64, 64, 2, 1, 1)),               # SAME padding 0 before, 1 after
    "t2_128_1": ("wgrad2_kernel<128,1>", (1, 8, 16, 96, 128, 1, 1, 1)),
    "t2_64_1": ("wgrad2_kernel<64,1>", (2, 9, 11, 96, 64, 1, 1, 1)),
    "gen_5x1": ("wgrad_kernel<9>", (2, 9, 37, 64, 128, (5, 1), 1, 1)),
    "gen_4x2": ("wgrad_kernel<9>", (1, 10, 33, 128, 64, (4, 2), 1, 1)),
}
# what the plan must show for the row to test what its name says (read from the variant string)
PLAN = {
    "pw_xcd_on": lambda v: v["xcd"] == 1 and v["grid"] % 8 == 0 and v["grid"] > v["slabs"],
    "pw_short_split": lambda v: v["xcd"] == 0 and v["grid"] % 8 != 0 and v["grid"] > v["slabs"] and v["slabs"] == 35,
    "pw_dil6": lambda v: v["grid"] == 9 * v["slabs"],
    "pw_69_slabs": lambda v: v["slabs"] == 69 and v["reduce"] == "slab_reduce_kernel<64>",
    "t3_128_blocks": lambda v: v["xcd"] == 1 and v["grid"] == 8 * v["slabs"],
    "t3_128_short_split": lambda v: v["slabs"] == 5 and v["xcd"] == 1 and v["reduce"] == "slab_reduce_kernel<1>",
    "t3_64_tiny": lambda v: v["slabs"] == 6 and v["xcd"] == 0,
    "t2_64_9": lambda v: v["slabs"] == 2 * v["grid"] // 6,        # 2 ci x 3 co blocks; two slabs per split
    "t2_128_1": lambda v: v["reduce"] == "slab_reduce_kernel<1>",
    "gen_5x1": lambda v: v["slabs"] == 16 and v["grid"] == 16,    # 8 splits x 2 co blocks; two slabs per split
}
UNSUPPORTED_SHAPES = {
    "cin48": (2, 9, 11, 48, 64, 3, 1, 1),
    "k5x5": (2, 9, 11, 64, 64, 5, 1, 1),
    "k3_stride2": (2, 18, 36, 64, 128, 3, 1, 2),      # see the module docstring
    "k1_stride2_cin96": (2, 17, 35, 96, 128, 1, 1, 2),
}
# the slab sum on its own — name: (slabs, sum kernel, descriptor).  1x1 64 -> 64 descriptors write one slab per
# 2 x 32-pixel stage; the last two have a [2048][1024] filter, wide enough for one lane per output.  Each lane keeps
# four slabs in flight: the counts end in the first, a middle and the LAST of the four (15 on 4 lanes, 63 on 16, 8 and
# 256 on 1 and 64), and leave lanes without a slab in a round (6 on 4, 21 on 16, 69 on 64).
SLAB_SUM = {
    "one": (1, "slab_reduce_kernel<1>", (1, 2, 8, 64, 64, 1, 1, 1)),
    "three": (3, "slab_reduce_kernel<1>", (1, 6, 8, 64, 64, 1, 1, 1)),
    "six_on_4": (6, "slab_reduce_kernel<4>", (1, 12, 8, 64, 64, 1, 1, 1)),
    "15_on_4": (15, "slab_reduce_kernel<4>", (1, 30, 8, 64, 64, 1, 1, 1)),
    "21_on_16": (21, "slab_reduce_kernel<16>", (1, 42, 8, 64, 64, 1, 1, 1)),
    "63_on_16": (63, "slab_reduce_kernel<16>", (3, 42, 8, 64, 64, 1, 1, 1)),
    "69_on_64": (69, "slab_reduce_kernel<64>", (3, 46, 20, 64, 64, 1, 1, 1)),
    "256_on_64": (256, "slab_reduce_kernel<64>", (4, 64, 64, 64, 64, 1, 1, 1)),
    "five_on_1": (5, "slab_reduce_kernel<1>", (1, 10, 8, 2048, 1024, 1, 1, 1)),
    "eight_on_1": (8, "slab_reduce_kernel<1>", (1, 16, 8, 2048, 1024, 1, 1, 1)),
}

BAR = 5e-6

_REF = {}                       # (row, kind) -> (x, dy, float64 dw), computed once


def _desc(ops, shape):
    n, h, w, cin, cout, k, dil, stride = shape
    kh, kw = k if isinstance(k, tuple) else (k, k)
    d = ops.conv_desc((n, h, w, cin), cout, kh, kw, stride, dil)
    d.flags = 0
    return d


def _dw_float64(x, dy, d):
    """dw[ky,kx,ci,co] = sum x[n, oy*s + ky*dil - pt, ox*s + kx*dil - pl, ci] * dy[n,oy,ox,co] in float64: the input
    is padded with zeros explicitly (pt / pl before, enough after), one einsum per tap."""
    s, dil = d.stride, d.dilation
    eh, ew = (d.oh - 1) * s + (d.kh - 1) * dil + 1, (d.ow - 1) * s + (d.kw - 1) * dil + 1
    xp = np.zeros((d.n, max(eh, d.pad_top + d.h), max(ew, d.pad_left + d.w), d.cin), np.float64)
    xp[:, d.pad_top:d.pad_top + d.h, d.pad_left:d.pad_left + d.w] = x
    dy64 = dy.astype(np.float64)
    dw = np.empty((d.kh, d.kw, d.cin, d.cout), np.float64)
    for ky in range(d.kh):
        for kx in range(d.kw):
            xs = np.ascontiguousarray(xp[:, ky * dil:ky * dil + (d.oh - 1) * s + 1:s, kx * dil:kx * dil + (d.ow - 1) * s + 1:s])
            dw[ky, kx] = np.einsum("nyxi,nyxo->io", xs, dy64, optimize=True)
    return dw


def _impulse_operands(d):
    """x: zero except a few pixels — the four corners of the first image, an interior pixel of the last (one the stride
    lands on) and, under a stride, that pixel's diagonal neighbour, which the stride may skip — each with a different
    value k / 4, |k| <= 15, in every channel.  dy: zero except, for
    each of those pixels and each tap, the one output pixel that sees the pixel through that tap (where the padding
    and the stride leave one), with values k / 8, |k| <= 15, in every channel.  Every dw element is then a sum of at
    most six multiples of 1 / 32 below 8: exact in f32 in any order."""
    x = np.zeros((d.n, d.h, d.w, d.cin), np.float32)
    dy = np.zeros((d.n, d.oh, d.ow, d.cout), np.float32)
    ci, co = np.arange(d.cin), np.arange(d.cout)
    seen = set()
    my, mx = d.h // 2, d.w // 2
    my, mx = my - (my + d.pad_top) % d.stride, mx - (mx + d.pad_left) % d.stride
    pixels = [(0, 0, 0), (0, 0, d.w - 1), (0, d.h - 1, 0), (0, d.h - 1, d.w - 1), (d.n - 1, my, mx)]
    if d.stride > 1:
        pixels.append((d.n - 1, my + 1, mx + 1))
    for j, (img, iy, ix) in enumerate(pixels):
        x[img, iy, ix] = (((ci * 7 + j * 11) % 31) - 15) / 4.0
        for ky in range(d.kh):
            for kx in range(d.kw):
                ny, nx = iy - ky * d.dilation + d.pad_top, ix - kx * d.dilation + d.pad_left
                if ny % d.stride or nx % d.stride:
                    continue
                oy, ox = ny // d.stride, nx // d.stride
                if 0 <= oy < d.oh and 0 <= ox < d.ow:
                    dy[img, oy, ox] = (((co * 5 + (ky * d.kw + kx) * 3 + j) % 31) - 15) / 8.0
                    seen.add((ky, kx))
    assert len(seen) == d.kh * d.kw, "an impulse row must reach every tap"
    return x, dy


def _operands(ops, row, kind):
    key = (row, kind)
    if key not in _REF:
        shape = ROWS[row][1]
        d = _desc(ops, shape)
        if kind == "random":
            rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
            x = _h(rng.standard_normal((d.n, d.h, d.w, d.cin)))
            dy = _h(rng.standard_normal((d.n, d.oh, d.ow, d.cout)) * 0.25)
        else:
            x, dy = _impulse_operands(d)
            assert np.array_equal(_h(x), x) and np.array_equal(_h(dy), dy)
        _REF[key] = (x, dy, _dw_float64(x, dy, d))
    return _REF[key]


def _buffers(L, d, device, slabs=None):
    """(workspace guard, workspace, dw guard, dw): the workspace is exactly ocr_conv2d_wgrad_workspace bytes (or
    `slabs` slabs where that is 0), the bands one slab's worth."""
    elems = d.kh * d.kw * d.cin * d.cout
    band = (elems + 3) // 4 * 4
    nbytes = L.call_size("ocr_conv2d_wgrad_workspace", ctypes.byref(d))
    if slabs is None:
        assert nbytes > 0 and nbytes % (4 * elems) == 0
        slabs = nbytes // (4 * elems)
    wg, ws = carve((slabs * elems,), torch.float32, band, device)
    dg, dw = carve((elems,), torch.float32, band, device)
    return wg, ws, dg, dw


def _launch(L, form, d, xd, dyd, ws, dw):
    st = L.stream_ptr()
    nbytes = ctypes.c_size_t(ws.numel() * 4)
    if form == "one":
        return _raw(L, "ocr_conv2d_wgrad_f16", ctypes.byref(d), L.ptr(xd), L.ptr(dyd), L.ptr(dw), L.ptr(ws), nbytes, st)
    rc = _raw(L, "ocr_conv2d_wgrad_slabs_f16", ctypes.byref(d), L.ptr(xd), L.ptr(dyd), L.ptr(ws), nbytes, st)
    if rc != OK:
        return rc
    return _raw(L, "ocr_conv2d_wgrad_reduce_f32", ctypes.byref(d), L.ptr(ws), L.ptr(dw), st)


def _run(ops, L, device, row, kind, form):
    """One weight gradient of the row in guarded NaN-filled buffers -> (dw as numpy, float64 reference); asserts the
    kernel, the slab count, that every slab element and every dw element was written and nothing else."""
    kernel, shape = ROWS[row]
    d = _desc(ops, shape)
    v = ops.conv2d_wgrad_variant(d)
    assert v["kernel"] == kernel, v
    assert PLAN.get(row, lambda v: True)(v), v
    x, dy, ref = _operands(ops, row, kind)
    xd = torch.from_numpy(x).to(O.STORAGE).to(device)       # (copies: the shared operands stay as they were drawn)
    dyd = torch.from_numpy(dy).to(O.STORAGE).to(device)
    wg, ws, dg, dw = _buffers(L, d, device)
    assert ws.numel() == v["slabs"] * dw.numel(), (v, ws.numel(), dw.numel())
    assert _launch(L, form, d, xd, dyd, ws, dw) == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ws).any()), "%s: slab elements the kernel did not write" % row
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(dw).all())
    assert bands_untouched(wg), "%s: written outside the workspace" % row
    assert bands_untouched(dg), "%s: written outside dw" % row
    return dw.cpu().numpy().reshape(ref.shape), ref, v


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("row", list(ROWS))
def test_wgrad_vs_float64(device, row):
    """The one-call form, and the two calls the recorded step issues (slabs, then the sum): each inside the float64
    bar, and bit-identical to each other."""
    from tensorflow_ocr_amd import _lib as L, ops
    one, ref, v = _run(ops, L, device, row, "random", "one")
    two, _, _ = _run(ops, L, device, row, "random", "two")
    e1, e2 = _rel(one, ref), _rel(two, ref)
    print("wgrad %-18s %s slabs %d grid %d xcd %d %s: one-call %.2e two-call %.2e" % (
        row, v["kernel"], v["slabs"], v["grid"], v["xcd"], v["reduce"], e1, e2))
    assert e1 <= BAR and e2 <= BAR
    assert np.array_equal(one.view(np.int32), two.view(np.int32))


@pytest.mark.parametrize("row", list(ROWS))
def test_wgrad_impulse_exact(device, row):
    from tensorflow_ocr_amd import _lib as L, ops
    got, ref, _ = _run(ops, L, device, row, "impulse", "one")
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)                  # the reference itself is exact in f32
    assert np.abs(ref).reshape(-1, ref.shape[2], ref.shape[3]).max(axis=(1, 2)).min() > 0   # every tap carries something
    bad = np.argwhere(got != ref32)
    assert bad.size == 0, "%s: %d elements differ, first (ky, kx, ci, co) = %s" % (row, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("name", list(UNSUPPORTED_SHAPES))
def test_unsupported_shapes_write_nothing(device, name):
    from tensorflow_ocr_amd import _lib as L, ops
    d = _desc(ops, UNSUPPORTED_SHAPES[name])
    assert L.call_size("ocr_conv2d_wgrad_workspace", ctypes.byref(d)) == 0
    buf = ctypes.create_string_buffer(128)
    assert _raw(L, "ocr_conv2d_wgrad_variant", ctypes.byref(d), buf, ctypes.c_size_t(128)) == UNSUPPORTED
    xd = torch.zeros((d.n, d.h, d.w, d.cin), dtype=O.STORAGE, device=device)
    dyd = torch.zeros((d.n, d.oh, d.ow, d.cout), dtype=O.STORAGE, device=device)
    wg, ws, dg, dw = _buffers(L, d, device, slabs=2)
    for form in ("one", "two"):
        assert _launch(L, form, d, xd, dyd, ws, dw) == UNSUPPORTED
    assert _raw(L, "ocr_conv2d_wgrad_reduce_f32", ctypes.byref(d), L.ptr(ws), L.ptr(dw), L.stream_ptr()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched(ws) and untouched(dw) and bands_untouched(wg) and bands_untouched(dg)


@pytest.mark.parametrize("name", list(SLAB_SUM))
def test_slab_sum_alone(device, name):
    """ocr_conv2d_wgrad_reduce_f32 on random f32 slabs written by the host, against their float64 sum:
    |got - ref| <= slabs * 2^-24 * sum|slab| element-wise (f32 addition of `slabs` terms in any order: at most
    slabs - 1 roundings, each of at most 2^-24 of a partial sum that sum|slab| bounds) — derived, not measured."""
    from tensorflow_ocr_amd import _lib as L, ops
    slabs, reduce, shape = SLAB_SUM[name]
    d = _desc(ops, shape)
    v = ops.conv2d_wgrad_variant(d)
    assert (v["slabs"], v["reduce"]) == (slabs, reduce), v
    elems = d.kh * d.kw * d.cin * d.cout
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    host = rng.standard_normal((slabs, elems), dtype=np.float32)
    wg, ws, dg, dw = _buffers(L, d, device)
    assert ws.numel() == slabs * elems
    ws.copy_(torch.from_numpy(host).reshape(-1))
    assert _raw(L, "ocr_conv2d_wgrad_reduce_f32", ctypes.byref(d), L.ptr(ws), L.ptr(dw), L.stream_ptr()) == OK
    torch.cuda.synchronize()
    got = dw.cpu().numpy().astype(np.float64)
    ref = host.sum(axis=0, dtype=np.float64)
    bound = slabs * 2.0 ** -24 * np.abs(host).sum(axis=0, dtype=np.float64)
    excess = np.abs(got - ref) - bound
    print("slab sum %-10s %3d slabs %s: max |err| / bound %.3f" % (name, slabs, reduce, float((np.abs(got - ref) / bound).max())))
    assert np.isfinite(got).all() and excess.max() <= 0
    assert bands_untouched(dg) and bands_untouched(wg)
    assert np.array_equal(ws.cpu().numpy().reshape(slabs, elems), host)           # the slabs are only read


def test_return_codes_and_nothing_written(device):
    from tensorflow_ocr_amd import _lib as L, ops
    shape = ROWS["t3_64_tiny"][1]
    d = _desc(ops, shape)
    xd = torch.zeros((d.n, d.h, d.w, d.cin), dtype=O.STORAGE, device=device)
    dyd = torch.zeros((d.n, d.oh, d.ow, d.cout), dtype=O.STORAGE, device=device)
    wg, ws, dg, dw = _buffers(L, d, device)
    st = L.stream_ptr()
    nbytes = ws.numel() * 4
    ref, px, pdy, pws, pdw = ctypes.byref(d), L.ptr(xd), L.ptr(dyd), L.ptr(ws), L.ptr(dw)
    null = ctypes.c_void_p(0)
    name = ctypes.create_string_buffer(128)
    # a workspace one byte short
    assert _raw(L, "ocr_conv2d_wgrad_f16", ref, px, pdy, pdw, pws, ctypes.c_size_t(nbytes - 1), st) == WORKSPACE
    assert _raw(L, "ocr_conv2d_wgrad_slabs_f16", ref, px, pdy, pws, ctypes.c_size_t(nbytes - 1), st) == WORKSPACE
    # null pointers
    assert _raw(L, "ocr_conv2d_wgrad_f16", ref, px, pdy, null, pws, ctypes.c_size_t(nbytes), st) == INVALID_ARG
    assert _raw(L, "ocr_conv2d_wgrad_f16", ref, px, pdy, pdw, null, ctypes.c_size_t(nbytes), st) == INVALID_ARG
    assert _raw(L, "ocr_conv2d_wgrad_f16", ref, null, pdy, pdw, pws, ctypes.c_size_t(nbytes), st) == INVALID_ARG
    assert _raw(L, "ocr_conv2d_wgrad_reduce_f32", ref, pws, null, st) == INVALID_ARG
    assert _raw(L, "ocr_conv2d_wgrad_variant", ref, None, ctypes.c_size_t(128)) == INVALID_ARG
    assert _raw(L, "ocr_conv2d_wgrad_variant", ref, name, ctypes.c_size_t(8)) == INVALID_ARG     # too small for the answer
    assert _raw(L, "ocr_conv2d_wgrad_variant", ref, name, ctypes.c_size_t(128)) == OK
    # malformed descriptors: a supported-looking shape with one extent zeroed is INVALID_ARG, not UNSUPPORTED
    for field in ("n", "oh", "cin", "kh", "stride", "dilation"):
        bad = _desc(ops, shape)
        setattr(bad, field, 0)
        b = ctypes.byref(bad)
        assert _raw(L, "ocr_conv2d_wgrad_f16", b, px, pdy, pdw, pws, ctypes.c_size_t(nbytes), st) == INVALID_ARG, field
        assert _raw(L, "ocr_conv2d_wgrad_slabs_f16", b, px, pdy, pws, ctypes.c_size_t(nbytes), st) == INVALID_ARG, field
        assert _raw(L, "ocr_conv2d_wgrad_reduce_f32", b, pws, pdw, st) == INVALID_ARG, field
        assert _raw(L, "ocr_conv2d_wgrad_variant", b, name, ctypes.c_size_t(128)) == INVALID_ARG, field
        assert L.call_size("ocr_conv2d_wgrad_workspace", b) == 0, field
    torch.cuda.synchronize()
    assert untouched(ws) and untouched(dw) and bands_untouched(wg) and bands_untouched(dg)
    # and the same buffers take the well-formed call
    assert _raw(L, "ocr_conv2d_wgrad_f16", ref, px, pdy, pdw, pws, ctypes.c_size_t(nbytes), st) == OK
    torch.cuda.synchronize()
    assert bool((dw == 0).all())
