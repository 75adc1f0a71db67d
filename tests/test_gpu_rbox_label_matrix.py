"""GPU: every extern "C" entry of csrc/rbox.hip (9) and csrc/labels.hip (4) through the C ABI, at the shapes where its code
changes path, against float64 NumPy written here from the formulas of include/ocr_hip.h, tests/test_rbox_host.decode_ref,
oracle.cvgeom.fill_poly and oracle/labels.py.  No kernel is its own oracle: the label entries read cover maps built on the
host from fill_poly, the head backward reads what the device stored and is compared with the derivative at the true z.
Every output and workspace is a Guard (0xFF-filled between bands), a workspace Guard has exactly the queried size, and on
every refusal status every one of them must come back untouched.  ROWS is the inventory (name -> Row);
tests/test_rbox_label_matrix_inventory.py lists it against the sources and checks, with the oracles alone, that each row's
inputs have the pattern the row is named after.

Rows and the edges they are built to reach
  head/<P>            P 1 | 255 | 256 | 257 | 1000 (256-thread workgroups).  z in [-4, 4]; the first min(P, 13) pixels carry
                      the directed values 0, +-1e-4, +-17, +-30, +-88, +-89, +-104 in every column (expf overflow from 88.8,
                      sigma stored as 0, 1, the angle as +-f32(pi/4)), z5 = 0 at every seventh later pixel.
  loss/<P>            P 1 | 255 | 1024 | 1025 (one -> two workgroups of 256 x 4) | 32 * 1024 + 1 (T = 33 partial rows: the
                      finaliser's second trip over its 32 row groups) | 1024 * 1024 + 1 (ceil(P / 1024) = 1025 > the 1024
                      cap: the grid-stride loops of reduce and of bwd take further trips)
  loss/1025/<content> ties (pixels p % 8 = 1 | 2 | 3 tie gp[k] == gt[k] in one | two | all four components, nowhere
                      else), zero-gt, big (distances in [480, 512]), angles (theta differences 0, 1e-4, pi/2), no-positive
                      (y = 0), all-masked (m = 0: U = 1e-5)
  decode/<hw>/<pattern>  n = 3; h * w 1 | 255 | 256 | 257 | 257 * 256 (257 workgroups: the scan's first carry across a
                      256-wide chunk) | 2 * 65536 + 300 (514 workgroups: the second carry); w != h except at h * w = 1,
                      where the three totals cannot all differ either.  Image 0 carries the pattern, image 1 a random half,
                      image 2 nothing (everything, where the pattern selects nothing).  Each under max_k = 1, T - 1, T, T + 1
                      (T the largest total).  Patterns: all, none, last, lane63, lane0, runs (lane 63 and lane 0 of the next
                      wave, so every fourth run crosses a workgroup), random, threshold (unselected pixels hold exactly the
                      threshold), nan (unselected pixels hold NaN).  Angles +0.0, -0.0, +-1e-6, +-f32(pi/4) among the rest.
  mean/<h>x<w>/<inv>  masks 1x1 | 40x56 | 300x520 x inv_scale 1 | 0.5 | 0.25; per row random quads, a point, two lines, a quad
                      off each side, the whole mask (300x520: 156000 / 256 > 600 strides), negative fractions, +-2^22,
                      +-1e9, a NaN and an Inf vertex
  cover/<h>x<w>/v<V>  (3,63) (4,64) (5,65) (37,130) x V 3 | 4 | 5 | 8 (64 x 4 tiles, 32 polygons staged per pass); four images
                      with counts from {0, 1, 32, 33, 64, 65, 254}, the last with counts = max_polys + 7 (clamped)
  icdar/<size>/<step> 64 | 65 x step 1 | 4 (x == h - 1 is sampled at 65 only), n = 3 at 420 step 1 (4 233 600 items > the
                      16384 x 256 threads of lgrid: a second trip)
  pixellink/<row>     (100,140) -> (25,35) | (33,47), (64,64) -> (128,128) | (1,1), n = 3 (210,210) -> (420,420) past the cap
  rboxlab/<P>/<h>x<w>s<step>  max_polys 1 | 12 | 254 x (64,64,1) (37,53,4) (130,97,4: 825 cells, the last workgroup has 57);
                      rboxlab/above: a cover map with owners above max_polys

Bounds (u = 2^-24, g(m) = m u / (1 - m u); library calls: logf ELOG = 3.064 ulp as tests/test_gpu_loss_matrix.py measured
and took it, sinf / cosf ESIN = 4 ulp, the OpenCL full-profile figure; one ulp = 2 u; nothing is fitted to the kernels)
  head forward   |err| <= 16 * 2^-23 |ref| + 2^-126 scale (scale 1 | text_scale | pi/4): the present 16 ulp, and the smallest
                 normal where the true sigma is subnormal (z <= -87.4: the quotient may be flushed).  Finite, distances in
                 [0, text_scale], |angle| <= f32(pi/4) (the f32 the kernel multiplies tanhf <= 1 by; 2.2e-8 above pi/4).
  head backward  reference: the float64 derivative d K sigma(z) sigma(-z) at the TRUE z (K = 1 | text_scale | pi/2).  The
                 kernel recovers sigma from the stored output, which carries the forward bound: eps = 16 * 2^-23 sigma +
                 2^-126 for the score, one more u sigma (the division by text_scale) for a distance; for the angle
                 sigma = geo4 / (pi/2) + 0.5 and eps is ABSOLUTE, about ulp(0.5): (16 * 2^-23 + 2 u) |sigma - 0.5| + 2^-126
                 + 2^-24 (the addition rounds at 2^-24 whatever sigma - 0.5 was).  Through sigma (1 - sigma):
                 E = (|1 - 2 sigma| eps + eps^2) |d| K, and the kernel's own five operations: E + g(5) (|ref| + E) + 2^-149.
  loss sums      per term v_i formed with |v^_i - v_i| <= d_i:  |dev - ref| <= g(m) sum(|v_i| + d_i) + sum d_i + 2^-149,
                 m = ceil(P / (256 T)) [per-thread trips] + 6 [wave steps] + 3 [cross-wave adds] + 1 [f64 -> f32].
                 d: y p m g(2); y m, p m g(1); L_aabb y m: A_i three roundings, A_i + 1 four; A_u = A_g + A_p - A_i with
                 A_u >= (A_g + A_p) / 2 and A_i <= A_u: 8 + 3 + 1 = 12, A_u + 1 thirteen; the quotient 18: d = g(18) y m +
                 g(2 ELOG + 1) |v|; L_theta = 2 sin^2(x / 2), x = q4 - g4 rounded once (|x| <= pi: (x/2) / sin(x/2) <= pi/2):
                 rel(sin) <= (2 ESIN + pi/2) u, squared, doubled, times y m: d = g(4 ESIN + 6) |v|.
  loss out       formed in double on the device from the double totals: out2 = tot3 / P, out3 = tot4 / P: B / P + u |ref|;
                 L_cls = 0.01 (1 - 2 I / U): 0.02 (B0 / U' + I (B1 + B2) / U'^2) + u |ref| with U' = U - B1 - B2; out0 the sum.
  d_cls          m (y c0 + c1), c0 = -0.02 s / U, c1 = 0.02 s I / U^2 from the f32 sums: U two additions, c0 two more, c1
                 four more, multiply-add and mask three: g(11) S, S = |m| (|y c0| + |c1|), plus the sums' own bounds
                 carried through c0 (rU = (B1 + B2) / U') and c1 (2 rU and B0 / I), referred to the float64 sums.
  d_geo          c = s y m / P three roundings; reciprocals of A_u + 1 (14) and A_i + 1 (5); (dap - dai) iu: 17, dai ii: 7,
                 the difference and c: g(22) |c| ((|dap| + |dai|) iu + |dai| ii); angle: g(2 ESIN + 6) 20 |c| (|sin x| + |x|).
                 dai follows the header's STRICT rule, written out: the intersection share only where gp[k] < gt[k].
  decode         counts, total, order, score column, untouched rows: exact.  Coordinates: 16 ulp at the magnitude
                 M = max(|origin|) + 2 (W + H) of each quad's own intermediates (sin and cos 8 u each on at most
                 2 (W + H), eight more roundings: <= 16 u M <= 16 ulp(M)).
  mean           u |ref| + n 2^-53 mean|score| + 2^-149: one f32 rounding of the f64 mean and the f64 reordering of n terms.
  cover, icdar, pixellink, rbox labels   bit for bit; the rbox geometry additionally within 2e-3 px of float64 (five f32
                 roundings at magnitude <= 2^12, the present test's bound).

Findings: none.  No row was over its bound, no exact row differed, no refusal wrote anything.

MEASURED (largest |err| / bound over the rows on the MI355X, f16 library; the kernels here read f32 and integers only)
  rbox_head_fwd score / geo      0.189 / 0.189        rbox_loss_bwd d_cls / d_geo    0.064 / 0.318
  rbox_head_bwd                  0.398                rbox_decode coordinates        0.083
  rbox_loss_fwd sums / out       0.129 / 0.375        quad_mean_score                0.946 (the one f32 rounding of the mean)
  No row was over its bound and no exact row differed; the bf16 library compiles the same code and passes the same rows
  (run once by hand; like tests/test_gpu_decode_matrix.py this file is not run a second time by tests/test_gpu_bf16.py).  Time on the MI355X: the file's 118 tests about 4 s;
  slowest test_loss[loss/1048577] 0.28 s (the float64 reference over 1 M pixels on the host).
"""
import ctypes
import math
from functools import partial

import numpy as np
import pytest
import torch

import matrix_support
import test_rbox_host as H
from matrix_support import (FL, INVALID_ARG, OK, SZ, U32, UNSUPPORTED, WORKSPACE, Guard, _bits_equal, _cdiv, _g, _lib, _ratio, _raw,
                            _rc, _rng, f32, f64)
from oracle import cvgeom as C
from oracle import labels as OL

pytestmark = pytest.mark.gpu
_note = partial(matrix_support._note, "rbl")
i32, u8 = np.int32, np.uint8
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
ELOG, ESIN = 3.064, 4.0
TINY = 2.0 ** -126


class Row:
    def __init__(self, name, entries, build, **meta):
        self.name, self.entries, self.build = name, tuple(entries), build
        self.__dict__.update(meta)


ROWS = {}
_CASES = {}


def _row(name, entries, build, **meta):
    assert name not in ROWS
    ROWS[name] = Row(name, entries, build, **meta)


def case(name):
    """a row's inputs and references, built once and left unchanged"""
    if name not in _CASES:
        _CASES[name] = ROWS[name].build()
    return _CASES[name]


def _t(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


def _size(L, name, *ints):
    return int(L._fn(name, SZ)(*[ctypes.c_int(int(v)) for v in ints]))


def _refused(L, name, args, status, guards, what):
    assert _rc(L, name, *args) == status, what
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards), what


# ------------------------------------------------------------------------------------------------ head
HEAD = ("ocr_rbox_head_fwd", "ocr_rbox_head_bwd")
HEAD_P = (1, 255, 256, 257, 1000)
DIRECTED = (0.0, 1e-4, -1e-4, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0)
TS = 512.0
HEAD_RTOL = 16 * 2.0 ** -23
HEAD_SCALE = np.array([1.0] + [TS] * 4 + [math.pi / 4])
HEAD_K = np.array([1.0] + [TS] * 4 + [math.pi / 2])


def _sigma(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def head_case(P):
    rng = _rng("rbl", "head", P)
    z = rng.uniform(-4, 4, (P, 6)).astype(f32)
    for p in range(min(P, 13)):
        for c in range(6):
            z[p, c] = DIRECTED[(p + 2 * c) % 13]
    z[13::7, 5] = 0.0
    d = rng.standard_normal((P, 6)).astype(f32)
    z64 = z.astype(f64)
    s = _sigma(z64)
    fwd = np.concatenate([s[:, :1], s[:, 1:5] * TS, np.tanh(z64[:, 5:] / 2) * (math.pi / 4)], axis=1)      # [P, 6]: score, geo
    eps = HEAD_RTOL * s + TINY
    eps[:, 1:5] += U32 * s[:, 1:5] + 2.0 ** -149
    eps[:, 5] = (HEAD_RTOL + 2 * U32) * np.abs(s[:, 5] - 0.5) + TINY + 2.0 ** -24
    bwd = d.astype(f64) * HEAD_K * (s * _sigma(-z64))
    E = (np.abs(1 - 2 * s) * eps + eps * eps) * np.abs(d.astype(f64)) * HEAD_K
    return dict(P=P, z=z, d=d, fwd=fwd, fwd_bound=HEAD_RTOL * np.abs(fwd) + TINY * HEAD_SCALE, bwd=bwd,
                bwd_bound=E + _g(5) * (np.abs(bwd) + E) + 2.0 ** -149)


for _P in HEAD_P:
    _row("head/%d" % _P, HEAD, lambda P=_P: head_case(P))


@pytest.mark.parametrize("P", HEAD_P)
def test_head(device, P):
    L, _ = _lib()
    c = case("head/%d" % P)
    z, d = _t(c["z"], device), c["d"]
    score, geo, dz = Guard((P,), F32, device), Guard((P, 5), F32, device), Guard((P, 6), F32, device)
    guards = (score, geo, dz)
    for what, a in {"z null": (None, P, FL(TS), score, geo), "score null": (z, P, FL(TS), None, geo), "geo null": (z, P, FL(TS), score, None),
                    "P 0": (z, 0, FL(TS), score, geo), "P -1": (z, -1, FL(TS), score, geo)}.items():
        _refused(L, "ocr_rbox_head_fwd", a, INVALID_ARG, guards, what)
    assert _rc(L, "ocr_rbox_head_fwd", z, P, FL(TS), score, geo) == OK
    torch.cuda.synchronize()
    got = np.concatenate([score.np()[:, None], geo.np()], axis=1)
    assert (got[:, :5] >= 0).all() and (got[:, 1:5] <= f32(TS)).all() and (got[:, 0] <= 1).all() and (np.abs(got[:, 5]) <= f32(math.pi / 4)).all()
    zero = c["z"][:, 5] == 0
    assert (got[zero, 5].view(i32) == 0).all(), "z5 = 0 must give the angle +0.0"
    _note("rbox_head_fwd", "score P%d" % P, _ratio(np.abs(got[:, 0] - c["fwd"][:, 0]), c["fwd_bound"][:, 0]))
    _note("rbox_head_fwd", "geo P%d" % P, _ratio(np.abs(got[:, 1:] - c["fwd"][:, 1:]), c["fwd_bound"][:, 1:]))
    # backward from the outputs the device stored
    ds, dg = _t(d[:, 0].copy(), device), _t(d[:, 1:].copy(), device)
    for what, a in {"score null": (None, ds, geo, dg, P, FL(TS), dz), "geo null": (score, ds, None, dg, P, FL(TS), dz),
                    "dz null": (score, ds, geo, dg, P, FL(TS), None), "P 0": (score, ds, geo, dg, 0, FL(TS), dz)}.items():
        assert _rc(L, "ocr_rbox_head_bwd", *a) == INVALID_ARG, what
        torch.cuda.synchronize()
        assert dz.untouched(), what
    for form, (a_ds, a_dg, zeros) in {"both": (ds, dg, []), "dgeo NULL": (ds, None, [1, 2, 3, 4, 5]), "dscore NULL": (None, dg, [0])}.items():
        out = Guard((P, 6), F32, device)
        assert _rc(L, "ocr_rbox_head_bwd", score, a_ds, geo, a_dg, P, FL(TS), out) == OK
        torch.cuda.synchronize()
        g = out.np()
        live = [k for k in range(6) if k not in zeros]
        assert (g[:, zeros] == 0).all(), form
        _note("rbox_head_bwd", "%s P%d" % (form, P), _ratio(np.abs(g[:, live] - c["bwd"][:, live]), c["bwd_bound"][:, live]))
    assert score.ok() and geo.ok()


# ------------------------------------------------------------------------------------------------ loss
LOSS = ("ocr_rbox_loss_workspace", "ocr_rbox_loss_fwd", "ocr_rbox_loss_bwd", "ocr_rbox_loss_bwd_dyn")
LOSS_P = (1, 255, 1024, 1025, 32 * 1024 + 1, 1024 * 1024 + 1)
LOSS_CONTENT = ("ties", "zero-gt", "big", "angles", "no-positive", "all-masked")
SEED = 768.0                                            # the static seed; 0.75 * 1024 for the _dyn form


def loss_blocks(P):
    return min(max(_cdiv(P, 1024), 1), 1024)


def tie_pattern(P):
    """bool [P, 4]: the components in which pixel p ties"""
    tie, idx = np.zeros((P, 4), bool), np.arange(P)
    k = (idx // 8) % 4
    one, two, four = idx % 8 == 1, idx % 8 == 2, idx % 8 == 3
    tie[one, k[one]] = True
    tie[two, k[two]] = True
    tie[two, (k[two] + 1 + (idx[two] // 32) % 3) % 4] = True
    tie[four] = True
    return tie


def loss_inputs(P, content):
    rng = _rng("rbl", "loss", P, content)
    y = (rng.uniform(size=P) < 0.4).astype(f32)
    p = rng.uniform(0.05, 0.95, P).astype(f32)
    m = (rng.uniform(size=P) < 0.8).astype(f32)
    gt, gp = np.empty((P, 5), f32), np.empty((P, 5), f32)
    gt[:, :4] = rng.uniform(1, 200, (P, 4))
    gt[:, 4] = rng.uniform(-0.7, 0.7, P)
    gp[:, :4] = gt[:, :4] * rng.uniform(0.6, 1.4, (P, 4)).astype(f32) + rng.uniform(0.5, 3.0, (P, 4)).astype(f32)
    gp[:, 4] = gt[:, 4] + rng.uniform(-0.3, 0.3, P).astype(f32)
    if P == 1:
        y[:], m[:] = 1, 1
    if content == "ties":
        tie = tie_pattern(P)
        gp[:, :4][tie] = gt[:, :4][tie]
        y[tie.any(1)], m[tie.any(1)] = 1, 1
    elif content == "zero-gt":
        gt[:, :4] = 0
        gp[:, :4] = rng.uniform(1, 200, (P, 4))
    elif content == "big":
        gt[:, :4], gp[:, :4] = rng.uniform(480, 512, (P, 4)), rng.uniform(480, 512, (P, 4))
    elif content == "angles":
        k = np.arange(P) % 3
        gp[k == 0, 4] = gt[k == 0, 4]
        gp[k == 1, 4] = gt[k == 1, 4] + f32(1e-4)
        gt[k == 2, 4], gp[k == 2, 4] = -f32(math.pi / 4), f32(math.pi / 4)
    elif content == "no-positive":
        y[:] = 0
    elif content == "all-masked":
        m[:] = 0
    return y, p, gt, gp, m


def loss_case(P, content="plain"):
    """inputs, float64 references and bounds (the docstring's derivation, line by line)"""
    y32, p32, gt32, gp32, m32 = loss_inputs(P, content)
    y, p, g, q, m = (a.astype(f64) for a in (y32, p32, gt32, gp32, m32))
    ym = y * m
    hg, wg, hp, wp = g[:, 0] + g[:, 2], g[:, 1] + g[:, 3], q[:, 0] + q[:, 2], q[:, 1] + q[:, 3]
    w = np.minimum(g[:, 1], q[:, 1]) + np.minimum(g[:, 3], q[:, 3])
    h = np.minimum(g[:, 0], q[:, 0]) + np.minimum(g[:, 2], q[:, 2])
    ai = w * h
    au = hg * wg + hp * wp - ai
    l_aabb = -np.log((ai + 1) / (au + 1))
    x = q[:, 4] - g[:, 4]
    assert (np.abs(x) <= math.pi).all()
    l_theta = 2 * np.sin(x / 2) ** 2                        # 1 - cos x
    v = np.stack([y * p * m, ym, p * m, l_aabb * ym, l_theta * ym])
    d = np.stack([_g(2) * v[0], _g(1) * v[1], _g(1) * v[2], _g(18) * ym + _g(2 * ELOG + 1) * np.abs(v[3]), _g(4 * ESIN + 6) * v[4]])
    T = loss_blocks(P)
    m_sum = _cdiv(P, 256 * T) + 6 + 3 + 1
    sums = v.sum(1)
    B = _g(m_sum) * (np.abs(v) + d).sum(1) + d.sum(1) + 2.0 ** -149
    U = sums[1] + sums[2] + 1e-5
    Ulo = U - B[1] - B[2]
    assert Ulo > 0
    l_cls = 0.01 * (1 - 2 * sums[0] / U)
    out = np.array([sums[3] / P + 20 * sums[4] / P + l_cls, l_cls, sums[3] / P, sums[4] / P])
    b_cls = 0.02 * (B[0] / Ulo + sums[0] * (B[1] + B[2]) / Ulo ** 2)
    out_b = np.array([B[3] / P + 20 * B[4] / P + b_cls, b_cls, B[3] / P, B[4] / P]) + U32 * np.abs(out) + 2.0 ** -149
    # gradients, seed s
    s = SEED
    U32f = f64(f32(1e-5))
    Ug = sums[1] + sums[2] + U32f
    c0, c1 = -0.02 * s / Ug, 0.02 * s * sums[0] / Ug ** 2
    d_cls = m * (y * c0 + c1)
    rU = (B[1] + B[2] + U32 * U32f) / Ulo
    d_cls_b = (_g(11) * m * (np.abs(y * c0) + abs(c1)) + 1.001 * m * (np.abs(y * c0) * rU + abs(c1) * 2 * rU + 0.02 * s * B[0] / Ulo ** 2)
               + 2.0 ** -149)
    c = s * ym / P
    iu, ii = 1 / (au + 1), 1 / (ai + 1)
    d_geo, d_geo_b = np.zeros((P, 5)), np.zeros((P, 5))
    for k in range(4):
        dap = hp if k & 1 else wp
        dai = np.where(q[:, k] < g[:, k], h if k & 1 else w, 0.0)           # STRICTLY smaller: a tie gives the prediction nothing
        d_geo[:, k] = c * ((dap - dai) * iu - dai * ii)
        d_geo_b[:, k] = _g(22) * np.abs(c) * ((np.abs(dap) + np.abs(dai)) * iu + np.abs(dai) * ii)
    d_geo[:, 4] = c * 20 * np.sin(x)
    d_geo_b[:, 4] = _g(2 * ESIN + 6) * 20 * np.abs(c) * (np.abs(np.sin(x)) + np.abs(x))
    d_geo_b += 2.0 ** -149 * (ym[:, None] != 0)
    return dict(P=P, content=content, inputs=(y32, p32, gt32, gp32, m32), T=T, sums=sums, sums_b=B, out=out, out_b=out_b, d_cls=d_cls,
                d_cls_b=d_cls_b, d_geo=d_geo, d_geo_b=d_geo_b, live=ym != 0)


for _P in LOSS_P:
    _row("loss/%d" % _P, LOSS, lambda P=_P: loss_case(P))
for _c in LOSS_CONTENT:
    _row("loss/1025/%s" % _c, LOSS, lambda c=_c: loss_case(1025, c))


class LossCall:
    def __init__(self, L, device, c):
        self.L, self.P = L, c["P"]
        self.y, self.p, self.gt, self.gp, self.m = (_t(a, device) for a in c["inputs"])
        self.bytes = _size(L, "ocr_rbox_loss_workspace", self.P)
        self.sums, self.out = Guard((5,), F32, device), Guard((4,), F32, device)
        self.ws = Guard((self.bytes,), U8, device)
        self.d_cls, self.d_geo = Guard((self.P,), F32, device), Guard((self.P, 5), F32, device)

    def fwd(self, **over):
        a = dict(y=self.y, p=self.p, gt=self.gt, gp=self.gp, m=self.m, P=self.P, sums=self.sums, out=self.out, ws=self.ws, ws_bytes=self.bytes)
        a.update(over)
        return _rc(self.L, "ocr_rbox_loss_fwd", a["y"], a["p"], a["gt"], a["gp"], a["m"], a["P"], a["sums"], a["out"], a["ws"], SZ(a["ws_bytes"]))

    def bwd(self, seed, d_cls=None, d_geo=None, scale=False, **over):
        a = dict(y=self.y, gt=self.gt, gp=self.gp, m=self.m, P=self.P, sums=self.sums, d_cls=d_cls or self.d_cls, d_geo=d_geo or self.d_geo)
        a.update(over)
        head = (a["y"], a["gt"], a["gp"], a["m"], a["P"], a["sums"], FL(seed))
        if scale is False:
            return _rc(self.L, "ocr_rbox_loss_bwd", *head, a["d_cls"], a["d_geo"])
        return _rc(self.L, "ocr_rbox_loss_bwd_dyn", *head, scale, a["d_cls"], a["d_geo"])


LOSS_ROWS = [n for n in ROWS if n.startswith("loss/")]


@pytest.mark.parametrize("name", LOSS_ROWS)
def test_loss(device, name):
    L, _ = _lib()
    c = case(name)
    P = c["P"]
    call = LossCall(L, device, c)
    assert call.bytes == loss_blocks(P) * 32
    assert call.fwd() == OK
    assert call.bwd(SEED) == OK
    torch.cuda.synchronize()
    assert call.ws.ok()
    sums, out, d_cls, d_geo = call.sums.np(), call.out.np(), call.d_cls.np(), call.d_geo.np()
    _note("rbox_loss_fwd", "sums " + name, _ratio(np.abs(sums - c["sums"]), c["sums_b"]))
    _note("rbox_loss_fwd", "out " + name, _ratio(np.abs(out - c["out"]), c["out_b"]))
    _note("rbox_loss_bwd", "d_cls " + name, _ratio(np.abs(d_cls - c["d_cls"]), c["d_cls_b"]))
    _note("rbox_loss_bwd", "d_geo " + name, _ratio(np.abs(d_geo - c["d_geo"]), c["d_geo_b"]))
    assert (d_geo[~c["live"]] == 0).all(), "d_geo is exactly 0 where y m = 0"
    if c["content"] == "no-positive":
        assert (d_geo == 0).all() and abs(c["out"][0] - 0.01) < 1e-15 and c["out"][2] == 0 and c["out"][3] == 0
    if c["content"] == "all-masked":
        assert (d_cls == 0).all() and (d_geo == 0).all() and abs(c["out"][1] - 0.01) < 1e-15
    if c["content"] in ("plain", "ties") and P > 1:
        assert (d_geo[c["live"]] != 0).any()


def test_loss_dyn_and_status(device):
    L, _ = _lib()
    c = case("loss/1025")
    call = LossCall(L, device, c)
    guards = (call.sums, call.out, call.ws, call.d_cls, call.d_geo)
    for what, over, status in [("ws_bytes - 1", dict(ws_bytes=call.bytes - 1), WORKSPACE), ("P 0", dict(P=0), INVALID_ARG),
                               ("P -1", dict(P=-1), INVALID_ARG)] + [("%s null" % k, {k: None}, INVALID_ARG)
                                                                      for k in ("y", "p", "gt", "gp", "m", "sums", "out", "ws")]:
        assert call.fwd(**over) == status, what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in guards), what
    assert [_size(L, "ocr_rbox_loss_workspace", P) for P in (0, -3) + LOSS_P] == [0, 0] + [loss_blocks(P) * 32 for P in LOSS_P]
    assert [loss_blocks(P) for P in LOSS_P] == [1, 1, 1, 2, 33, 1024]
    assert call.fwd() == OK
    scale = _t(np.array([1024.0], f32), device)
    for what, kw in [("loss_scale null", dict(scale=None)), ("P 0", dict(P=0)), ("P 0 dyn", dict(P=0, scale=scale))] + \
            [("%s null" % k, {k: None}) for k in ("y", "gt", "gp", "m", "sums")]:
        assert call.bwd(0.75, **kw) == INVALID_ARG, what
        torch.cuda.synchronize()
        assert call.d_cls.untouched() and call.d_geo.untouched(), what
    for k in ("d_cls", "d_geo"):
        assert _rc(L, "ocr_rbox_loss_bwd", call.y, call.gt, call.gp, call.m, call.P, call.sums, FL(1.0),
                   None if k == "d_cls" else call.d_cls, None if k == "d_geo" else call.d_geo) == INVALID_ARG
    torch.cuda.synchronize()
    assert call.d_cls.untouched() and call.d_geo.untouched()
    a_cls, a_geo = Guard((call.P,), F32, device), Guard((call.P, 5), F32, device)
    assert call.bwd(SEED) == OK and call.bwd(0.75, d_cls=a_cls, d_geo=a_geo, scale=scale) == OK
    torch.cuda.synchronize()
    _bits_equal(a_cls.np(), call.d_cls.np(), "d_cls, dyn against the static product")
    _bits_equal(a_geo.np(), call.d_geo.np(), "d_geo, dyn against the static product")


# ------------------------------------------------------------------------------------------------ decode
DECODE = ("ocr_rbox_decode_workspace", "ocr_rbox_decode")
DECODE_HW = {1: (1, 1), 255: (15, 17), 256: (8, 32), 257: (1, 257), 257 * 256: (257, 256), 2 * 65536 + 300: (4, 32843)}
THR, SCALE = f32(0.7), 4.0
ANGLES = (0.0, -0.0, 1e-6, -1e-6, math.pi / 4, -math.pi / 4)
PATTERNS = {
    "all": lambda i, rng: np.ones(i.size, bool),
    "none": lambda i, rng: np.zeros(i.size, bool),
    "last": lambda i, rng: i == i.size - 1,
    "lane63": lambda i, rng: i % 64 == 63,
    "lane0": lambda i, rng: i % 64 == 0,
    "runs": lambda i, rng: (i % 64 == 63) | ((i % 64 == 0) & (i > 0)),
    "random": lambda i, rng: rng.uniform(size=i.size) < 0.3,
    "threshold": lambda i, rng: rng.uniform(size=i.size) < 0.3,
    "nan": lambda i, rng: rng.uniform(size=i.size) < 0.3,
}


def decode_vec(score, geo, thresh, scale):
    """decode_ref of tests/test_rbox_host.py for whole arrays (float64; the inventory test holds the two together)"""
    h, w = score.shape
    ys, xs = np.nonzero(score > score.dtype.type(thresh))
    g = geo[ys, xs].astype(f64)
    d0, d1, d2, d3, th = g.T
    Hh, W, c, s, z = d0 + d2, d1 + d3, np.cos(th), np.sin(th), np.zeros(len(ys))
    pos = th >= 0
    lx = np.where(pos, [z, W, W, z], [-W, z, z, -W])
    ly = np.stack([-Hh, -Hh, z, z])
    ax, ay = np.where(pos, d3, -d1), -d2
    rax, ray = ax * c + ay * s, -ax * s + ay * c
    rows = np.zeros((len(ys), 9))
    rows[:, 0:8:2] = ((xs * scale + (lx * c + ly * s)) - rax).T
    rows[:, 1:8:2] = ((ys * scale + (-lx * s + ly * c)) - ray).T
    rows[:, 8] = score[ys, xs]
    return rows


def decode_case(hw, pattern):
    h, w = DECODE_HW[hw]
    rng = _rng("rbl", "decode", hw, pattern)
    i = np.arange(hw)
    sel = [PATTERNS[pattern](i, rng), rng.uniform(size=hw) < 0.5]
    sel.append(np.zeros(hw, bool) if sel[0].any() else np.ones(hw, bool))
    j = 0
    while hw > 2 and int(sel[1].sum()) in (int(sel[0].sum()), int(sel[2].sum())):
        sel[1][j] = not sel[1][j]
        j += 1
    sel = np.stack(sel)
    score = np.where(sel, rng.uniform(0.71, 1.0, (3, hw)), rng.uniform(0.0, 0.69, (3, hw))).astype(f32)
    off = ~sel & (rng.uniform(size=(3, hw)) < 0.1)
    score[off] = THR                                        # a tenth of the unselected pixels sit exactly at the threshold
    if pattern == "threshold":
        score[0][~sel[0]] = THR
    if pattern == "nan":
        score[0][~sel[0]] = np.nan
    geo = np.zeros((3, hw, 5), f32)
    geo[..., :4] = rng.uniform(1, 200, (3, hw, 4))
    geo[..., 4] = rng.uniform(-0.78, 0.78, (3, hw))
    for k, a in enumerate(ANGLES):
        geo[:, k::16, 4] = f32(a)
    totals = [int(s.sum()) for s in sel]
    T = max(totals)
    return dict(h=h, w=w, hw=hw, sel=sel, score=score.reshape(3, h, w), geo=geo.reshape(3, h, w, 5), totals=totals,
                max_ks=sorted({k for k in (1, T - 1, T, T + 1) if k >= 1}))


def decode_oracle(c):
    """per image: (rows float64 [k, 9], coordinate bound [k, 1]); decode_ref itself on the small maps"""
    if "ref" not in c:
        fn = H.decode_ref if c["hw"] <= 257 else decode_vec
        c["ref"] = []
        for b in range(3):
            rows = fn(c["score"][b], c["geo"][b], THR, SCALE)
            ys, xs = np.nonzero(c["sel"][b].reshape(c["h"], c["w"]))
            g = c["geo"][b][ys, xs].astype(f64)
            M = np.maximum(xs, ys) * SCALE + 2 * g[:, :4].sum(1)
            c["ref"].append((rows, 16 * np.spacing(M.astype(f32)).astype(f64)[:, None]))
    return c["ref"]


for _hw in DECODE_HW:
    for _pat in PATTERNS:
        _row("decode/%d/%s" % (_hw, _pat), DECODE, lambda hw=_hw, p=_pat: decode_case(hw, p))


def _decode_call(L, device, score, geo, n, h, w, max_k, boxes, counts, total, ws, ws_bytes, thr=THR):
    return _rc(L, "ocr_rbox_decode", score, geo, n, h, w, FL(thr), FL(SCALE), max_k, boxes, counts, total, ws, SZ(ws_bytes))


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("hw", list(DECODE_HW))
def test_decode(device, hw, pattern):
    L, _ = _lib()
    c = case("decode/%d/%s" % (hw, pattern))
    ref = decode_oracle(c)
    h, w = c["h"], c["w"]
    score, geo = _t(c["score"], device), _t(c["geo"], device)
    need = _size(L, "ocr_rbox_decode_workspace", 3, h, w)
    assert need == 3 * _cdiv(hw, 256) * 4
    bits = [c["score"][b].reshape(-1)[c["sel"][b]].view(i32) for b in range(3)]
    worst = 0.0
    for max_k in c["max_ks"]:
        boxes, counts, total = Guard((3, max_k, 9), F32, device), Guard((3,), I32, device), Guard((3,), I32, device)
        ws = Guard((need,), U8, device)
        assert _decode_call(L, device, score, geo, 3, h, w, max_k, boxes, counts, total, ws, need) == OK
        torch.cuda.synchronize()
        assert ws.ok()
        assert total.raw().tolist() == c["totals"] and counts.raw().tolist() == [min(t, max_k) for t in c["totals"]], max_k
        got = boxes.raw()
        for b in range(3):
            k = min(c["totals"][b], max_k)
            assert np.array_equal(got[b, :k, 8].view(i32), bits[b][:k]), "the score column is the raster-ordered selection"
            assert (got[b, k:].view(i32) == -1).all(), "rows at or beyond counts[i] were written"
            rows, bound = ref[b]
            assert len(rows) == c["totals"][b]
            worst = max(worst, _ratio(np.abs(got[b, :k, :8] - rows[:k, :8]), bound[:k]))
    _note("rbox_decode", "%d/%s" % (hw, pattern), worst)


def test_decode_status(device):
    L, _ = _lib()
    c = case("decode/257/random")
    h, w = c["h"], c["w"]
    score, geo = _t(c["score"], device), _t(c["geo"], device)
    need = _size(L, "ocr_rbox_decode_workspace", 3, h, w)
    boxes, counts, total, ws = Guard((3, 16, 9), F32, device), Guard((3,), I32, device), Guard((3,), I32, device), Guard((need,), U8, device)
    guards = (boxes, counts, total, ws)
    base = dict(score=score, geo=geo, n=3, h=h, w=w, max_k=16, boxes=boxes, counts=counts, total=total, ws=ws, ws_bytes=need)
    cases = [("%s null" % k, {k: None}, INVALID_ARG) for k in ("score", "geo", "boxes", "counts", "total", "ws")]
    cases += [("%s %d" % (k, v), {k: v}, INVALID_ARG) for k in ("n", "h", "w", "max_k") for v in (0, -1)]
    cases += [("ws_bytes - 1", dict(ws_bytes=need - 1), WORKSPACE), ("n 65536", dict(n=65536, h=1, w=1, ws_bytes=1 << 40), UNSUPPORTED),
              ("n h w 2^31", dict(n=8, h=16384, w=16384, ws_bytes=1 << 40), UNSUPPORTED)]
    for what, over, status in cases:
        a = dict(base)
        a.update(over)
        assert _decode_call(L, device, a["score"], a["geo"], a["n"], a["h"], a["w"], a["max_k"], a["boxes"], a["counts"], a["total"], a["ws"],
                            a["ws_bytes"]) == status, what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in guards), what
    assert [_size(L, "ocr_rbox_decode_workspace", *a) for a in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (8, 16384, 16384))] == [0, 0, 0, 0]
    assert _decode_call(L, device, score, geo, 3, h, w, 16, boxes, counts, total, ws, need) == OK
    torch.cuda.synchronize()
    assert all(g.ok() for g in guards) and counts.raw().tolist() == [min(t, 16) for t in c["totals"]]


# ------------------------------------------------------------------------------------------------ mean score
MEAN = ("ocr_quad_mean_score",)
MEAN_MASKS, MEAN_INV = ((1, 1), (40, 56), (300, 520)), (1.0, 0.5, 0.25)
LIMIT = 2.0 ** 22


def mean_verts(q, inv):
    """the header's vertices: floor(trunc(coord) * inv_scale), coordinates clamped at 2^22 in magnitude"""
    t = np.clip(np.trunc(np.asarray(q, f64)), -LIMIT, LIMIT)
    return np.floor(t * inv).astype(np.int64).reshape(4, 2)


def mean_case(h, w, inv):
    rng = _rng("rbl", "mean", h, w, inv)
    W, Hh = w / inv, h / inv                                # the image the quads live in
    box = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    quads = {"random%d" % j: rng.uniform(-0.2, 1.2, 8) * np.tile([W, Hh], 4) for j in range(6)}
    quads["point"] = box(W * 0.4, Hh * 0.4, W * 0.4, Hh * 0.4)
    quads["hline"] = box(W * 0.1, Hh * 0.6, W * 0.9, Hh * 0.6)
    quads["vline"] = box(W * 0.6, Hh * 0.1, W * 0.6, Hh * 0.9)
    quads["off left"] = box(-W - 200.0, Hh * 0.2, -40.5, Hh * 0.7)
    quads["off right"] = box(W + 40.5, Hh * 0.2, 2 * W + 200.0, Hh * 0.7)
    quads["off above"] = box(W * 0.2, -Hh - 200.0, W * 0.7, -40.5)
    quads["off below"] = box(W * 0.2, Hh + 40.5, W * 0.7, 2 * Hh + 200.0)
    quads["whole"] = box(0.0, 0.0, W - 0.5, Hh - 0.5)
    quads["negative fractions"] = [-36.5, -20.5, 90.2, -8.5, 95.5, 60.1, -28.5, 55.5]
    quads["2^22"] = box(-LIMIT, -LIMIT, LIMIT, LIMIT)
    quads["1e9"] = box(-1e9, -1e9, 1e9, 1e9)
    quads["band 1e9"] = box(-1e9, Hh * 0.25, 1e9, Hh * 0.75)
    quads["nan"] = box(W * 0.1, Hh * 0.1, W * 0.8, Hh * 0.8)
    quads["inf"] = box(W * 0.1, Hh * 0.1, W * 0.8, Hh * 0.8)
    names = list(quads)
    q = np.array([quads[k] for k in names], f32)
    q[names.index("nan"), 3] = np.nan
    q[names.index("inf"), 0] = np.inf
    score = rng.uniform(0, 1, (h, w)).astype(f32)
    ref, bound, count = np.zeros(len(q)), np.zeros(len(q)), np.zeros(len(q), np.int64)
    for j, quad in enumerate(q):
        if not np.isfinite(quad).all():
            continue
        mask = C.fill_poly(np.zeros((h, w), u8), mean_verts(quad, inv).astype(i32), 1) > 0
        count[j] = mask.sum()
        if count[j]:
            v = score[mask].astype(f64)
            ref[j] = v.mean()
            bound[j] = U32 * ref[j] + count[j] * 2.0 ** -53 * np.abs(v).mean() + 2.0 ** -149
    return dict(h=h, w=w, inv=inv, names=names, quads=q, score=score, ref=ref, bound=bound, count=count)


for _h, _w in MEAN_MASKS:
    for _inv in MEAN_INV:
        _row("mean/%dx%d/%g" % (_h, _w, _inv), MEAN, lambda h=_h, w=_w, v=_inv: mean_case(h, w, v))


@pytest.mark.parametrize("inv", MEAN_INV)
@pytest.mark.parametrize("hw", MEAN_MASKS, ids=lambda s: "%dx%d" % s)
def test_quad_mean_score(device, hw, inv):
    L, _ = _lib()
    c = case("mean/%dx%d/%g" % (hw + (inv,)))
    k = len(c["quads"])
    quads, score, mean = _t(c["quads"], device), _t(c["score"], device), Guard((k,), F32, device)
    h, w = hw
    assert _rc(L, "ocr_quad_mean_score", quads, 0, score, h, w, FL(inv), mean) == OK            # k = 0: no launch
    assert _raw(L, "ocr_quad_mean_score", None, ctypes.c_int(0), None, ctypes.c_int(h), ctypes.c_int(w), FL(inv), None, L.stream_ptr()) == OK
    for what, a in {"k -1": (quads, -1, score, h, w, FL(inv), mean), "h 0": (quads, k, score, 0, w, FL(inv), mean),
                    "w 0": (quads, k, score, h, 0, FL(inv), mean), "h 32769": (quads, k, score, 32769, w, FL(inv), mean),
                    "w 32769": (quads, k, score, h, 32769, FL(inv), mean), "inv 0": (quads, k, score, h, w, FL(0.0), mean),
                    "inv -1": (quads, k, score, h, w, FL(-1.0), mean), "inv 1.5": (quads, k, score, h, w, FL(1.5), mean)}.items():
        _refused(L, "ocr_quad_mean_score", a, UNSUPPORTED, (mean,), what)
    for what, a in {"quads null": (None, k, score, h, w, FL(inv), mean), "score null": (quads, k, None, h, w, FL(inv), mean),
                    "mean null": (quads, k, score, h, w, FL(inv), None)}.items():
        _refused(L, "ocr_quad_mean_score", a, INVALID_ARG, (mean,), what)
    assert _rc(L, "ocr_quad_mean_score", quads, k, score, h, w, FL(inv), mean) == OK
    torch.cuda.synchronize()
    got = mean.np()
    assert (got[c["count"] == 0] == 0).all(), "an empty raster or a non-finite vertex gives 0"
    _note("quad_mean_score", "%dx%d/%g" % (h, w, inv), _ratio(np.abs(got - c["ref"]), c["bound"]))


# ------------------------------------------------------------------------------------------------ cover maps on the host
def cover_ref(h, w, polys, count, ignore):
    """uint32 [h, w]: first | last << 8 | ignored << 16 from one fill_poly raster per polygon"""
    first, last, ign = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
    for j in range(count):
        m = C.fill_poly(np.zeros((h, w), u8), polys[j], 1) > 0
        first[m & (first == 0)] = j + 1
        last[m] = j + 1
        if ignore[j]:
            ign[m] = 1
    return first | (last << 8) | (ign << 16)


# ------------------------------------------------------------------------------------------------ poly_cover
COVER = ("ocr_poly_cover",)
COVER_SHAPES, COVER_VERTS = ((3, 63), (4, 64), (5, 65), (37, 130)), (3, 4, 5, 8)
COVER_COUNTS = {254: (254, 0, 65), 65: (64, 1, 33), 33: (32, 33, 0), 64: (1, 64, 32)}           # max_polys -> counts of images 0..2
COVER_MAX = (254, 65, 33, 64)


def cover_polys(rng, count, V, h, w):
    """integer polygons in [-12, max(h, w) + 12): concave, self-intersecting, straddling tile edges, partly off the image;
    by position mod 8: [1] inside the image, [2] a repeated vertex, [3] one row (a line), [5] a point, [6] wholly off;
    the last one is a triangle on the image's corner (so the highest index covers a pixel)"""
    p = rng.integers(-12, max(h, w) + 12, size=(count, V, 2)).astype(i32)
    p[1::8] = np.clip(p[1::8], 0, [w - 1, h - 1])
    p[2::8, 1] = p[2::8, 0]
    p[3::8, :, 1] = h // 2
    p[5::8] = p[5::8, :1]
    p[6::8, :, 0] -= 10000
    if count:
        p[-1] = np.array([(0, 0), (w - 1, 0), (0, h - 1)] + [(0, h - 1)] * (V - 3), i32)
    return p


def cover_case(h, w, V, max_polys):
    rng = _rng("rbl", "cover", h, w, V)
    counts = list(COVER_COUNTS[max_polys]) + [max_polys + 7]
    polys = np.zeros((4, max_polys, V, 2), i32)
    polys[:, :, 1:3, 0], polys[:, :, 2, 1] = 4 * w, 4 * h          # beyond a count: a triangle over the whole image, never read
    for b, k in enumerate(counts):
        k = min(k, max_polys)
        polys[b, :k] = cover_polys(rng, k, V, h, w)
    ignore = (rng.uniform(size=(4, max_polys)) < 0.25).astype(u8)
    ref = np.stack([cover_ref(h, w, polys[b], min(counts[b], max_polys), ignore[b]) for b in range(4)])
    return dict(h=h, w=w, V=V, max_polys=max_polys, counts=np.array(counts, i32), polys=polys, ignore=ignore, ref=ref)


for _s, (_h, _w) in enumerate(COVER_SHAPES):
    for _v, _V in enumerate(COVER_VERTS):
        _row("cover/%dx%d/v%d" % (_h, _w, _V), COVER, lambda h=_h, w=_w, V=_V, m=COVER_MAX[(_s + _v) % 4]: cover_case(h, w, V, m))


@pytest.mark.parametrize("V", COVER_VERTS)
@pytest.mark.parametrize("hw", COVER_SHAPES, ids=lambda s: "%dx%d" % s)
def test_poly_cover(device, hw, V):
    L, _ = _lib()
    h, w = hw
    c = case("cover/%dx%d/v%d" % (h, w, V))
    polys, counts, ignore = _t(c["polys"], device), _t(c["counts"], device), _t(c["ignore"], device)
    cover = Guard((4, h, w), I32, device)
    mp = c["max_polys"]
    for what, a in {"max_polys 0": (4, 0, V, h, w), "max_polys 255": (4, 255, V, h, w), "verts 2": (4, mp, 2, h, w), "verts 9": (4, mp, 9, h, w),
                    "h 16385": (4, mp, V, 16385, w), "w 16385": (4, mp, V, h, 16385), "n 65536": (65536, mp, V, h, w)}.items():
        _refused(L, "ocr_poly_cover", (polys, counts, ignore) + a + (cover,), UNSUPPORTED, (cover,), what)
    for what, a in {"polys null": (None, counts, ignore, 4, mp, V, h, w, cover), "counts null": (polys, None, ignore, 4, mp, V, h, w, cover),
                    "ignore null": (polys, counts, None, 4, mp, V, h, w, cover), "cover null": (polys, counts, ignore, 4, mp, V, h, w, None),
                    "n 0": (polys, counts, ignore, 0, mp, V, h, w, cover), "h 0": (polys, counts, ignore, 4, mp, V, 0, w, cover),
                    "w -1": (polys, counts, ignore, 4, mp, V, h, -1, cover)}.items():
        _refused(L, "ocr_poly_cover", a, INVALID_ARG, (cover,), what)
    assert _rc(L, "ocr_poly_cover", polys, counts, ignore, 4, mp, V, h, w, cover) == OK
    torch.cuda.synchronize()
    got = cover.raw().view(np.uint32)
    assert np.array_equal(got, c["ref"]), np.argwhere(got != c["ref"])[:4].tolist()


# ------------------------------------------------------------------------------------------------ icdar / pixellink labels
ICDAR, PIXELLINK = ("ocr_icdar_labels",), ("ocr_pixellink_labels",)
ICDAR_ROWS = {"64/1": (1, 64, 1), "64/4": (1, 64, 4), "65/1": (1, 65, 1), "65/4": (1, 65, 4), "420/1": (3, 420, 1)}
PIXELLINK_ROWS = {"100x140-25x35": (1, 100, 140, 25, 35), "100x140-33x47": (1, 100, 140, 33, 47), "64x64-128x128": (1, 64, 64, 128, 128),
                  "64x64-1x1": (1, 64, 64, 1, 1), "210x210-420x420": (3, 210, 210, 420, 420)}
LGRID_THREADS = 16384 * 256


def text_quads(rng, k, h, w):
    """k float32 quadrangles (rotated rectangles, some small) clipped to the image; [0] spans the top rows from border to
    border and [1] runs down the right border, so row 0, column 0 and their wrapped neighbours are all owned"""
    out = []
    for _ in range(k):
        c = rng.uniform([5, 5], [w - 5, h - 5])
        a, b = (rng.uniform(3, 9), rng.uniform(2, 6)) if rng.uniform() < 0.4 else (rng.uniform(10, w / 3), rng.uniform(6, h / 6))
        th = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out.append((np.array([[-a, -b], [a, -b], [a, b], [-a, b]]) / 2) @ R.T + c)
    q = np.clip(np.array(out).reshape(-1, 4, 2), 0, [w - 1, h - 1])
    if k >= 2:
        q[0] = [[0, 0], [w - 1, 0], [w - 1, 7], [0, 7]]
        q[1] = [[w - 9, 3], [w - 1, 3], [w - 1, h - 1], [w - 9, h - 1]]
    return q.astype(f32)


def icdar_ignore(polys, tags, min_text_size=10):
    """the reference's rule for clearing the training mask (datasets/icdar.py, restated in oracle/labels.py)"""
    out = []
    for poly, tag in zip(polys, tags):
        ph = min(np.linalg.norm(poly[0] - poly[3]), np.linalg.norm(poly[1] - poly[2]))
        pw = min(np.linalg.norm(poly[0] - poly[1]), np.linalg.norm(poly[2] - poly[3]))
        out.append(bool(tag) or min(ph, pw) < min_text_size)
    return np.array(out, bool)


def icdar_vec(cover, step):
    """(score [oh, ow, 1], geo [oh, ow, 8], mask [oh, ow, 1]) from one image's cover words: the (first, last) closed form of
    csrc/labels.hip's header, vectorised; held bit for bit to oracle/labels.py on the small rows by the inventory test"""
    h, w = cover.shape
    first, last, ign = (cover & 255).astype(np.int64), ((cover >> 8) & 255).astype(np.int64), (cover >> 16) & 1
    ys, xs = np.mgrid[0:h, 0:w]
    border = (xs == h - 1) | (ys == w - 1)
    geo = np.zeros((h, w, 8), f32)
    for ch, (dx, dy) in enumerate(OL.ICDAR_DIRS):
        nb = np.roll(first, (-dy, -dx), axis=(0, 1))        # first[y + dy, x + dx]; -1 wraps as numpy's index does
        geo[..., ch] = (last > 0) & (border | ((nb != 0) & (nb <= last)))
    s = (slice(None, None, step), slice(None, None, step))
    return (first > 0).astype(f32)[s][..., None], geo[s], (1 - ign).astype(f32)[s][..., None]


def icdar_case(n, size, step):
    rng = _rng("rbl", "icdar", n, size, step)
    polys = [text_quads(rng, k, size, size) for k in ((7, 9, 0) if n == 3 else (8,))]
    tags = [rng.uniform(size=len(p)) < 0.3 for p in polys]
    cover = np.stack([cover_ref(size, size, p.astype(i32), len(p), icdar_ignore(p, t)) for p, t in zip(polys, tags)])
    ref = [icdar_vec(cv, step) for cv in cover]
    return dict(n=n, size=size, step=step, polys=polys, tags=tags, cover=cover, ref=[np.stack([r[j] for r in ref]) for j in range(3)])


def pixellink_vec(cover, nh, nw):
    """(score [nh, nw], link [nh, nw, 8]) from one image's cover words: INTER_NEAREST of score and poly_mask (oracle/labels.py's
    own _resize_nearest), link = the neighbour has the same poly_mask value, borders 1"""
    score = OL._resize_nearest((cover & 255 != 0).astype(u8), nw, nh).astype(f32)
    lab = OL._resize_nearest(((cover >> 8) & 255).astype(np.int64), nw, nh)
    ys, xs = np.mgrid[0:nh, 0:nw]
    border = (xs == nw - 1) | (ys == nh - 1) | (xs == 0) | (ys == 0)
    link = np.zeros((nh, nw, 8), f32)
    for ch, (dx, dy) in enumerate(OL.PIXELLINK_DIRS):
        link[..., ch] = (lab > 0) & (border | (np.roll(lab, (-dy, -dx), axis=(0, 1)) == lab))
    return score, link


def pixellink_case(n, h, w, nh, nw):
    rng = _rng("rbl", "pixellink", n, h, w, nh, nw)
    norm, polys = [], []
    for b in range(n):
        q = text_quads(rng, (6, 9, 0)[b], 1000, 1000).astype(f64) * 1.06 / 1000.0 - 0.03        # normalised, partly outside [0, 1]
        xs, ys = q[:, :, 0].astype(f32), q[:, :, 1].astype(f32)
        norm.append((xs, ys))
        polys.append(np.stack([xs * w, ys * h], axis=2).astype(i32))                           # the reference's np.array(points, np.int32)
    cover = np.stack([cover_ref(h, w, p, len(p), np.zeros(len(p), bool)) for p in polys])
    ref = [pixellink_vec(cv, nh, nw) for cv in cover]
    return dict(n=n, h=h, w=w, nh=nh, nw=nw, norm=norm, cover=cover, ref=[np.stack([r[j] for r in ref]) for j in range(2)])


for _k, _a in ICDAR_ROWS.items():
    _row("icdar/" + _k, ICDAR, lambda a=_a: icdar_case(*a))
for _k, _a in PIXELLINK_ROWS.items():
    _row("pixellink/" + _k, PIXELLINK, lambda a=_a: pixellink_case(*a))


@pytest.mark.parametrize("key", list(ICDAR_ROWS))
def test_icdar_labels(device, key):
    L, _ = _lib()
    c = case("icdar/" + key)
    n, size, step = c["n"], c["size"], c["step"]
    o = _cdiv(size, step)
    cover = _t(c["cover"].view(i32), device)
    score, geo, mask = Guard((n, o, o, 1), F32, device), Guard((n, o, o, 8), F32, device), Guard((n, o, o, 1), F32, device)
    guards = (score, geo, mask)
    _refused(L, "ocr_icdar_labels", (cover, n, size, size - 1, step, score, geo, mask), UNSUPPORTED, guards, "h != w")
    for what, a in {"cover null": (None, n, size, size, step, score, geo, mask), "geo null": (cover, n, size, size, step, score, None, mask),
                    "n 0": (cover, 0, size, size, step, score, geo, mask), "step 0": (cover, n, size, size, 0, score, geo, mask)}.items():
        _refused(L, "ocr_icdar_labels", a, INVALID_ARG, guards, what)
    assert _rc(L, "ocr_icdar_labels", cover, n, size, size, step, score, geo, mask) == OK
    torch.cuda.synchronize()
    want = c["ref"]
    if size <= 65:                                          # the oracle itself; the inventory test holds icdar_vec to it as well
        s, g, m = OL.icdar_generate_rbox((size, size), c["polys"][0], c["tags"][0])
        want = [s[None, ::step, ::step, None].astype(f32), g[None, ::step, ::step], m[None, ::step, ::step, None].astype(f32)]
    for got, ref, what in zip(guards, want, ("score", "geo", "mask")):
        _bits_equal(got.np(), ref, what)


@pytest.mark.parametrize("key", list(PIXELLINK_ROWS))
def test_pixellink_labels(device, key):
    L, _ = _lib()
    c = case("pixellink/" + key)
    n, h, w, nh, nw = c["n"], c["h"], c["w"], c["nh"], c["nw"]
    cover = _t(c["cover"].view(i32), device)
    score, link = Guard((n, nh, nw), F32, device), Guard((n, nh, nw, 8), F32, device)
    for what, a in {"cover null": (None, n, h, w, nh, nw, score, link), "link null": (cover, n, h, w, nh, nw, score, None),
                    "n 0": (cover, 0, h, w, nh, nw, score, link), "new_h 0": (cover, n, h, w, 0, nw, score, link),
                    "w -1": (cover, n, h, -1, nh, nw, score, link)}.items():
        _refused(L, "ocr_pixellink_labels", a, INVALID_ARG, (score, link), what)
    assert _rc(L, "ocr_pixellink_labels", cover, n, h, w, nh, nw, score, link) == OK
    torch.cuda.synchronize()
    want = c["ref"]
    if (nh, nw) == (h // 4, w // 4):                        # the oracle's own ratio
        xs, ys = c["norm"][0]
        s, lk, _ = OL.pixellink_generate_rbox(h, w, xs, ys, np.zeros((len(xs), 4), f32), np.zeros(len(xs), i32))
        want = [s[None], lk[None]]
    _bits_equal(score.np(), want[0], "score")
    _bits_equal(link.np(), want[1], "link")


# ------------------------------------------------------------------------------------------------ rbox labels
RBOXLAB = ("ocr_icdar_rbox_labels",)
RBOXLAB_P, RBOXLAB_SHAPES = (1, 12, 254), ((64, 64, 1), (37, 53, 4), (130, 97, 4))


def small_polys(rng, count, h, w):
    """count integer quadrangles of a few pixels each, so that many of them own cells; the last lies on the sampled origin"""
    c = np.stack([rng.integers(0, w, count), rng.integers(0, h, count)], axis=1)[:, None, :]
    p = (c + rng.integers(-9, 10, size=(count, 4, 2))).astype(i32)
    if count:
        p[-1] = [(0, 0), (8, 0), (8, 8), (0, 8)]
    return p


def rboxlab_case(P, h, w, step, drawn=None):
    """drawn: polygons in the cover maps (default P); more than P gives owners above max_polys"""
    rng = _rng("rbl", "rboxlab", P, h, w, step, drawn)
    drawn = drawn or P
    n, counts = 3, (drawn, max(drawn // 2, 1), 0)
    cs, cf = [], []
    for b in range(n):
        full = small_polys(rng, counts[b], h, w)
        shrunk = (full + np.sign(full.mean(1, keepdims=True) - full).astype(i32)).astype(i32)
        ign = rng.uniform(size=counts[b]) < 0.3
        ign[:1] = b == 0                                    # image 0 always has an ignored polygon
        cs.append(cover_ref(h, w, shrunk, counts[b], np.zeros(counts[b], bool)))
        cf.append(cover_ref(h, w, full, counts[b], ign))
    th = rng.uniform(0, 2 * math.pi, (n, P, 4))
    rects = np.zeros((n, P, 5, 3), f32)
    rects[:, :, :4, 0], rects[:, :, :4, 1] = np.cos(th), np.sin(th)
    rects[:, :, :4, 2] = rng.uniform(-200, 200, (n, P, 4))
    rects[:, :, 4, 0] = rng.uniform(-0.78, 0.78, (n, P))
    rects[:, :, 4, 1:] = rng.uniform(-5, 5, (n, P, 2))              # documented as 0 and never read
    cs, cf = np.stack(cs), np.stack(cf)
    s = (slice(None), slice(None, None, step), slice(None, None, step))
    owner = ((cs >> 8) & 255)[s].astype(np.int64)
    owner[owner > P] = 0
    ys, xs = np.mgrid[0:h:step, 0:w:step].astype(f32)
    r = rects[np.arange(n)[:, None, None], np.maximum(owner, 1) - 1]            # [n, oh, ow, 5, 3]
    with np.errstate(invalid="ignore"):
        g32 = np.abs((r[..., :4, 0] * xs[None, ..., None] + r[..., :4, 1] * ys[None, ..., None]) + r[..., :4, 2])     # f32, op by op
    assert g32.dtype == f32
    g64 = np.abs(r[..., :4, 0].astype(f64) * xs[None, ..., None] + r[..., :4, 1].astype(f64) * ys[None, ..., None] + r[..., :4, 2])
    geo = np.concatenate([g32, r[..., 4, :1]], axis=-1) * (owner > 0)[..., None].astype(f32)
    return dict(P=P, h=h, w=w, step=step, n=n, cover_score=cs, cover_full=cf, rects=rects, owner=owner, raw_owner=((cs >> 8) & 255)[s],
                score=(owner > 0).astype(f32)[..., None], geo=geo.astype(f32), geo64=g64 * (owner > 0)[..., None],
                mask=(1 - ((cf >> 16) & 1)[s]).astype(f32)[..., None])


for _P in RBOXLAB_P:
    for _s in RBOXLAB_SHAPES:
        _row("rboxlab/%d/%dx%ds%d" % ((_P,) + _s), RBOXLAB, lambda P=_P, s=_s: rboxlab_case(P, *s))
_row("rboxlab/above", RBOXLAB, lambda: rboxlab_case(12, 37, 53, 4, drawn=40))
RBOXLAB_ROWS = [n for n in ROWS if n.startswith("rboxlab/")]


@pytest.mark.parametrize("name", RBOXLAB_ROWS)
def test_rbox_labels(device, name):
    L, _ = _lib()
    c = case(name)
    n, P, h, w, step = c["n"], c["P"], c["h"], c["w"], c["step"]
    oh, ow = _cdiv(h, step), _cdiv(w, step)
    cs, cf, rects = _t(c["cover_score"].view(i32), device), _t(c["cover_full"].view(i32), device), _t(c["rects"], device)
    score, geo, mask = Guard((n, oh, ow, 1), F32, device), Guard((n, oh, ow, 5), F32, device), Guard((n, oh, ow, 1), F32, device)
    guards = (score, geo, mask)
    for what, a in {"n 0": (0, P, h, w, step), "max_polys 0": (n, 0, h, w, step), "max_polys 255": (n, 255, h, w, step), "h 0": (n, P, 0, w, step),
                    "w -1": (n, P, h, -1, step), "step 0": (n, P, h, w, 0), "n 65536": (65536, P, h, w, step), "h 16385": (n, P, 16385, w, step),
                    "w 16385": (n, P, h, 16385, step)}.items():
        _refused(L, "ocr_icdar_rbox_labels", (cs, cf, rects) + a + guards, UNSUPPORTED, guards, what)
    for k in range(6):
        a = [cs, cf, rects, n, P, h, w, step, score, geo, mask]
        a[k if k < 3 else k + 5] = None
        _refused(L, "ocr_icdar_rbox_labels", a, INVALID_ARG, guards, "pointer %d null" % k)
    assert _rc(L, "ocr_icdar_rbox_labels", cs, cf, rects, n, P, h, w, step, score, geo, mask) == OK
    torch.cuda.synchronize()
    _bits_equal(score.np(), c["score"], "score")
    _bits_equal(mask.np(), c["mask"], "mask")
    got = geo.np()
    _bits_equal(got, c["geo"], "geometry against separate f32 multiplies and adds")
    assert (np.abs(got[..., :4] - c["geo64"]) <= 2e-3).all()
    assert (got[c["owner"] == 0].view(i32) == 0).all(), "no owner (or one above max_polys): all zero"
