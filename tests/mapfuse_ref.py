"""Not a test: the NumPy references of score-map fusion (include/ocr_map_fuse.h: ocr_link_map_accumulate) that
tests/test_map_fuse_host.py pins by hand and tests/test_gpu_map_fuse.py compares the device with.

`accumulate_f32` is the header's rule in float32, operation by operation; it takes the PROBABILITIES at the source pixels
(on the GPU: the device's own, from ocr_softmax_pairs / ocr_link_softmax_stack), so that the comparison is bit for bit
whatever expf rounds to.  `accumulate_f64` is an independent float64 version that starts from the logits; `f64_bound`
is the per-element distance the float32 rule may have from it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24                                   # float32 unit roundoff


# ------------------------------------------------------------------------------------------------ the direction table
def parse_tables(name):
    """(dx, dy) from the `kDx[8] = {...}` / `kDy[8] = {...}` initialisers of csrc/<name>"""
    txt = open(os.path.join(ROOT, "tensorflow_ocr_amd", "csrc", name)).read()
    out = []
    for var in ("kDx", "kDy"):
        m = re.search(r"\bint %s\[8\]\s*=\s*\{([^}]*)\}" % var, txt)
        assert m, (name, var)
        vals = [int(v) for v in m.group(1).split(",")]
        assert len(vals) == 8, (name, var, vals)
        out.append(vals)
    return out[0], out[1]


def mirror_perm(dx, dy):
    """perm[d] = the direction with the opposite dx and the same dy"""
    perm = []
    for d in range(8):
        hits = [e for e in range(8) if dx[e] == -dx[d] and dy[e] == dy[d]]
        assert len(hits) == 1, (d, hits)
        perm.append(hits[0])
    return perm


def decode_perm():
    return mirror_perm(*parse_tables("decode.hip"))


# ------------------------------------------------------------------------------------------------ float32, by the rule
def axis_taps(size_out, size_src):
    """-> (i0 int64 [size_out], i1 int64 [size_out], t float32 [size_out]), every operation in float32"""
    r = f32(size_src) / f32(size_out)
    i = np.arange(size_out, dtype=f32)
    s = (i + f32(0.5)) * r - f32(0.5)
    f0 = np.floor(s)
    t = (s - f0).astype(f32)
    lo = f0 < f32(0)
    hi = f0 >= f32(size_src - 1)
    i0 = np.where(lo, 0, np.where(hi, size_src - 1, f0)).astype(np.int64)
    t = np.where(lo | hi, f32(0), t).astype(f32)
    i1 = np.minimum(i0 + 1, size_src - 1)
    return i0, i1, t


def plane_order(flip, perm):
    """source plane read by each of the nine output planes"""
    return [0] + [1 + (perm[d] if flip else d) for d in range(8)]


def sample_f32(P, hf, wf, flip=False, perm=None):
    """P float32 [9,n,hs,ws], the probabilities of ONE pass in the pass's own layout (plane 1 + d = pair d, column c = the
    pass's column c) -> v float32 [9,n,hf,wf]"""
    P = np.asarray(P, f32)
    _, n, hs, ws = P.shape
    if flip:
        P = P[plane_order(True, perm or decode_perm())]
    y0, y1, ty = axis_taps(hf, hs)
    x0, x1, tx = axis_taps(wf, ws)
    c0, c1 = (ws - 1 - x0, ws - 1 - x1) if flip else (x0, x1)
    one = f32(1)
    with np.errstate(invalid="ignore"):
        def row(yy):
            a = P[:, :, yy][:, :, :, c0]
            b = P[:, :, yy][:, :, :, c1]
            blend = (a * (one - tx)).astype(f32) + (b * tx).astype(f32)
            return np.where(tx == 0, a, blend).astype(f32)
        top, bot = row(y0), row(y1)
        ty_ = ty[:, None]
        blend = (top * (one - ty_)).astype(f32) + (bot * ty_).astype(f32)
        return np.where(ty_ == 0, top, blend).astype(f32)


def accumulate_f32(P, hf, wf, flip, weight, first, acc=None, perm=None):
    """one ocr_link_map_accumulate call on tap probabilities -> the new accumulator float32 [9,n,hf,wf]"""
    v = sample_f32(P, hf, wf, flip, perm)
    with np.errstate(invalid="ignore"):
        wv = (f32(weight) * v).astype(f32)
        return wv if first else (np.asarray(acc, f32) + wv).astype(f32)


def stack_probs(pixel_probs, link_probs):
    """softmax outputs in the layouts of ocr_softmax_pairs [n,h,w,2] and ocr_link_softmax_stack [8,n,h,w,2] -> [9,n,h,w]"""
    return np.concatenate([np.asarray(pixel_probs, f32)[None, ..., 1], np.asarray(link_probs, f32)[..., 1]]).astype(f32)


# ------------------------------------------------------------------------------------------------ float64, from logits
def accumulate_f64(pixel_logits, link_logits, hf, wf, flip, weight, first, acc=None, perm=None):
    """the same pass in float64 from LOGITS [n,hs,ws,2] / [n,hs,ws,16], written differently: sigmoid of the logit
    difference, the mirrored source built explicitly, coordinates in float64, all four taps always blended"""
    px = np.asarray(pixel_logits, np.float64)
    lk = np.asarray(link_logits, np.float64)
    n, hs, ws, _ = px.shape
    sig = lambda a, b: 1.0 / (1.0 + np.exp(a - b))                       # softmax index 1 of the pair (a, b)
    P = np.stack([sig(px[..., 0], px[..., 1])] + [sig(lk[..., 2 * d], lk[..., 2 * d + 1]) for d in range(8)])
    if flip:                                                                # un-mirror the pass: columns and directions
        perm = perm or decode_perm()
        P = P[[0] + [1 + perm[d] for d in range(8)]][..., ::-1]

    def taps(size_out, size_src):
        s = (np.arange(size_out) + 0.5) * (size_src / float(size_out)) - 0.5
        s = np.clip(s, 0.0, size_src - 1.0)
        i0 = np.minimum(np.floor(s).astype(np.int64), size_src - 1)
        return i0, np.minimum(i0 + 1, size_src - 1), s - i0
    y0, y1, ty = taps(hf, hs)
    x0, x1, tx = taps(wf, ws)
    ty = ty[:, None]
    g = lambda yy, xx: P[:, :, yy][:, :, :, xx]
    v = (g(y0, x0) * (1 - tx) + g(y0, x1) * tx) * (1 - ty) + (g(y1, x0) * (1 - tx) + g(y1, x1) * tx) * ty
    return weight * v if first else np.asarray(acc, np.float64) + weight * v


def f64_bound(max_logit_gap, hs, ws, passes):
    """What one element of the float32 accumulator may differ from `accumulate_f64` by, from the operation count (values
    and weights in [0, 1], the weights summing to at most 1 + passes * U):
      a tap: a - mx rounds once and exp multiplies that into a relative error of |a - b| * U; expf and the division are
        faithful to 1 ulp = 2 U each at worst, the sum rounds once, and p's sensitivity to the relative error of either
        exponential is p (1 - p) <= 1/4: below (|a - b| + 8) * U;
      the sample coordinate: i + 0.5 exact, r and the product round once each, - 0.5 once more: |ds| <= 3 U * (s + 1) <=
        3 U * (size + 1) per axis, and the blend moves by at most |ds| times a tap difference <= 1 (a tap pair that
        changes at an integer s changes continuously);
      the two blends: 1 - t, two products and a sum each: 4 U per level, 8 U;
      the weighting: one product and one add per pass: 2 U each."""
    return ((max_logit_gap + 8.0) + 3.0 * (hs + 1) + 3.0 * (ws + 1) + 8.0 + 2.0 * passes) * U
