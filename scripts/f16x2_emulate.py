#!/usr/bin/env python3
"""Host emulation of the f16x2 inference precision (csrc/f16x2_infer.hip), CPU only.

An f32 value v is carried as two IEEE halves, hi = half(v) and lo' = half((v - hi) * 2^11); a product is
xhi*whi + 2^-11 (xhi*wlo' + xlo'*whi), main and correction terms accumulated in f32 apart and joined at the end — the
device's roundings (round-to-nearest-even half conversions, saturation at the largest finite half, f32 accumulation).

  * `split`, `split_matmul`: the helper (tests/test_f16x2_host.py pins its accuracy, and why the 2^11 scaling exists);
  * `table()`: the GEMM table of DESIGN.md section 4 (scaled / unscaled / hi-only vs a plain f32 GEMM, against float64);
  * `whole_net()`: the oracle's whole model_vgg at 64^2 with EVERY convolution's operands split and recombined, f32
    everywhere else, against O.model_vgg(..., mixed=False): L-inf of logits / P(text) / P(link).

    python scripts/f16x2_emulate.py [--out profiles/f16x2_emulation.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LO_SCALE = 2048.0            # 2^11
HALF_MAX = 65504.0
HALF_MIN_NORMAL = 2.0 ** -14


def _half(v, ftz):
    h = np.clip(v, -HALF_MAX, HALF_MAX).astype(np.float16)
    if ftz:                                        # a matrix core that flushes half subnormals on its inputs
        h = np.where(np.abs(h.astype(np.float32)) < HALF_MIN_NORMAL, np.float16(0), h)
    return h


def split(v, scaled=True, ftz=False):
    """f32 array -> (hi, lo) float16 arrays; lo carries the factor 2^11 when `scaled`."""
    v = np.asarray(v, dtype=np.float32)
    hi = _half(v, ftz)
    res = v - hi.astype(np.float32)                # exact in f32
    lo = _half(res * np.float32(LO_SCALE) if scaled else res, ftz)
    return hi, lo


def split_matmul(x, w, scaled=True, ftz=False, correction=True):
    """x [M, K] @ w [K, N] in the split form: half products are exact in f32, sums are numpy's f32 GEMM; main and
    correction accumulators apart, joined at the end.  correction=False: hi*hi only (= an f16 GEMM)."""
    xh, xl = (a.astype(np.float32) for a in split(x, scaled, ftz))
    wh, wl = (a.astype(np.float32) for a in split(w, scaled, ftz))
    main = xh @ wh
    if not correction:
        return main
    corr = xh @ wl + xl @ wh
    return main + corr * np.float32(1.0 / LO_SCALE if scaled else 1.0)


def rel_err(y, ref):
    return float(np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max())


def table_row(x, w):
    ref = x.astype(np.float64) @ w.astype(np.float64)
    return {"f32_gemm": rel_err(x @ w, ref), "split_scaled": rel_err(split_matmul(x, w), ref),
            "split_scaled_ftz": rel_err(split_matmul(x, w, ftz=True), ref),
            "split_unscaled": rel_err(split_matmul(x, w, scaled=False), ref),
            "hi_only": rel_err(split_matmul(x, w, correction=False), ref)}


def operands(kind, K, seed=0, M=512, N=64):
    """The operand distributions of the table (fixed seeds)."""
    rng = np.random.default_rng(seed)
    if kind == "normal":                           # N(0,1) . N(0,1)/sqrt(K)
        x, w = rng.standard_normal((M, K)), rng.standard_normal((K, N)) / np.sqrt(K)
    elif kind == "normal_small_x":                 # the same, x scaled by 2^-16
        x, w = rng.standard_normal((M, K)) * 2.0 ** -16, rng.standard_normal((K, N)) / np.sqrt(K)
    elif kind == "relu_he":
        x, w = np.maximum(rng.standard_normal((M, K)), 0), rng.standard_normal((K, N)) * np.sqrt(2.0 / K)
    elif kind == "image_he":
        x, w = rng.uniform(-150, 150, (M, K)), rng.standard_normal((K, N)) * np.sqrt(2.0 / K)
    elif kind == "wide":                           # per-element magnitudes 10^U(-6,2) . 10^U(-3,0)
        x = rng.standard_normal((M, K)) * 10.0 ** rng.uniform(-6, 2, (M, K))
        w = rng.standard_normal((K, N)) / np.sqrt(K) * 10.0 ** rng.uniform(-3, 0, (K, N))
    else:
        raise ValueError(kind)
    return x.astype(np.float32), w.astype(np.float32)


def table():
    rows = {}
    for kind, K in (("normal", 27), ("normal", 576), ("normal", 4608), ("normal_small_x", 4608), ("relu_he", 4608),
                    ("image_he", 27), ("wide", 4608)):
        rows["%s_K%d" % (kind, K)] = table_row(*operands(kind, K))
    return rows


def whole_net(size=64, n=2, seed=0, ftz=False):
    """O.model_vgg with every convolution in the split form (inference mode, moving statistics randomised so that the
    batch norms are not identities)."""
    import torch
    import torch.nn.functional as F
    from oracle import ocr_oracle as O
    rng = np.random.default_rng(seed)
    p = O.init_model_vgg_params(rng)
    for k in p:
        if k.endswith("moving_mean"):
            p[k] = rng.normal(0, 0.1, p[k].shape).astype(np.float32)
        if k.endswith("moving_variance"):
            p[k] = rng.uniform(0.5, 1.5, p[k].shape).astype(np.float32)
    images, _, _, _ = O.synthetic_batch(rng, n, size)
    tp = O.to_torch_params(p, requires_grad=False)
    with torch.no_grad():
        rpx, rlk, _ = O.model_vgg(torch.from_numpy(images), tp, False, mixed=False)
    plain = O.conv2d

    def t_split(t):
        hi, lo = split(t.numpy(), ftz=ftz)
        return torch.from_numpy(hi.astype(np.float32)), torch.from_numpy(lo.astype(np.float32))

    def conv2d_split(x, w_hwio, stride=1, rate=1, padding="SAME"):
        xh, xl = t_split(x)
        wh, wl = t_split(w_hwio)
        main = plain(xh, wh, stride, rate, padding)
        corr = plain(xh, wl, stride, rate, padding) + plain(xl, wh, stride, rate, padding)
        return main + corr * (1.0 / LO_SCALE)

    O.conv2d = conv2d_split
    try:
        with torch.no_grad():
            px, lk, _ = O.model_vgg(torch.from_numpy(images), tp, False, mixed=False)
    finally:
        O.conv2d = plain
    sm = lambda t: F.softmax(t, -1)
    plk = lambda t: F.softmax(t.reshape(t.shape[:-1] + (8, 2)), -1)
    return {"size": size, "n": n, "half_subnormals_flushed": ftz,
            "pixel_logits_linf": float((px - rpx).abs().max()), "link_logits_linf": float((lk - rlk).abs().max()),
            "p_text_linf": float((sm(px) - sm(rpx)).abs().max()), "p_link_linf": float((plk(lk) - plk(rlk)).abs().max()),
            "logit_range": float(rpx.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"what": "host emulation of the f16x2 precision (scripts/f16x2_emulate.py): error = Linf / max|float64 result|",
           "gemm_table": table(), "model_vgg_64": [whole_net(ftz=False), whole_net(ftz=True)]}
    print(json.dumps(res, indent=1))
    worst = max(max(r["pixel_logits_linf"], r["link_logits_linf"], r["p_text_linf"], r["p_link_linf"])
                for r in res["model_vgg_64"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if worst >= 1e-3:
        sys.exit("emulated model_vgg error %.2e is not below 1e-3" % worst)


if __name__ == "__main__":
    main()
