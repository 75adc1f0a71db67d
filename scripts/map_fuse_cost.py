#!/usr/bin/env python3
"""What score-map fusion for the link geometry costs (csrc/map_fuse.hip).

    python scripts/map_fuse_cost.py [--repeats 20] [--warmup 3] [--out profiles/map_fuse.json]

(a) One ocr_link_map_accumulate launch onto a 192 x 320 fusion grid, batch 8 (the 1/4 maps of the 768 x 1280 eval size),
    between a pair of HIP events: from the identity size, from 1/2 x (96 x 160) and from 2 x (384 x 640) logits, storing
    (first) and adding, un-flipped and flipped.  Beside the identity launch, timed alternately in the same process, what
    it replaces at that size in the single-scale chain: ocr_softmax_pairs + ocr_link_softmax_stack + the [..., 1] copy.
(b) One `LinkEvaluator` pass over a synthetic directory (8 images of 256 x 256, eval size 256, planted words, a stub
    forward that returns prepared device logits, so the figure is the post-processing alone) on the host clock, its one
    read of the device included: single-scale, map_scales=[0.5, 1, 2], and flip=True.

Every figure is the median of --repeats runs after --warmup, with the minimum and maximum as its spread; no bar was set:
the file records the numbers, their ratios and the fingerprint of the kernel sources they were measured on."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def accumulate_rows(g, args):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    dev, n, hf, wf = g.device, args.batch, 192, 320
    gen = torch.Generator(device="cpu").manual_seed(0)
    logits = {}
    for name, (hs, ws) in (("identity", (hf, wf)), ("half", (hf // 2, wf // 2)), ("double", (2 * hf, 2 * wf))):
        logits[name] = (torch.randn((n, hs, ws, 2), generator=gen).to(dev), torch.randn((n, hs, ws, 16), generator=gen).to(dev))
    acc = torch.zeros((9, n, hf, wf), dtype=torch.float32, device=dev)
    px, lk = logits["identity"]

    def replaced():                            # the single-scale chain's three launches (LinkEvaluator._chain)
        ps = P.pixel_scores(px, graph=g)[..., 1].contiguous()
        ls = P.link_scores(lk, graph=g)
        return ps, ls

    def fused_identity():
        ops.link_map_accumulate(px, lk, False, 1.0, True, acc)
    event_ms(replaced, 0, args.warmup)
    event_ms(fused_identity, 0, args.warmup)
    new_ms, old_ms = [], []
    for _ in range(args.repeats):              # alternately, so that both see the same clocks
        new_ms += event_ms(fused_identity, 1, 0)
        old_ms += event_ms(replaced, 1, 0)
    out = {"grid": [hf, wf], "batch": n, "identity_first": summary(new_ms), "replaced_three_launches": summary(old_ms)}
    out["identity_over_replaced"] = out["identity_first"]["median_ms"] / out["replaced_three_launches"]["median_ms"]
    print("identity accumulate %.4f ms, softmax_pairs + link_softmax_stack + copy %.4f ms, ratio %.2f" % (
        out["identity_first"]["median_ms"], out["replaced_three_launches"]["median_ms"], out["identity_over_replaced"]), flush=True)
    rows = []
    for name in ("identity", "half", "double"):
        a, b = logits[name]
        for flip in (False, True):
            for first in (True, False):
                ms = event_ms(lambda: ops.link_map_accumulate(a, b, flip, 0.25, first, acc), args.repeats, args.warmup)
                # logits read once, the accumulator written (and, when adding, read) once
                nbytes = a.numel() * 4 + b.numel() * 4 + acc.numel() * 4 * (1 if first else 2)
                row = dict(summary(ms), source=name, source_hw=list(a.shape[1:3]), flip=flip, first=first, bytes=nbytes)
                row["gb_per_s"] = nbytes / (row["median_ms"] * 1e-3) / 1e9
                rows.append(row)
                print("%-8s flip=%d first=%d: %.4f ms (%.4f .. %.4f), %.0f GB/s" % (
                    name, flip, first, row["median_ms"], row["min_ms"], row["max_ms"], row["gb_per_s"]), flush=True)
    out["launches"] = rows
    return out


def evaluator_rows(g, args):
    from tensorflow_ocr_amd import evaluate
    dev, side = g.device, 256
    rng = np.random.default_rng(3)
    words = [(16 + 8 * k, 12 + 30 * k, 150 + 8 * k, 12 + 30 * k + 6 + 3 * k) for k in range(8)]     # heights 6 .. 27

    def logits(size):                          # every word, at its place at this size
        q, s = size // 4, size / float(side)
        ys, xs = np.mgrid[0:q, 0:q]
        cx, cy = 4.0 * xs, 4.0 * ys
        inside = np.zeros((q, q), bool)
        for x0, y0, x1, y1 in words:
            inside |= (cx >= x0 * s) & (cx <= x1 * s) & (cy >= y0 * s) & (cy <= y1 * s)
        px = np.zeros((q, q, 2), np.float32)
        px[..., 1] = np.where(inside, 4.0, -4.0)
        lk = np.zeros((q, q, 16), np.float32)
        lk[..., 1::2] = 5.0
        up = lambda a: torch.from_numpy(np.stack([a] * args.batch)).to(dev)
        return up(px), up(lk)
    prepared = {size: logits(size) for size in (128, 256, 512)}
    forward = lambda x: prepared[x.shape[1]]   # the mirrored pass gets the same logits: the cost does not depend on them
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.batch):
            np.save(os.path.join(tmp, "img_%d.npy" % i), rng.integers(0, 256, (side, side, 3)).astype(np.uint8))
            with open(os.path.join(tmp, "gt_img_%d.txt" % i), "w") as f:
                for x0, y0, x1, y1 in words:
                    f.write("%d,%d,%d,%d,%d,%d,%d,%d,text\r\n" % (x0, y0, x1, y0, x1, y1, x0, y1))

        def timed(**kw):
            ev = evaluate.LinkEvaluator(g, forward, tmp, batch_size=args.batch, eval_image_height=side, eval_image_width=side, **kw)
            ms = []
            for it in range(args.warmup + args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ev.run()
                if it >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return dict(summary(ms), result={k: res[k] for k in ("tp", "fp", "num_gt", "num_det")})
        out["single_scale"] = timed()
        out["map_scales_0.5_1_2"] = timed(map_scales=[0.5, 1, 2])
        out["flip"] = timed(flip=True)
    for k in ("map_scales_0.5_1_2", "flip"):
        out[k + "_over_single"] = out[k]["median_ms"] / out["single_scale"]["median_ms"]
    out["what"] = ("host clock per LinkEvaluator pass (uploads, resizes, softmaxes or fusion, link decode, boxes, matching, one "
                   "device read); %d images of %d x %d, 8 planted words, stub forward returning prepared logits" % (args.batch, side, side))
    print(json.dumps({k: v for k, v in out.items() if "over" in k}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_fuse.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib
    from tensorflow_ocr_amd.graph import Graph
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    record = {"script": "scripts/map_fuse_cost.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "hip": torch.version.hip, "csrc_fingerprint": _lib.csrc_fingerprint(), "date": time.strftime("%Y-%m-%d"),
              "repeats": args.repeats, "warmup": args.warmup,
              "timing": "HIP events around the launches, the new launch and the three it replaces alternately in one process; medians",
              "accumulate": accumulate_rows(g, args), "evaluator": evaluator_rows(g, args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
