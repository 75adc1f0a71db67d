#!/usr/bin/env python3
"""What the cross-scale fusion of multi-scale RBOX inference costs (csrc/multiscale.hip).

    python scripts/multiscale_cost.py [--repeats 20] [--warmup 3] [--out profiles/multiscale.json]

1. The append + fuse chain — zeroing the counters, three ocr_ms_pool_append calls (one per scale) and one ocr_quad_fuse —
   between a pair of HIP events, for a batch of 8 images at 256, 1024 and 4096 pooled quads per image (the clustered
   rotated rectangles of tests/ms_ref.cluster_case), in both modes; and, in the same process and on the same lists,
   ocr_lanms (unchanged code: the yardstick — the new NMS runs a subset of its phases plus the owner pass and, in mode 1,
   the vote).  The two are timed alternately, the medians and their ratio are recorded.
2. One `Evaluator(scales=[0.5, 1, 2])` pass over a synthetic directory (8 images of 256 x 256, planted words, a stub
   forward that returns prepared device maps, so the figure is the post-processing alone) on the host clock, its one read
   of the device included, beside the sum of three single-scale passes over the same images stored at the three sizes.

Every figure is the median of --repeats runs after --warmup; no bar was set: the file records the numbers, their ratios and
the fingerprint of the kernel sources they were measured on."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def fusion_rows(g, args):
    import ms_ref as M
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.tool import lanms
    dev, n = g.device, args.batch
    rows = []
    for P in (256, 1024, 4096):
        cases = [M.cluster_case(P, 500 + 10 * P + i) for i in range(n)]
        pool_h = np.stack([c[0] for c in cases])
        scale_h = np.stack([c[1] for c in cases])
        per_scale = []                         # each scale's rows as a LANMS-shaped list: merged, identity keep, count, mean
        for s in range(3):
            cnt = (scale_h == s).sum(axis=1).astype(np.int32)
            merged = np.zeros((n, P, 9), np.float32)
            for i in range(n):
                merged[i, :cnt[i]] = pool_h[i][scale_h[i] == s]
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            per_scale.append((up(merged), up(np.tile(np.arange(P, dtype=np.int32), (n, 1))), up(cnt),
                              up(merged[..., 8].copy())))
        ratio = torch.ones((n, 2), dtype=torch.float32, device=dev)
        pool = torch.empty((n, P, 9), dtype=torch.float32, device=dev)
        pool_scale = torch.empty((n, P), dtype=torch.int32, device=dev)
        counters = torch.zeros((3, n), dtype=torch.int32, device=dev)
        fused, keep, owner = torch.empty_like(pool), torch.empty_like(pool_scale), torch.empty_like(pool_scale)
        n_keep = torch.empty((n,), dtype=torch.int32, device=dev)
        boxes, counts = torch.from_numpy(pool_h).to(dev), torch.full((n,), P, dtype=torch.int32, device=dev)

        def chain(mode):
            counters.zero_()
            for s, (merged, kp, cnt, mean) in enumerate(per_scale):
                ops.ms_pool_append(merged, kp, cnt, None, mean, ratio, s, pool, pool_scale, counters[0], counters[1], counters[2])
            ops.quad_fuse(pool, counters[0], 0.2, mode, fused, keep, n_keep, owner, g.workspace())

        def yardstick():
            lanms.lanms_batch(boxes, counts, 0.2, graph=g)
        for mode in ("nms", "vote"):
            new_ms, old_ms = [], []
            event_ms(lambda: chain(mode), 0, args.warmup)
            event_ms(yardstick, 0, args.warmup)
            for _ in range(args.repeats):       # alternately, so that both see the same clocks
                new_ms += event_ms(lambda: chain(mode), 1, 0)
                old_ms += event_ms(yardstick, 1, 0)
            torch.cuda.synchronize()
            assert counters[1].tolist() == [P] * n and counters[2].sum().item() == 0
            row = {"pooled_per_image": P, "batch": n, "mode": mode, "kept_per_image": n_keep.tolist(),
                   "append_fuse": summary(new_ms), "ocr_lanms_same_lists": summary(old_ms)}
            row["ratio_to_lanms"] = row["append_fuse"]["median_ms"] / row["ocr_lanms_same_lists"]["median_ms"]
            rows.append(row)
            print("P=%d %s: append+fuse %.3f ms, ocr_lanms %.3f ms, ratio %.2f" % (
                P, mode, row["append_fuse"]["median_ms"], row["ocr_lanms_same_lists"]["median_ms"], row["ratio_to_lanms"]), flush=True)
    return rows


def evaluator_rows(g, args):
    from tensorflow_ocr_amd import evaluate
    dev, side, scales = g.device, 256, [0.5, 1, 2]
    rng = np.random.default_rng(3)
    words = [(16 + 8 * k, 12 + 30 * k, 150 + 8 * k, 12 + 30 * k + 6 + 3 * k) for k in range(8)]     # heights 6 .. 27

    def maps(size):                            # every word, at its place at this size (angle 0)
        q, s = size // 4, size / float(side)
        score, geo = np.zeros((q, q, 1), np.float32), np.zeros((q, q, 5), np.float32)
        ys, xs = np.mgrid[0:q, 0:q]
        px, py = 4.0 * xs, 4.0 * ys
        for x0, y0, x1, y1 in words:
            x0, y0, x1, y1 = x0 * s, y0 * s, x1 * s, y1 * s
            inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
            d = np.stack([py - y0, x1 - px, y1 - py, px - x0, np.zeros_like(px)], axis=-1)
            score[inside, 0] = 1.0
            geo[inside] = d[inside].astype(np.float32)
        return score, geo
    prepared = {}
    for size in (128, 256, 512):
        sc, ge = maps(size)
        prepared[size] = (torch.from_numpy(np.stack([sc] * args.batch)).to(dev), torch.from_numpy(np.stack([ge] * args.batch)).to(dev))
    forward = lambda x: prepared[x.shape[1]]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for size in (128, 256, 512):
            d = os.path.join(tmp, str(size))
            os.makedirs(d)
            s = size / float(side)
            for i in range(args.batch):
                np.save(os.path.join(d, "img_%d.npy" % i), rng.integers(0, 256, (size, size, 3)).astype(np.uint8))
                with open(os.path.join(d, "gt_img_%d.txt" % i), "w") as f:
                    for x0, y0, x1, y1 in words:
                        f.write("%d,%d,%d,%d,%d,%d,%d,%d,text\r\n" % tuple(int(v * s) for v in (x0, y0, x1, y0, x1, y1, x0, y1)))
            dirs[size] = d

        def timed(ev):
            ms = []
            for it in range(args.warmup + args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ev.run()
                if it >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return summary(ms), res
        for fuse in ("nms", "vote"):
            s, res = timed(evaluate.Evaluator(g, forward, dirs[side], batch_size=args.batch, scales=scales, fuse=fuse))
            out["multiscale_" + fuse] = dict(s, result={k: res[k] for k in ("tp", "fp", "num_gt", "num_det")})
        singles = {}
        for size in (128, 256, 512):
            s, res = timed(evaluate.Evaluator(g, forward, dirs[size], batch_size=args.batch))
            singles[str(size)] = dict(s, result={k: res[k] for k in ("tp", "fp", "num_gt", "num_det")})
        out["single_scale_passes"] = singles
        out["single_scale_sum_median_ms"] = sum(v["median_ms"] for v in singles.values())
        for fuse in ("nms", "vote"):
            out["multiscale_%s_over_single_sum" % fuse] = out["multiscale_" + fuse]["median_ms"] / out["single_scale_sum_median_ms"]
    out["what"] = ("host clock per Evaluator pass (uploads, resizes, decode, LANMS, mean scores, fusion, matching, one device read); "
                   "%d images of %d x %d, 8 planted words, stub forward returning prepared maps" % (args.batch, side, side))
    print(json.dumps({k: v for k, v in out.items() if "over" in k or "sum" in k}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiscale.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib
    from tensorflow_ocr_amd.graph import Graph
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    record = {"script": "scripts/multiscale_cost.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "hip": torch.version.hip, "csrc_fingerprint": _lib.csrc_fingerprint(), "date": time.strftime("%Y-%m-%d"),
              "repeats": args.repeats, "warmup": args.warmup, "iou_thresh": 0.2,
              "timing": "HIP events around the launches of one chain, new chain and ocr_lanms alternately in one process; medians",
              "fusion": fusion_rows(g, args), "evaluator": evaluator_rows(g, args)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
