#!/usr/bin/env python3
"""What the score-threshold sweep adds to an evaluation pass: the chain after the forward pass (pixellink_fn.detect_device
-> ocr_eval_collect -> matching) without a sweep, as it ran before the sweep existed, and with T = 16 thresholds (the
curve entry and the AP pool rows behind the same matching), under both protocols, in one process on the inputs of
scripts/link_eval_cost.py and scripts/ic15_eval_cost.py: n = 8 images of 1280 x 768, 192 detections and 8 ground truths
each, max_d = 512.  Also the matcher and the curve entry alone — what the sweep replaces is T runs of the matcher — and
ocr_eval_ap alone on a pool of 500 images x max_d (the 8 images' pool rows repeated).

    python scripts/eval_sweep_cost.py [--repeats 20] [--warmup 3] [--out profiles/eval_sweep.json]

Each figure is the median of --repeats runs between a pair of HIP events after the warm-up, the variants in turn.  No bar
was set: the file records the medians and their ratios, with the fingerprint of the kernel sources they were measured on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--gts", type=int, default=8, help="ground truths per image")
    ap.add_argument("--thresholds", type=int, default=16)
    ap.add_argument("--pool_images", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_sweep.json"))
    args = ap.parse_args()
    from link_eval_cost import painted_maps
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import bboxes, metrics, pixellink_fn as P
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    n, max_d, T = args.batch, 512, args.thresholds
    rng = np.random.default_rng(9)
    h4, w4 = args.height // 4, args.width // 4
    ps_d = torch.from_numpy(painted_maps(rng, n, h4, w4, cols=16, rows=12)).to(dev)
    link_d = torch.full((8, n, h4, w4), 0.95, dtype=torch.float32, device=dev)
    ones = torch.ones((n, 2), dtype=torch.float32, device=dev)
    dets_d = torch.zeros((n, max_d, 4, 2), dtype=torch.int32, device=dev)
    det_score = torch.empty((n, max_d), dtype=torch.float32, device=dev)
    nd_d, nd_total = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)

    def front():
        merged, keep, n_keep, passed, _ = P.detect_device(ps_d, link_d, 0.8, 0.9, 10, args.width / float(w4), args.height / float(h4),
                                                          max_comps=1024, graph=g)
        ops.eval_collect(merged, keep, n_keep, passed, ones, dets_d, det_score, nd_d, nd_total)
    front()
    dets, counts = dets_d.cpu().numpy(), nd_d.cpu().numpy()
    gts_h = [np.clip(dets[i, :c][:: max(1, c // args.gts)][:args.gts] + rng.integers(-3, 4, (1, 1, 2)), 0, None).astype(np.int32)
             for i, c in enumerate(counts)]
    max_g = max(max(len(q) for q in gts_h), 1)
    gts, ng, ign = np.zeros((n, max_g, 4, 2), np.int32), np.zeros(n, np.int32), np.zeros((n, max_g), np.uint8)
    for i, q in enumerate(gts_h):
        gts[i, :len(q)], ng[i], ign[i, :len(q)] = q, len(q), np.arange(len(q)) % 3 == 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gts_d, ng_d, ign_d = up(gts), up(ng), up(ign)
    side = 2 * max(args.height, args.width) + 10
    scores = det_score.cpu().numpy()
    live = np.concatenate([scores[i, :c] for i, c in enumerate(counts)])
    thresholds = [float(v) for v in np.linspace(float(live.min()), float(live.max()), T)]
    acc = metrics.DeviceTpFp(g)
    curve = metrics.DeviceCurve(thresholds, n, max_d, g)
    out = {}

    def match(protocol):
        if protocol == "raster":
            out["m"] = bboxes.bboxes_matching_batch(dets_d, nd_d, gts_d, ng_d, ign_d, 0.5, record=acc.record, graph=g, mask_hw=(side, side))
        else:
            out["m"] = bboxes.ic15_matching_batch(dets_d, nd_d, gts_d, ng_d, ign_d, 0.5, 0.5, record=acc.record, graph=g)

    def count(protocol):
        curve.seq = 0
        if protocol == "raster":
            curve.add_raster(out["m"][0], out["m"][1], det_score, nd_d, ng_d, ign_d)
        else:
            curve.add_ic15(out["m"][0], out["m"][1], det_score, nd_d, ng_d)

    def chain(protocol, sweep):
        front()
        match(protocol)
        if sweep:
            count(protocol)
    # the AP pool of --pool_images images: the rows of the last counted batch, repeated
    match("icdar15")
    count("icdar15")
    reps = (args.pool_images + n - 1) // n
    big = [t.repeat((reps,) + (1,) * (t.dim() - 1))[:args.pool_images].contiguous() for t in (curve.pool_score, curve.pool_cum, curve.pool_nd)]
    ap_out = torch.zeros((1,), dtype=torch.float64, device=dev)
    big_record = torch.tensor([int(ng.sum()) * reps, 0, 0, 0], dtype=torch.int64, device=dev)
    variants = {"ap_pool": lambda: ops.eval_ap(big[0], big[1], big[2], big_record, ap_out, g.workspace())}
    for protocol in ("raster", "icdar15"):
        variants["chain_%s" % protocol] = lambda p=protocol: chain(p, False)
        variants["chain_%s_sweep" % protocol] = lambda p=protocol: chain(p, True)
        variants["match_%s" % protocol] = lambda p=protocol: match(p)
        variants["curve_%s" % protocol] = lambda p=protocol: count(p)      # (after match_<protocol>: its outputs are in place)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    order = ["chain_raster", "chain_raster_sweep", "match_raster", "curve_raster", "chain_icdar15", "chain_icdar15_sweep",
             "match_icdar15", "curve_icdar15", "ap_pool"]
    for _ in range(args.warmup):
        for name in order:
            variants[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in order}
    for _ in range(args.repeats):
        for name in order:
            times[name].append(timed(variants[name]))
    med = {name: statistics.median(v) for name, v in times.items()}
    res = {
        "what": "the chain after the forward pass (detect_device -> ocr_eval_collect -> matching) on %d images of %d x %d with %s "
                "detections and %d ground truths each (max_d %d), without a sweep and with T = %d thresholds (curve entry + AP pool "
                "rows), the matcher and the curve entry alone, and ocr_eval_ap on a pool of %d images x %d; variants in turn in "
                "one process, each between a pair of HIP events; medians of %d runs after %d warm-up runs"
                % (n, args.width, args.height, [int(c) for c in counts], max_g, max_d, T, args.pool_images, max_d, args.repeats,
                   args.warmup),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats, "thresholds": T, "max_d": max_d, "max_g": max_g, "pool_images": args.pool_images,
        "ap_of_the_pool": float(ap_out.item()),
    }
    for name in order:
        res[name + "_ms"] = round(med[name], 4)
        res[name + "_ms_min_max"] = [round(min(times[name]), 4), round(max(times[name]), 4)]
    for protocol in ("raster", "icdar15"):
        res["chain_%s_sweep_over_plain" % protocol] = round(med["chain_%s_sweep" % protocol] / med["chain_%s" % protocol], 3)
        res["T_matcher_runs_over_curve_%s" % protocol] = round(T * med["match_%s" % protocol] / med["curve_%s" % protocol], 1)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
