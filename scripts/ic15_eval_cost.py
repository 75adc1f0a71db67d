#!/usr/bin/env python3
"""What matching a batch costs under the two evaluation protocols: ocr_eval_match_batch (the reference's raster rule, one
workgroup per pair rasterising two quads) against ocr_eval_ic15_match_batch (the official ICDAR-2015 protocol, one thread
per pair clipping two triangles), in one process on the inputs of scripts/link_eval_cost.py: n = 8 images of 1280 x 768,
its painted maps through pixellink_fn.detect_device and ocr_eval_collect (192 detections each, a jittered 16 x 12 grid of
rectangles) and 8 ground truths each (a handful of the detections moved by a few pixels, every third one don't-care),
max_d = 512.

    python scripts/ic15_eval_cost.py [--repeats 20] [--warmup 3] [--out profiles/ic15_eval.json]

Each figure is the median of --repeats runs between a pair of HIP events after the warm-up, the two matchers in turn.  The
yardstick is the raster matcher in the same process.  No bar was set: the file records the two medians and their ratio,
with the fingerprint of the kernel sources they were measured on.  The two protocols count different things, so their
records are written side by side and not compared."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ic15_eval.json"))
    args = ap.parse_args()
    from link_eval_cost import painted_maps
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import bboxes, metrics, pixellink_fn as P
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    n, max_d = args.batch, 512
    rng = np.random.default_rng(9)
    # the detections of scripts/link_eval_cost.py: its painted maps through the device chain up to the ordered list
    h4, w4 = args.height // 4, args.width // 4
    ps_d = torch.from_numpy(painted_maps(rng, n, h4, w4, cols=16, rows=12)).to(dev)
    link_d = torch.full((8, n, h4, w4), 0.95, dtype=torch.float32, device=dev)
    merged, keep, n_keep, passed, _ = P.detect_device(ps_d, link_d, 0.8, 0.9, 10, args.width / float(w4), args.height / float(h4),
                                                      max_comps=1024, graph=g)
    dets_d = torch.zeros((n, max_d, 4, 2), dtype=torch.int32, device=dev)
    det_score = torch.empty((n, max_d), dtype=torch.float32, device=dev)
    nd_d, nd_total = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    ops.eval_collect(merged, keep, n_keep, passed, torch.ones((n, 2), dtype=torch.float32, device=dev), dets_d, det_score, nd_d, nd_total)
    dets, counts = dets_d.cpu().numpy(), nd_d.cpu().numpy()
    # ground truths: a few of each image's boxes moved by some pixels, every third one don't-care
    gts_h = [np.clip(dets[i, :c][:: max(1, c // args.gts)][:args.gts] + rng.integers(-3, 4, (1, 1, 2)), 0, None).astype(np.int32)
             for i, c in enumerate(counts)]
    max_g = max(max(len(q) for q in gts_h), 1)
    gts, ng, ign = np.zeros((n, max_g, 4, 2), np.int32), np.zeros(n, np.int32), np.zeros((n, max_g), np.uint8)
    for i, q in enumerate(gts_h):
        gts[i, :len(q)], ng[i], ign[i, :len(q)] = q, len(q), np.arange(len(q)) % 3 == 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gts_d, ng_d, ign_d = up(gts), up(ng), up(ign)
    k = [int(c) for c in counts]
    side = 2 * max(args.height, args.width) + 10
    acc = {name: metrics.DeviceTpFp(g) for name in ("raster", "icdar15")}

    def raster():
        bboxes.bboxes_matching_batch(dets_d, nd_d, gts_d, ng_d, ign_d, 0.5, record=acc["raster"].record, graph=g, mask_hw=(side, side))

    def icdar15():
        bboxes.ic15_matching_batch(dets_d, nd_d, gts_d, ng_d, ign_d, 0.5, 0.5, record=acc["icdar15"].record, graph=g)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    for _ in range(args.warmup):
        raster()
        icdar15()
    torch.cuda.synchronize()
    times = {"raster": [], "icdar15": []}
    records = {}
    for _ in range(args.repeats):
        for name, fn in (("raster", raster), ("icdar15", icdar15)):
            acc[name].reset()
            times[name].append(timed(fn))
            records[name] = list(acc[name].value())
    med = statistics.median
    res = {
        "what": "matching %d images of %d x %d with %s detections and %d ground truths each (max_d %d): ocr_eval_match_batch "
                "(raster rule) and ocr_eval_ic15_match_batch (ICDAR-2015 polygon rule) in turn in one process, each between a "
                "pair of HIP events; medians of %d runs after %d warm-up runs" % (n, args.width, args.height, k, max_g, max_d,
                                                                                 args.repeats, args.warmup),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats,
        "detections_per_image": k, "max_d": max_d, "max_g": max_g,
        "raster_record_gt_tp_fp_det": records["raster"],
        "icdar15_record_caregt_matched_fp_det": records["icdar15"],
        "eval_match_ms": round(med(times["raster"]), 4),
        "eval_match_ms_min_max": [round(min(times["raster"]), 4), round(max(times["raster"]), 4)],
        "eval_ic15_match_ms": round(med(times["icdar15"]), 4),
        "eval_ic15_match_ms_min_max": [round(min(times["icdar15"]), 4), round(max(times["icdar15"]), 4)],
        "raster_over_icdar15": round(med(times["raster"]) / med(times["icdar15"]), 2),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
