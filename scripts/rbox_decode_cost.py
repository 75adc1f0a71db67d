#!/usr/bin/env python3
"""What the RBOX post-processing costs on the device: tool/rbox.decode (three launches of csrc/rbox.hip) and
tool/rbox.detect (decode + locality-aware NMS + the single host read) at n = 16 maps of 256 x 256 with about 10 % of
the pixels above the threshold (synthetic.rbox_labels at 1024 x 1024, two rectangles per image whose pixels score
uniformly in [0.72, 1), per-pixel noise on the geometry).

    python scripts/rbox_decode_cost.py [--repeats 20] [--warmup 3] [--out profiles/rbox_decode.json]

Every figure is the median of repeated runs inside one process after the warm-up: decode and decode + LANMS between a
pair of HIP events each, detect on the host clock (it ends in the synchronising read of the kept quads).  The result is
written with the fingerprint of the kernel sources it was measured on."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    """ms of `fn()` between a pair of events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbox_decode.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import lanms, rbox
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    rng = np.random.default_rng(7)
    label, geo, _ = synthetic.rbox_labels(args.batch, args.size, rng, rects=2)
    score = (label[..., 0] * rng.uniform(0.72, 1.0, label.shape[:3])).astype(np.float32)   # 5 in 7 of a rectangle's pixels pass 0.8
    geo[..., :4] += (label * rng.uniform(-1.5, 1.5, geo[..., :4].shape)).astype(np.float32)
    geo[..., 4] += (label[..., 0] * rng.uniform(-0.02, 0.02, label.shape[:3])).astype(np.float32)
    sd, gd = torch.from_numpy(score).to(dev), torch.from_numpy(geo).to(dev)
    positives = (score > np.float32(0.8)).sum(axis=(1, 2))
    max_k = min(int(-(-int(positives.max()) // 1024) * 1024), rbox.LANMS_MAX_K)

    def decode():
        return rbox.decode(sd, gd, max_k=max_k, graph=g)

    def decode_lanms():
        boxes, counts, _ = decode()
        return lanms.lanms_batch(boxes, counts, 0.2, graph=g)

    def detect():
        t0 = time.perf_counter()
        kept = rbox.detect(sd, gd, max_k=max_k, graph=g)
        return (time.perf_counter() - t0) * 1e3, kept
    for _ in range(args.warmup):
        decode_lanms()
        kept = detect()[1]
    torch.cuda.synchronize()
    t_dec = [timed(decode) for _ in range(args.repeats)]
    t_both = [timed(decode_lanms) for _ in range(args.repeats)]
    t_det = [detect()[0] for _ in range(args.repeats)]
    med = statistics.median
    res = {
        "what": "tool/rbox.decode and tool/rbox.detect (decode + ocr_lanms + host read) on %d maps of %d x %d, medians of "
                "%d runs in one process after %d warm-up runs" % (args.batch, args.size // 4, args.size // 4, args.repeats, args.warmup),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats,
        "positives_per_image_min_max": [int(positives.min()), int(positives.max())],
        "positive_share": round(float(positives.sum()) / score.size, 4),
        "max_k": max_k,
        "kept_quads_per_image_min_max": [min(len(k) for k in kept), max(len(k) for k in kept)],
        "decode_ms": round(med(t_dec), 4),
        "decode_ms_min_max": [round(min(t_dec), 4), round(max(t_dec), 4)],
        "decode_lanms_device_ms": round(med(t_both), 4),
        "decode_lanms_device_ms_min_max": [round(min(t_both), 4), round(max(t_both), 4)],
        "detect_host_ms": round(med(t_det), 4),
        "detect_host_ms_min_max": [round(min(t_det), 4), round(max(t_det), 4)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
