#!/usr/bin/env python3
"""What the decode-threshold grid of the link geometry costs (csrc/decode_grid.hip).

    timeout -k 10 900 python scripts/decode_grid_cost.py [--repeats 10] [--warmup 2] [--out profiles/decode_grid.json]

Maps of the 768 x 1280 eval size (192 x 320 at 1/4 resolution), batch 8, drawn once from a fixed seed: planted words with
P(text) uniform in (0.55, 0.99) inside and (0, 0.45) outside, link probabilities uniform in (0.5, 1) inside and (0, 0.5)
outside, so that every grid point between 0.5 and 0.9 decodes a different set.  Three ground truths per image.  For G = 9,
25 and 64 points (k x k, both axes 0.5 .. 0.9) plus the base pair, in ONE process, the arms alternately:

  grid     what `LinkEvaluator(grid=...)` launches per batch behind the maps: pixellink_fn.detect_device_grid per chunk
           (the default chunk, points x images <= 512), one ocr_eval_collect per chunk, the matcher once per point
  loop     what a user of the parent commit runs for the same points: pixellink_fn.detect_device + ocr_eval_collect + the
           matcher, once per point (the forwards, process starts and device reads of that loop are not in the figure)
  forward  one PixelLinkNet forward of the batch at the eval size, for scale

Host clock around work that ends in a device synchronise; medians of --repeats after --warmup with minimum and maximum.
Peak device memory (torch's allocator) is taken around one run of each arm.  The per-point records of the two arms are
compared: they must be equal.  No bar was set: the file records the numbers and the fingerprint of the kernel sources."""
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
EVAL_H, EVAL_W = 768, 1280


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"peak_bytes": torch.cuda.max_memory_allocated(), "held_before_bytes": base}


def planted_maps(n, h, w, device):
    rng = np.random.default_rng(7)
    inside = np.zeros((n, h, w), bool)
    quads = []
    for i in range(n):
        rows = []
        for k in range(12):
            y0, x0 = int(rng.integers(4, h - 30)), int(rng.integers(4, w - 90))
            hh, ww = int(rng.integers(5, 20)), int(rng.integers(20, 80))
            inside[i, y0:y0 + hh, x0:x0 + ww] = True
            if k < 3:
                rows.append([4 * x0, 4 * y0, 4 * (x0 + ww), 4 * y0, 4 * (x0 + ww), 4 * (y0 + hh), 4 * x0, 4 * (y0 + hh)])
        quads.append(np.asarray(rows, np.int32).reshape(-1, 4, 2))
    ps = np.where(inside, rng.uniform(0.55, 0.99, inside.shape), rng.uniform(0.0, 0.45, inside.shape)).astype(np.float32)
    lk = np.where(inside[None], rng.uniform(0.5, 1.0, (8,) + inside.shape), rng.uniform(0.0, 0.5, (8,) + inside.shape)).astype(np.float32)
    return torch.from_numpy(ps).to(device), torch.from_numpy(lk).to(device), quads


def forward_row(g, n, args):
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import pixellink

    def logits(gr, im):
        net = pixellink.PixelLinkNet((im - 120.0) / 60.0, graph=gr)
        return net.pixel_cls, net.link_cls
    forward = GraphedForward(g, logits)
    x = torch.rand((n, EVAL_H, EVAL_W, 3), device=g.device) * 255.0
    ms = [clocked(lambda: forward(x)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    return dict(summary(ms), what="one PixelLinkNet forward (GraphedForward, f16 storage), %d x %d x %d" % (n, EVAL_H, EVAL_W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sides", type=str, default="3,5,8", help="k of the k x k grids")
    ap.add_argument("--no_forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_grid.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, evaluate
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    n, h, w = args.batch, EVAL_H // 4, EVAL_W // 4
    ps, lk, quads = planted_maps(n, h, w, dev)
    record = {"script": "scripts/decode_grid_cost.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "hip": torch.version.hip, "csrc_fingerprint": _lib.csrc_fingerprint(), "date": time.strftime("%Y-%m-%d"),
              "repeats": args.repeats, "warmup": args.warmup, "maps": [n, h, w], "eval_size": [EVAL_H, EVAL_W],
              "timing": "host clock around work that ends in a device synchronise; the two arms alternately in one process; medians",
              "grids": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if not args.no_forward:
        record["forward"] = forward_row(Graph(dev), n, args)
        print("forward %.3f ms" % record["forward"]["median_ms"], flush=True)
        write()
    batch = [(np.zeros((EVAL_H, EVAL_W, 3), np.uint8), quads[i], np.zeros(len(quads[i]), bool)) for i in range(n)]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:                 # the evaluators want a directory with one sample in it
        np.save(os.path.join(tmp, "img.npy"), np.zeros((EVAL_H, EVAL_W, 3), np.uint8))
        with open(os.path.join(tmp, "gt_img.txt"), "w") as f:
            f.write("0,0,8,0,8,8,0,8,text\r\n")
        for side in [int(v) for v in args.sides.split(",")]:
            axis = [0.5 + 0.4 * k / (side - 1) for k in range(side)]
            kw = dict(batch_size=n, eval_image_height=EVAL_H, eval_image_width=EVAL_W)
            ev = evaluate.LinkEvaluator(g, None, tmp, grid=(axis, axis), **kw)
            plain = evaluate.LinkEvaluator(g, None, tmp, **kw)
            ev.detector.maps = lambda srcs: (ps, lk)
            points = ev.grid_points
            gts = ev._ground_truths(batch)
            box_scales = ev.detector.scales(EVAL_H, EVAL_W)
            ones = evaluate.ratio_rows(n, device=dev)
            loop_records = torch.empty((len(points), 4), dtype=torch.int64, device=dev)

            def grid_arm():
                ev.acc.reset()
                return ev._grid_chain(batch, None, gts)

            def loop_arm():
                det = plain.detector
                for k, (p, l) in enumerate(points):
                    plain.acc.reset()
                    rows = P.detect_device(ps, lk, p, l, det.min_size, *box_scales, max_comps=det.max_comps, min_side=det.min_side,
                                           min_area=det.min_area, graph=g)
                    plain._match(*rows[:4], ones, *gts)
                    loop_records[k].copy_(plain.acc.record)
            for _ in range(args.warmup):
                grid_arm()
                loop_arm()
            grid_ms, loop_ms = [], []
            for _ in range(args.repeats):                      # alternately, so that both see the same clocks
                grid_ms.append(clocked(grid_arm))
                loop_ms.append(clocked(loop_arm))
            over = grid_arm()
            loop_arm()
            torch.cuda.synchronize()
            row = {"points": len(points), "grid_points": side * side, "slices": len(points) * n,
                   "chunk_points": ev.grid_chunk or max(1, evaluate.GRID_MAX_SLICES // n),
                   "grid": summary(grid_ms), "loop": summary(loop_ms),
                   "records_equal": bool(torch.equal(ev.acc.records, loop_records)),
                   "overflowing_points": int((over.max(dim=1).values > 0).sum()),
                   "detections_per_point": ev.acc.records[:, 3].tolist(),
                   "memory_grid": peak_of(grid_arm), "memory_loop": peak_of(loop_arm)}
            row["grid_over_loop"] = row["grid"]["median_ms"] / row["loop"]["median_ms"]
            if "forward" in record:
                row["grid_over_forward"] = row["grid"]["median_ms"] / record["forward"]["median_ms"]
            record["grids"][str(side * side)] = row
            print("G = %d + 1: grid %.3f ms, loop %.3f ms, ratio %.3f, records equal %s, peak %.0f MiB (loop %.0f MiB)" % (
                side * side, row["grid"]["median_ms"], row["loop"]["median_ms"], row["grid_over_loop"], row["records_equal"],
                row["memory_grid"]["peak_bytes"] / 2 ** 20, row["memory_loop"]["peak_bytes"] / 2 ** 20), flush=True)
            write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
