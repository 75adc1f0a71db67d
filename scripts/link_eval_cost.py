#!/usr/bin/env python3
"""What evaluating a batch of PixelLink maps costs after the forward pass: the device chain (pixellink_fn.detect_device =
link_cc -> min-area rectangles -> component scores -> boxes, then ocr_eval_collect -> bboxes_matching_batch, the counters
left on the device) against the same work through the host path it replaces (link_cc_decode -> min_area_rect_boxes with its
per-box Python loop, NumPy mean scores, oracle/evalboxes.py per image), on n = 8 maps of 192 x 320 (1280 x 768 images) with a
jittered grid of painted rectangles, a few hundred components per image, and a handful of the host path's own boxes,
shifted by a few pixels, as ground truths.

    python scripts/link_eval_cost.py [--repeats 20] [--host_repeats 3] [--warmup 3] [--out profiles/link_eval.json]

Every device figure is the median of repeated runs inside one process after the warm-up: between a pair of HIP events (the
work on the device), entry by entry with an event between the stages, and on the host clock including the one read of the
record that ends a pass.  The host path is timed on
the host clock in two parts — boxes and scores, then the matching, whose full-image rasters per pair dominate it — over
--host_repeats runs (a pass takes the better part of a minute).  Synchronisations are counted by wrapping Tensor.cpu /
.item / .tolist.  No bar was set: the file records the numbers and their ratio, with the fingerprint of the kernel sources
they were measured on."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def painted_maps(rng, n, h, w, cols, rows):
    """pixel scores: a cols x rows grid of rectangles, jittered in place and size, 0.82..0.99 inside, below 0.5 outside"""
    ps = rng.uniform(0.0, 0.5, (n, h, w)).astype(np.float32)
    ch, cw = h // rows, w // cols
    for b in range(n):
        for r in range(rows):
            for c in range(cols):
                hh, ww = int(rng.integers(4, ch - 4)), int(rng.integers(6, cw - 4))
                y0 = r * ch + 1 + int(rng.integers(0, ch - hh - 2))
                x0 = c * cw + 1 + int(rng.integers(0, cw - ww - 2))
                ps[b, y0:y0 + hh, x0:x0 + ww] = rng.uniform(0.82, 0.99, (hh, ww))
    return ps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host_repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--gts", type=int, default=8, help="ground truths per image")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_eval.json"))
    args = ap.parse_args()
    from eval_chain_cost import SyncCounter
    from oracle import evalboxes as OE
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import bboxes, metrics, pixellink_fn as P
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    n, h4, w4 = args.batch, args.height // 4, args.width // 4
    rng = np.random.default_rng(9)
    ps = painted_maps(rng, n, h4, w4, cols=16, rows=12)
    ps_d = torch.from_numpy(ps).to(dev)
    link_d = torch.full((8, n, h4, w4), 0.95, dtype=torch.float32, device=dev)
    max_comps, max_d, min_size = 1024, 512, 10
    sx, sy = args.width / float(w4), args.height / float(h4)

    def host_boxes():
        """the parent path up to the ordered detection list: [(boxes int32 [k,4,2], scores f32 [k])]"""
        labels, ncomp, _ = P.link_cc_decode(ps_d, link_d, 0.8, 0.9, min_size=min_size, max_comps=max_comps, graph=g)
        boxes = P.min_area_rect_boxes(labels, ncomp, sx, sy, max_comps=max_comps, graph=g)
        lab = labels.cpu().numpy()
        q = np.rint(np.clip(np.where(np.isnan(ps), 0, ps), 0, 1).astype(np.float64) * 16777216.0)
        out = []
        for b, (_, bx) in enumerate(boxes):
            k = len(bx)
            sums = np.bincount(lab[b].reshape(-1), weights=q[b].reshape(-1), minlength=k + 1)[1:k + 1]      # exact below 2^53
            cnt = np.bincount(lab[b].reshape(-1), minlength=k + 1)[1:k + 1]
            sc = (sums / np.maximum(cnt, 1) / 16777216.0).astype(np.float32)
            order = np.argsort(-sc.astype(np.float64), kind="stable")
            out.append((bx[order].astype(np.int32), sc[order]))
        return out
    first = host_boxes()
    comps = [len(b) for b, _ in first]
    # ground truths: a few of each image's boxes moved by some pixels, every third one ignored
    gts_h = [np.clip(b[:: max(1, len(b) // args.gts)][:args.gts] + rng.integers(-3, 4, (1, 1, 2)), 0, None).astype(np.int32) for b, _ in first]
    ign_h = [(np.arange(len(q)) % 3 == 2) for q in gts_h]
    max_g = max(max(len(q) for q in gts_h), 1)
    gts, ng, ign = np.zeros((n, max_g, 4, 2), np.int32), np.zeros(n, np.int32), np.zeros((n, max_g), np.uint8)
    for i, q in enumerate(gts_h):
        gts[i, :len(q)], ng[i], ign[i, :len(q)] = q, len(q), ign_h[i]
    up = lambda a: torch.from_numpy(a).to(dev)
    gts_d, ng_d, ign_d = up(gts), up(ng), up(ign)
    ones = torch.ones((n, 2), dtype=torch.float32, device=dev)
    side = 2 * max(args.height, args.width) + 10
    acc = metrics.DeviceTpFp(g)

    def device_chain():
        merged, keep, n_keep, passed, total = P.detect_device(ps_d, link_d, 0.8, 0.9, min_size, sx, sy, max_comps=max_comps, graph=g)
        dets = torch.empty((n, max_d, 4, 2), dtype=torch.int32, device=dev)
        det_score = torch.empty((n, max_d), dtype=torch.float32, device=dev)
        nd, nd_total = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        ops.eval_collect(merged, keep, n_keep, passed, ones, dets, det_score, nd, nd_total)
        bboxes.bboxes_matching_batch(dets, nd, gts_d, ng_d, ign_d, 0.5, record=acc.record, graph=g, mask_hw=(side, side))
        return total, nd_total

    def device_pass():
        acc.reset()
        t0 = time.perf_counter()
        device_chain()
        value = acc.value()
        return (time.perf_counter() - t0) * 1e3, value

    def device_events():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_chain()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    STAGES = ("link_cc", "min_area_rects", "component_scores", "link_boxes", "eval_collect", "eval_match")

    def device_stages():
        """the chain entry by entry (what detect_device launches, spelled out), a HIP event between the stages -> ms per stage"""
        F32, I32 = torch.float32, torch.int32
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        labels, ncomp, _ = P.link_cc_decode(ps_d, link_d, 0.8, 0.9, min_size=min_size, max_comps=max_comps, graph=g)
        ev[1].record()
        hull_n = torch.zeros((n, max_comps), dtype=I32, device=dev)
        head = torch.zeros((n, max_comps, 4), dtype=I32, device=dev)
        cal = torch.zeros((n, max_comps, 6), dtype=F32, device=dev)
        ops.min_area_rects(labels, ncomp, max_comps, sx, sy, hull_n, head, cal, g.workspace())
        ev[2].record()
        comp_score = torch.empty((n, max_comps), dtype=F32, device=dev)
        ops.component_scores(labels, ps_d, ncomp, comp_score, g.workspace())
        ev[3].record()
        merged = torch.empty((n, max_comps, 9), dtype=F32, device=dev)
        keep = torch.empty((n, max_comps), dtype=I32, device=dev)
        n_keep, total = torch.empty((n,), dtype=I32, device=dev), torch.empty((n,), dtype=I32, device=dev)
        passed = torch.empty((n, max_comps), dtype=torch.uint8, device=dev)
        ops.link_boxes(hull_n, head, cal, comp_score, ncomp, 0.0, 0.0, merged, keep, n_keep, passed, total)
        ev[4].record()
        dets = torch.empty((n, max_d, 4, 2), dtype=I32, device=dev)
        det_score = torch.empty((n, max_d), dtype=F32, device=dev)
        nd, nd_total = torch.empty((n,), dtype=I32, device=dev), torch.empty((n,), dtype=I32, device=dev)
        ops.eval_collect(merged, keep, n_keep, passed, ones, dets, det_score, nd, nd_total)
        ev[5].record()
        bboxes.bboxes_matching_batch(dets, nd, gts_d, ng_d, ign_d, 0.5, record=acc.record, graph=g, mask_hw=(side, side))
        ev[6].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(STAGES))]

    def host_pass():
        t0 = time.perf_counter()
        found = host_boxes()
        t1 = time.perf_counter()
        tot = np.zeros(4, np.int64)
        for i, (box, _) in enumerate(found):
            n_g, tp, fp = OE.bboxes_matching(box.reshape(-1, 8), gts_h[i][:, :, 0], gts_h[i][:, :, 1], ign_h[i], 0.5)
            tot += [n_g, int(tp.sum()), int(fp.sum()), len(box)]
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, tuple(int(v) for v in tot)
    for _ in range(args.warmup):
        dv = device_pass()[1]
    with SyncCounter() as sc:
        device_pass()
    device_syncs = sc.n
    with SyncCounter() as sc:
        host_boxes()
    host_syncs = sc.n
    torch.cuda.synchronize()
    t_ev = [device_events() for _ in range(args.repeats)]
    t_dev = [device_pass()[0] for _ in range(args.repeats)]
    t_st = [device_stages() for _ in range(args.repeats)]
    host = [host_pass() for _ in range(max(1, args.host_repeats))]
    assert all(hv[2] == dv for hv in host), (dv, host)     # the two paths count the same
    med = statistics.median
    t_hb, t_hm = [x[0] for x in host], [x[1] for x in host]
    t_host = [a + b for a, b in zip(t_hb, t_hm)]
    res = {
        "what": "evaluating %d PixelLink maps of %d x %d (%d x %d images) after the forward pass: device chain (detect_device = "
                "link_cc + min_area_rects + component_scores + link_boxes, ocr_eval_collect, ocr_eval_match_batch, one read of the "
                "record) against the host path (link_cc_decode + min_area_rect_boxes + NumPy scores, then oracle/evalboxes.py per "
                "image); device medians of %d runs in one process after %d warm-up runs, host medians of %d runs"
                % (n, h4, w4, args.width, args.height, args.repeats, args.warmup, len(host)),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats, "host_repeats": len(host),
        "components_per_image": comps,
        "max_comps": max_comps, "max_d": max_d, "max_g": max_g,
        "record_gt_tp_fp_det": list(dv),
        "device_chain_events_ms": round(med(t_ev), 4),
        "device_chain_events_ms_min_max": [round(min(t_ev), 4), round(max(t_ev), 4)],
        "device_pass_host_ms": round(med(t_dev), 4),
        "device_pass_host_ms_min_max": [round(min(t_dev), 4), round(max(t_dev), 4)],
        "device_pass_syncs": device_syncs,
        "device_stage_events_ms": {name: round(med([t[i] for t in t_st]), 4) for i, name in enumerate(STAGES)},
        "host_boxes_and_scores_ms": round(med(t_hb), 4),
        "host_boxes_and_scores_syncs": host_syncs,
        "host_matching_ms": round(med(t_hm), 4),
        "host_path_ms": round(med(t_host), 4),
        "host_path_ms_min_max": [round(min(t_host), 4), round(max(t_host), 4)],
        "host_over_device_pass": round(med(t_host) / med(t_dev), 2),
        "host_boxes_and_scores_over_device_pass": round(med(t_hb) / med(t_dev), 2),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
