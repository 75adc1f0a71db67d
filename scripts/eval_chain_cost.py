#!/usr/bin/env python3
"""What evaluating a batch costs: the device chain (rbox.detect_device -> ocr_eval_collect -> bboxes_matching_batch, the
counters left on the device) against the per-image host path it replaces (rbox.detect, divide on the host,
bboxes.bboxes_matching per image), on n = 16 maps of 256 x 256 with the synthetic RBOX labels of
scripts/rbox_decode_cost.py (two rectangles per image, about 10 % of the pixels above the threshold) and the rectangles'
detections, shifted by a few pixels, as ground truths.

    python scripts/eval_chain_cost.py [--repeats 20] [--warmup 3] [--out profiles/eval_chain.json]

Every figure is the median of repeated runs inside one process after the warm-up.  The device chain is timed twice: between
a pair of HIP events (the work on the device) and on the host clock including the one read of the record that ends a pass;
the host path on the host clock (it synchronises by itself).  Synchronisations are counted by wrapping Tensor.cpu / .item.
Nobody had measured either path before: there is no bar, the file records both numbers.  Written with the fingerprint of
the kernel sources it was measured on."""
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


class SyncCounter:
    """counts Tensor.cpu() / .item() / .tolist() calls on device tensors while active"""

    def __init__(self):
        self.n = 0

    def __enter__(self):
        self.saved = {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}
        for k, fn in self.saved.items():
            def wrapped(t, *a, _fn=fn, **kw):
                if t.is_cuda:
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_chain.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, ops, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import bboxes, metrics, rbox
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    n = args.batch
    rng = np.random.default_rng(7)
    label, geo, _ = synthetic.rbox_labels(n, args.size, rng, rects=2)
    score = (label[..., 0] * rng.uniform(0.72, 1.0, label.shape[:3])).astype(np.float32)
    geo[..., :4] += (label * rng.uniform(-1.5, 1.5, geo[..., :4].shape)).astype(np.float32)
    geo[..., 4] += (label[..., 0] * rng.uniform(-0.02, 0.02, label.shape[:3])).astype(np.float32)
    sd, gd = torch.from_numpy(score).to(dev), torch.from_numpy(geo).to(dev)
    positives = (score > np.float32(0.8)).sum(axis=(1, 2))
    max_k = min(int(-(-int(positives.max()) // 1024) * 1024), rbox.LANMS_MAX_K)
    ratio = np.tile(np.array([[0.75, 1.5]], np.float32), (n, 1))

    def host_boxes(quads, i):
        q = quads[np.argsort(-quads[:, 8], kind="stable")]
        box = q[:, :8].reshape(-1, 4, 2).astype(np.float32)
        box[:, :, 0] /= ratio[i, 0]
        box[:, :, 1] /= ratio[i, 1]
        return box.astype(np.int32)
    # ground truths: each image's detections moved by a few pixels, every third one ignored
    kept = rbox.detect(sd, gd, max_k=max_k, graph=g)
    gts_h = [np.clip(host_boxes(q, i) + rng.integers(-3, 4, (len(q), 1, 2)), 0, None).astype(np.int32) for i, q in enumerate(kept)]
    ign_h = [(np.arange(len(q)) % 3 == 2) for q in gts_h]
    max_g = max(max(len(q) for q in gts_h), 1)
    max_d = 64
    gts, ng, ign = np.zeros((n, max_g, 4, 2), np.int32), np.zeros(n, np.int32), np.zeros((n, max_g), np.uint8)
    for i, q in enumerate(gts_h):
        gts[i, :len(q)], ng[i], ign[i, :len(q)] = q, len(q), ign_h[i]
    up = lambda a: torch.from_numpy(a).to(dev)
    gts_d, ng_d, ign_d, ratio_d = up(gts), up(ng), up(ign), up(ratio)
    side = int(2 * args.size / 0.75) + 10
    acc = metrics.DeviceTpFp(g)

    def device_chain():
        merged, keep, n_keep, passed, total = rbox.detect_device(sd, gd, max_k=max_k, graph=g)
        dets = torch.empty((n, max_d, 4, 2), dtype=torch.int32, device=dev)
        det_score = torch.empty((n, max_d), dtype=torch.float32, device=dev)
        nd, nd_total = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        ops.eval_collect(merged, keep, n_keep, None, ratio_d, dets, det_score, nd, nd_total)
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

    def host_pass():
        t0 = time.perf_counter()
        tot = np.zeros(4, np.int64)
        quads = rbox.detect(sd, gd, max_k=max_k, graph=g)
        for i, q in enumerate(quads):
            box = host_boxes(q, i)
            n_g, tp, fp = bboxes.bboxes_matching(box.reshape(-1, 8), gts_h[i][:, :, 0], gts_h[i][:, :, 1], ign_h[i], 0.5, graph=g)
            tot += [n_g, int(tp.sum()), int(fp.sum()), len(box)]
        return (time.perf_counter() - t0) * 1e3, tuple(int(v) for v in tot)
    for _ in range(args.warmup):
        dv = device_pass()[1]
        hv = host_pass()[1]
    assert dv == hv, (dv, hv)                              # the two paths count the same
    with SyncCounter() as sc:
        device_pass()
    device_syncs = sc.n
    with SyncCounter() as sc:
        host_pass()
    host_syncs = sc.n
    torch.cuda.synchronize()
    t_ev = [device_events() for _ in range(args.repeats)]
    t_dev = [device_pass()[0] for _ in range(args.repeats)]
    t_host = [host_pass()[0] for _ in range(args.repeats)]
    med = statistics.median
    res = {
        "what": "evaluating %d maps of %d x %d: device chain (detect_device + ocr_eval_collect + ocr_eval_match_batch, one read "
                "of the record) against the per-image host path (rbox.detect + bboxes_matching per image); medians of %d runs "
                "in one process after %d warm-up runs" % (n, args.size // 4, args.size // 4, args.repeats, args.warmup),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats,
        "max_k": max_k, "max_d": max_d, "max_g": max_g,
        "record_gt_tp_fp_det": list(dv),
        "device_chain_events_ms": round(med(t_ev), 4),
        "device_chain_events_ms_min_max": [round(min(t_ev), 4), round(max(t_ev), 4)],
        "device_pass_host_ms": round(med(t_dev), 4),
        "device_pass_host_ms_min_max": [round(min(t_dev), 4), round(max(t_dev), 4)],
        "device_pass_syncs": device_syncs,
        "host_path_ms": round(med(t_host), 4),
        "host_path_ms_min_max": [round(min(t_host), 4), round(max(t_host), 4)],
        "host_path_syncs": host_syncs,
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
