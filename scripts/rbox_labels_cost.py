#!/usr/bin/env python3
"""What the RBOX training labels and the post-NMS score filter cost on the device.

  labels   datasets/icdar.generate_rbox_batch on 32 images of 512 x 512 with 12 quadrangles each (perturbed rotated
           rectangles, every fifth tagged), the SAME polygon lists for geometry='RBOX' (ocr_poly_cover twice +
           ocr_icdar_rbox_labels) and for the link labels (ocr_poly_cover + ocr_icdar_labels): the launches alone between a pair
           of HIP events with the packed polygons already on the device, the whole call on the host clock (packing,
           upload, launches, a synchronisation), and the host packing alone (pack_rbox fits one rectangle per polygon).
  filter   ocr_quad_mean_score on the kept quads of scripts/rbox_decode_cost.py's maps (16 maps of 256 x 256, about 10 %
           of the pixels above the threshold): the launches alone on the kept quads, and tool/rbox.detect on the host
           clock without and with box_thresh.

    python scripts/rbox_labels_cost.py [--repeats 20] [--warmup 3] [--out profiles/rbox_labels.json]

Every figure is the median of repeated runs inside one process after the warm-up.  There is no pass / fail bar: nobody
had measured these.  The result is written with the fingerprint of the kernel sources it was measured on."""
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


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def polygons(rng, n, per_image, size):
    polys_l, tags_l = [], []
    for _ in range(n):
        pl = []
        for _ in range(per_image):
            W, H, a = rng.uniform(40, size / 3), rng.uniform(14, size / 10), rng.uniform(-0.7, 0.7)
            c = rng.uniform(0.1 * size, 0.9 * size, 2)
            u, v = np.array([np.cos(a), -np.sin(a)]), np.array([np.sin(a), np.cos(a)])
            q = np.array([c - W / 2 * u - H / 2 * v, c + W / 2 * u - H / 2 * v, c + W / 2 * u + H / 2 * v, c - W / 2 * u + H / 2 * v])
            pl.append(np.clip(q + rng.uniform(-1, 1, (4, 2)) * 0.1 * H, 0, size - 1))
        polys_l.append(np.array(pl, np.float32))
        tags_l.append(np.arange(per_image) % 5 == 4)
    return polys_l, tags_l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbox_labels.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, ops, synthetic
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import F32, Graph
    from tensorflow_ocr_amd.tool import rbox
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    med = statistics.median
    rng = np.random.default_rng(7)

    # ---- labels
    n, size, per_image, step = 32, 512, 12, 4
    polys_l, tags_l = polygons(rng, n, per_image, size)
    t0 = time.perf_counter()
    shrunk, full, counts, ignore, rects = icdar.pack_rbox(polys_l, tags_l)
    pack_rbox_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    icdar.pack_polys(polys_l, tags_l)
    pack_link_ms = (time.perf_counter() - t0) * 1e3
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(shrunk=shrunk, full=full, counts=counts, ignore=ignore, rects=rects).items()}
    zero_ignore = torch.zeros_like(d["ignore"])
    q = size // step
    cover_s = torch.empty((n, size, size), dtype=torch.int32, device=dev)
    cover_f = torch.empty_like(cover_s)
    score, mask = torch.empty((n, q, q, 1), dtype=F32, device=dev), torch.empty((n, q, q, 1), dtype=F32, device=dev)
    geo5, geo8 = torch.empty((n, q, q, 5), dtype=F32, device=dev), torch.empty((n, q, q, 8), dtype=F32, device=dev)

    def rbox_launches():
        ops.poly_cover(d["shrunk"], d["counts"], zero_ignore, size, size, cover_s)
        ops.poly_cover(d["full"], d["counts"], d["ignore"], size, size, cover_f)
        ops.rbox_labels(cover_s, cover_f, d["rects"], step, score, geo5, mask)

    def rbox_tail():
        ops.rbox_labels(cover_s, cover_f, d["rects"], step, score, geo5, mask)

    def link_launches():
        ops.poly_cover(d["full"], d["counts"], d["ignore"], size, size, cover_f)
        ops.icdar_labels(cover_f, step, score, geo8, mask)

    def rbox_call():
        icdar.generate_rbox_batch((size, size), polys_l, tags_l, graph=g, geometry='RBOX')

    def link_call():
        icdar.generate_rbox_batch((size, size), polys_l, tags_l, graph=g)
    for _ in range(args.warmup):
        rbox_launches(), link_launches(), rbox_call(), link_call()
    torch.cuda.synchronize()
    t_rl = [timed(rbox_launches) for _ in range(args.repeats)]
    t_rt = [timed(rbox_tail) for _ in range(args.repeats)]
    t_ll = [timed(link_launches) for _ in range(args.repeats)]
    t_rc = [host_timed(rbox_call) for _ in range(args.repeats)]
    t_lc = [host_timed(link_call) for _ in range(args.repeats)]

    # ---- filter: the maps of scripts/rbox_decode_cost.py
    rng = np.random.default_rng(7)
    batch, msize = 16, 1024
    label, geo, _ = synthetic.rbox_labels(batch, msize, rng, rects=2)
    sc = (label[..., 0] * rng.uniform(0.72, 1.0, label.shape[:3])).astype(np.float32)
    geo[..., :4] += (label * rng.uniform(-1.5, 1.5, geo[..., :4].shape)).astype(np.float32)
    geo[..., 4] += (label[..., 0] * rng.uniform(-0.02, 0.02, label.shape[:3])).astype(np.float32)
    sd, gd = torch.from_numpy(sc).to(dev), torch.from_numpy(geo).to(dev)
    positives = (sc > np.float32(0.8)).sum(axis=(1, 2))
    max_k = min(int(-(-int(positives.max()) // 1024) * 1024), rbox.LANMS_MAX_K)
    kept = rbox.detect(sd, gd, max_k=max_k, graph=g)
    filtered = rbox.detect(sd, gd, max_k=max_k, graph=g, box_thresh=0.1)
    quads = [torch.from_numpy(np.ascontiguousarray(k[:, :8])).to(dev) for k in kept]
    means = [torch.empty((len(k),), dtype=F32, device=dev) for k in kept]

    def mean_launches():
        for i in range(batch):
            ops.quad_mean_score(quads[i], sd[i], 0.25, means[i])

    def detect_plain():
        rbox.detect(sd, gd, max_k=max_k, graph=g)

    def detect_filtered():
        rbox.detect(sd, gd, max_k=max_k, graph=g, box_thresh=0.1)
    for _ in range(args.warmup):
        mean_launches(), detect_plain(), detect_filtered()
    torch.cuda.synchronize()
    t_ml = [timed(mean_launches) for _ in range(args.repeats)]
    t_dp = [host_timed(detect_plain) for _ in range(args.repeats)]
    t_df = [host_timed(detect_filtered) for _ in range(args.repeats)]

    def mm(t):
        return [round(min(t), 4), round(max(t), 4)]
    res = {
        "what": "RBOX vs link label maps on %d images of %d x %d, %d polygons each (step %d), and ocr_quad_mean_score on the kept "
                "quads of %d maps of %d x %d; medians of %d runs in one process after %d warm-up runs"
                % (n, size, size, per_image, step, batch, msize // 4, msize // 4, args.repeats, args.warmup),
        "csrc_fingerprint": _lib.csrc_fingerprint(),
        "dtype": _lib.STORAGE,
        "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats,
        "rbox_labels_launches_ms": round(med(t_rl), 4), "rbox_labels_launches_ms_min_max": mm(t_rl),
        "rbox_labels_kernel_alone_ms": round(med(t_rt), 4), "rbox_labels_kernel_alone_ms_min_max": mm(t_rt),
        "link_labels_launches_ms": round(med(t_ll), 4), "link_labels_launches_ms_min_max": mm(t_ll),
        "rbox_labels_call_host_ms": round(med(t_rc), 4), "rbox_labels_call_host_ms_min_max": mm(t_rc),
        "link_labels_call_host_ms": round(med(t_lc), 4), "link_labels_call_host_ms_min_max": mm(t_lc),
        "pack_rbox_host_ms": round(pack_rbox_ms, 4), "pack_link_host_ms": round(pack_link_ms, 4),
        "kept_quads_per_image_min_max": [min(len(k) for k in kept), max(len(k) for k in kept)],
        "kept_quads_after_box_thresh_0.1_min_max": [min(len(k) for k in filtered), max(len(k) for k in filtered)],
        "max_k": max_k,
        "quad_mean_score_launches_ms": round(med(t_ml), 4), "quad_mean_score_launches_ms_min_max": mm(t_ml),
        "detect_host_ms": round(med(t_dp), 4), "detect_host_ms_min_max": mm(t_dp),
        "detect_box_thresh_host_ms": round(med(t_df), 4), "detect_box_thresh_host_ms_min_max": mm(t_df),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
