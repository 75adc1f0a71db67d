#!/usr/bin/env python3
"""What the device augmentation costs, in one process on one box:

  (a) image preparation of a batch, 32 images of 1280x720 -> 512^2, device-resident source bytes: the un-augmented
      path's 32 launches of ocr_resize_linear_u8 against ONE launch of ocr_augment_u8_batch whose descriptors express the
      same plain stretch (the two interpolate differently — cv2's 11-bit fixed point against 5-bit fractions — so only
      the time is compared), alternated; plus both end to end (host packing + PCIe) through datasets/icdar.py;
  (b) the headline step (model_vgg + dice + Adam, batch 32 at 512^2) fed from disk through icdar.get_batch, augmentation
      off and `pixellink`, same num_workers, alternated off / on / off / on; with the split the issue asks for when the
      two differ: host planning time per batch (Augment.plan alone) and kernel time per batch.

Writes one JSON document (default profiles/augment_feed.json).  Dev/measurement tool: not part of the driver contract."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def dev_ms(fn, warmup=3, steps=20):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def wall_ms(fn, warmup=2, steps=8):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def prepare(rounds):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.datasets.augment import _scale, fixed_inverse, pack_desc
    from tensorflow_ocr_amd.graph import Graph
    dev = torch.device("cuda", 0)
    g = Graph(dev)
    rng = np.random.default_rng(9)
    n, H, W, S = 32, 720, 1280, 512
    ims = [rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(n)]
    sz = H * W * 3
    slab = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)
    A = fixed_inverse(_scale(S / float(W), S / float(H)))
    plans = [(A, np.eye(3, 4, dtype=np.float32))] * n
    desc = torch.from_numpy(pack_desc([b * sz for b in range(n)], [im.shape for im in ims], plans, n * sz).view(np.uint8).copy()).to(dev)
    out = torch.empty((n, S, S, 3), device=dev)
    views = [slab[b * sz:(b + 1) * sz].view(H, W, 3) for b in range(n)]

    def old():
        for b in range(n):
            ops.resize_linear_u8(views[b], out[b])

    def new():
        ops.augment_u8_batch(slab, desc, n, S, out)
    k_old, k_new, e_old, e_new = [], [], [], []
    for _ in range(rounds):
        k_old.append(dev_ms(old))
        k_new.append(dev_ms(new))
    for _ in range(rounds):
        e_old.append(wall_ms(lambda: icdar.resize_images(ims, S, graph=g)))
        e_new.append(wall_ms(lambda: icdar.augment_images(ims, plans, S, graph=g)))
    nbytes = n * (sz + S * S * 12)
    med = lambda v: float(np.median(v))
    return {"what": "%d images %dx%d -> %d^2, source bytes resident on the device; ms per batch, device events, %d alternated rounds of 20"
                    % (n, W, H, S, rounds),
            "resize_linear_u8_32_launches_ms": [round(v, 4) for v in k_old], "augment_u8_batch_1_launch_ms": [round(v, 4) for v in k_new],
            "median_ms": {"resize_linear_u8": round(med(k_old), 4), "augment_u8_batch": round(med(k_new), 4)},
            "new_over_old": round(med(k_new) / med(k_old), 4),
            "bytes_per_batch": nbytes, "augment_u8_batch_GBps": round(nbytes / (med(k_new) * 1e-3) / 1e9, 1),
            "resize_linear_u8_GBps": round(nbytes / (med(k_old) * 1e-3) / 1e9, 1),
            "end_to_end_incl_host_pack_and_pcie_ms": {"resize_images": [round(v, 3) for v in e_old], "augment_images": [round(v, 3) for v in e_new]}}


def fed(steps, warmup, workers, rounds, root):
    from bench_configs import make_icdar_dir
    from tensorflow_ocr_amd.datasets import _decode, icdar
    from tensorflow_ocr_amd.datasets.augment import Augment
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    batch, size = 32, 512
    root = make_icdar_dir(root)
    dev = torch.device("cuda", 0)
    g = Graph(dev, loss_scale=1024.0, seed=1)

    def fl(gr, im, sm, gm, tm):
        a, b = M.model_vgg(im, is_training=True, graph=gr)
        return M.loss(sm, a, gm, b, tm, graph=gr)
    step = TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-4))

    def run(spec):
        feeder = icdar.get_batch(num_workers=workers, training_data_path=root, input_size=size, batch_size=batch, graph=g,
                                 seed=1, augment=Augment.parse(spec))
        try:
            def nxt():
                images, _, score, geo, mask = next(feeder)
                return [images, score, geo, mask]
            for _ in range(max(warmup, 3)):
                step(*nxt())
            torch.cuda.synchronize()
            waits, t0 = 0.0, time.perf_counter()
            for _ in range(steps):
                tw = time.perf_counter()
                b = nxt()
                waits += time.perf_counter() - tw
                step(*b)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3, waits / steps * 1e3
        finally:
            feeder.close()
    off, on, w_off, w_on = [], [], [], []
    for _ in range(rounds):
        a, wa = run("none")
        b, wb = run("pixellink")
        off.append(a)
        on.append(b)
        w_off.append(wa)
        w_on.append(wb)
    # the split: planning on the host (one thread, the generator's) and the kernel, per batch of 32
    aug = Augment.parse("pixellink")
    files = sorted(icdar.get_images(root))[:64]
    smps = [s for s in (_decode.load_sample((f, size, True)) for f in files) if s is not None]
    rng = np.random.RandomState(1)
    t0, made, plans, ims = time.perf_counter(), 0, [], []
    for rep in range(4):
        for s in smps:
            made += 1
            p = aug.plan(rng, s[1].shape[0], s[1].shape[1], s[2], s[3], size)
            if p is not None and len(plans) < batch:
                plans.append(p)
                ims.append(s[1])
    plan_ms = (time.perf_counter() - t0) / made * 1e3
    e2e = wall_ms(lambda: icdar.augment_images(ims, plans, size, graph=g))
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.datasets.augment import pack_desc
    szs = [im.size for im in ims]
    offs = [int(o) for o in np.cumsum([0] + szs[:-1])]
    slab = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)
    desc = torch.from_numpy(pack_desc(offs, [im.shape for im in ims], plans, sum(szs)).view(np.uint8).copy()).to(dev)
    out = torch.empty((len(ims), size, size, 3), device=dev)
    k_ms = dev_ms(lambda: ops.augment_u8_batch(slab, desc, len(ims), size, out))
    med = lambda v: float(np.median(v))
    ratio = med(on) / med(off)
    return {"what": "model_vgg + dice + Adam, batch %d at %d^2, fed by icdar.get_batch from 128 synthetic 1280x720 JPEGs in the page "
                    "cache, %d decode worker processes, %d timed steps per run, runs alternated off / on" % (batch, size, workers, steps),
            "step_ms_augment_none": [round(v, 3) for v in off], "step_ms_augment_pixellink": [round(v, 3) for v in on],
            "host_wait_ms_per_step_none": [round(v, 3) for v in w_off], "host_wait_ms_per_step_pixellink": [round(v, 3) for v in w_on],
            "median_ms": {"none": round(med(off), 3), "pixellink": round(med(on), 3)}, "pixellink_over_none": round(ratio, 4),
            "within_2_percent": bool(ratio <= 1.02),
            "split_per_batch": {"plan_ms_per_sample_drawn": round(plan_ms, 4),
                                "plan_ms_per_batch_of_32_drawn": round(plan_ms * batch, 3),
                                "augment_kernel_ms": round(k_ms, 4), "augment_images_e2e_ms_incl_host_pack_and_pcie": round(e2e, 3),
                                "note": "the plan is drawn in the generator's thread, serial with its slab packing; pixellink "
                                        "skips samples (background draws that find text), so more than 32 are decoded and planned per batch"},
            "excess_owner": ("none: within 2 %" if ratio <= 1.02 else
                             ("host planning / decode of skipped samples" if plan_ms * batch > k_ms else "kernel"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--root", default="/tmp/ocr_icdar_synth")
    ap.add_argument("--which", default="prepare,fed")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "augment_feed.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_feed.py measures on the GPU; there is none here")
    from tensorflow_ocr_amd import _lib
    doc = {"script": "scripts/augment_feed.py", "device": torch.cuda.get_device_name(0), "csrc_fingerprint": _lib.csrc_fingerprint(),
           "args": {k: v for k, v in vars(a).items() if k not in ("out", "root")}}
    if "prepare" in a.which:
        doc["prepare"] = prepare(a.rounds)
        print(json.dumps(doc["prepare"]), flush=True)
    if "fed" in a.which:
        doc["fed"] = fed(a.steps, a.warmup, a.workers, a.rounds, a.root)
        print(json.dumps(doc["fed"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
