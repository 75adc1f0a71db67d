#!/usr/bin/env python3
"""What gradient accumulation (TrainStep(accumulate_steps=K)) costs on the headline configuration: VGG-16 `model_vgg` +
dice loss, 512 x 512, batch 32, one GPU.

    python scripts/grad_accum_cost.py [--steps 40] [--warmup 8] [--batch 32] [--size 512] [--out profiles/grad_accum.json]

In ONE process two towers take turns: the plain step (K = 1: what bench.py measures, the yardstick) and K = 4.  Every
replayed call stands between its own pair of HIP events; the K = 4 tower's calls are sorted by their phase into the
micro-steps inside a window (forward, backward, one accumulate pass that writes the second buffer, the advance) and the
closing ones (the accumulate pass that writes the gradient buffer, then optimiser and re-pack as in the plain step).
Medians, with the fingerprint of the kernel sources they were measured on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_step(device, K, batch, size):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=1)
    data = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), batch, size)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, data, TrainStep(g, fl, lambda gr: AdamOptimizer(gr), accumulate_steps=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed calls of the plain tower; the K = 4 tower makes as many")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib
    dev = torch.device("cuda", 0)
    K = 4
    plain, accum = make_step(dev, 1, args.batch, args.size), make_step(dev, K, args.batch, args.size)
    warm = K * -(-(3 + args.warmup) // K)            # whole windows; both towers are replaying afterwards
    for _ in range(warm):
        for g, d, s in (plain, accum):
            s(*d)
    torch.cuda.synchronize()
    assert plain[2].plan is not None and accum[2].plan is not None and accum[2].micro_step == 0
    ev = {"k1": [], "k4_inside": [], "k4_closing": []}
    for _ in range(K * max(1, args.steps // K)):     # the towers in turn: drift hits both alike
        for name, (g, d, s) in (("k1", plain), ("k4", accum)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s(*d)
            b.record()
            key = name if name == "k1" else ("k4_closing" if s.closes_window else "k4_inside")
            ev[key].append((a, b))
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    n = plain[0].store.flat.numel()
    out = {
        "what": "gradient accumulation vs none: model_vgg + dice, %d x %d, batch %d, replayed calls of two towers taking turns in "
                "one process, each call between its own pair of events: K = 1, and K = 4 split into the calls inside a window "
                "and the closing ones" % (args.size, args.size, args.batch),
        "csrc_fingerprint": _lib.csrc_fingerprint(), "dtype": _lib.STORAGE, "device": torch.cuda.get_device_name(0),
        "calls": {k: len(v) for k, v in ms.items()},
        "ms_per_call": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "k4_inside_minus_k1_ms": round(med["k4_inside"] - med["k1"], 4),
        "k4_closing_minus_k1_ms": round(med["k4_closing"] - med["k1"], 4),
        "k4_ms_per_image_over_k1": round(((K - 1) * med["k4_inside"] + med["k4_closing"]) / (K * med["k1"]), 4),
        "flat_elements": n, "accumulate_bytes_store_rule": 8 * n, "accumulate_bytes_add_and_close_rules": 12 * n,
        "windows_closed": accum[2].accum.windows(), "optimiser_steps": accum[2].opt.global_step,
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
