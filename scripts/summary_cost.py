#!/usr/bin/env python3
"""What one variables + gradients summary pass (summary.TensorStats, ocr_tensor_stats_f32) costs on the headline
configuration: VGG-16 `model_vgg` + dice loss, 512 x 512, batch 32, one GPU.

    python scripts/summary_cost.py [--repeats 10] [--warmup 6] [--batch 32] [--size 512] [--out profiles/summary_cost.json]

The yardstick is the reference's own price: it runs one more full train step per summary (multigpu_train.py:189-194).
So in ONE process a replayed train step and the summary pass take turns, each block between its own pair of HIP events:
a block of four steps, then the two passes (variables with factor 1, gradients with TrainStep.summary_factor()) enqueued
behind the last step as the training scripts do, then the read of both record buffers timed on the host.  The pass is
reported as a fraction of the median step of the same process.  The result is written with the fingerprint of the kernel
sources it was measured on."""
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


def make_step(device, batch, size):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=1)
    data = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), batch, size)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, data, TrainStep(g, fl, lambda gr: AdamOptimizer(gr))


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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_cost.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, summary
    dev = torch.device("cuda", 0)
    g, data, step = make_step(dev, args.batch, args.size)
    for _ in range(3 + args.warmup):
        step(*data)
    st = g.store
    var_stats, grad_stats = summary.TensorStats(st), summary.TensorStats(st)

    def both():
        var_stats.run(st.flat)
        grad_stats.run(st.flat_grad, *step.summary_factor())
    timed(both)                                   # warm
    B = 4                                         # steps per timed block: the queue stays full inside a block
    step_ms, pass_ms, read_ms = [], [], []
    for _ in range(args.repeats):                 # step block and pass in turn: drift hits both alike
        step_ms.append(timed(lambda: [step(*data) for _ in range(B)]) / B)
        pass_ms.append(timed(both))
        t0 = time.perf_counter()
        varis, grads = var_stats.read(), grad_stats.read()
        read_ms.append((time.perf_counter() - t0) * 1e3)
    n = st.flat.numel()
    med_step, med_pass = statistics.median(step_ms), statistics.median(pass_ms)
    out = {
        "what": "one variables + gradients summary pass (two ocr_tensor_stats_f32 calls) against the replayed train step of "
                "the same process: model_vgg + dice, %d x %d, batch %d; step blocks of four and the pass take turns" % (
                    args.size, args.size, args.batch),
        "csrc_fingerprint": _lib.csrc_fingerprint(), "dtype": _lib.STORAGE, "device": torch.cuda.get_device_name(0),
        "repeats": args.repeats, "flat_elements": n, "variables": len(var_stats.names), "chunks": var_stats.n_chunks,
        "step_ms": round(med_step, 4), "step_ms_min_max": [round(min(step_ms), 4), round(max(step_ms), 4)],
        "summary_pass_ms": round(med_pass, 4), "summary_pass_ms_min_max": [round(min(pass_ms), 4), round(max(pass_ms), 4)],
        "summary_pass_over_step": round(med_pass / med_step, 5),
        "records_read_host_ms": round(statistics.median(read_ms), 3),
        "pass_bytes_per_s": round(2 * 4.0 * n / (med_pass * 1e-3), 0),
        "reference_price": "one extra train step per summary (multigpu_train.py:189-194): 1.0 on this scale",
        "gradient_elements_counted": int(sum(r["num"] + r["nonfinite"] for r in grads.values())),
        "variable_elements_counted": int(sum(r["num"] + r["nonfinite"] for r in varis.values())),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
