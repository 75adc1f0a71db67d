#!/usr/bin/env python3
"""What dynamic loss scaling (graph.DynamicLossScale) costs on the headline configuration: VGG-16 `model_vgg` + dice loss,
512 x 512, batch 32, one GPU.

    python scripts/dynamic_loss_scale_cost.py [--steps 40] [--warmup 6] [--batch 32] [--size 512] [--out profiles/dynamic_loss_scale.json]

In ONE process a static (loss_scale=1024) and a dynamic (init_scale=1024: same arithmetic, no skip) tower take turns, four
replayed steps each, every block between a pair of HIP events: the difference of the medians is the price of the mode — one
more launch (ocr_grad_check_f32) and the state reads of the `_dyn` kernels.  Then the check kernel is event-timed alone
on the tower's flat gradient buffer, beside ocr_adam_step on the same buffers in the same run: Adam's bytes/s is the
streaming rate this box delivers on exactly these buffers, the yardstick for a pass that reads a ninth of what Adam
touches (g against w, g, m, v, ema read + w, m, v, ema written).  Both are timed over a ring of buffer sets larger than
the 256 MB infinity cache, so neither is flattered by a resident operand.  The result is written with the fingerprint of
the kernel sources it was measured on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_step(device, loss_scale, batch, size):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=loss_scale, seed=1)
    data = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), batch, size)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, data, TrainStep(g, fl, lambda gr: AdamOptimizer(gr))


def timed(fn, reps):
    """Median ms of `fn(i)` over `reps` calls, each between its own pair of events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamic_loss_scale.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd.graph import DynamicLossScale
    dev = torch.device("cuda", 0)
    gs, ds, ss = make_step(dev, 1024.0, args.batch, args.size)
    gd, dd, sd = make_step(dev, DynamicLossScale(init_scale=1024.0, growth_interval=1 << 30), args.batch, args.size)
    for _ in range(3 + args.warmup):
        ss(*ds)
        sd(*dd)
    torch.cuda.synchronize()
    ts, td = [], []
    B = 4                                         # steps per timed block: the queue stays full inside a block
    for _ in range(max(1, args.steps // B)):      # static, dynamic, static, dynamic, ...: drift hits both alike
        ts.append(timed(lambda i: [ss(*ds) for _ in range(B)], 1) / B)
        td.append(timed(lambda i: [sd(*dd) for _ in range(B)], 1) / B)
    same = bool(torch.equal(gs.store.flat, gd.store.flat))
    assert gd.loss_scaler.skipped_steps() == 0

    # the two streams alone, on a ring of buffer sets that does not fit the infinity cache
    st = gd.store
    n = st.flat.numel()
    ring = max(2, -(-(768 << 20) // (4 * n)))
    grads = [st.flat_grad.clone() for _ in range(ring)]
    sets = [[torch.zeros_like(st.flat) for _ in range(4)] for _ in range(ring)]          # w, m, v, ema per set
    state = gd.loss_scaler.state.clone()
    reps = 10 * ring
    sc = gd.loss_scaler

    def check(i):
        ops.grad_check(grads[i % ring], state, sc.growth_factor, sc.backoff_factor, 1 << 30, sc.min_scale, sc.max_scale)

    def adam(i):
        w, m, v, e = sets[i % ring]
        ops.adam_step(w, grads[i % ring], m, v, e, st.n_reg, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0 / 1024, 0.997)

    def adam_dyn(i):
        w, m, v, e = sets[i % ring]
        ops.adam_step_dyn(w, grads[i % ring], m, v, e, st.n_reg, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0, 0.997, state)
    for f in (check, adam, adam_dyn):
        timed(f, ring)                            # warm
    t_check, t_adam, t_adam_dyn = timed(check, reps), timed(adam, reps), timed(adam_dyn, reps)
    rate_check = 4.0 * n / (t_check * 1e-3)
    rate_adam = 36.0 * n / (t_adam * 1e-3)        # 5 reads + 4 writes of 4 bytes per element
    ms_s, ms_d = statistics.median(ts), statistics.median(td)
    out = {
        "what": "dynamic loss scaling vs the static scale: model_vgg + dice, %d x %d, batch %d, replayed steps taking turns in "
                "one process; then ocr_grad_check_f32 and ocr_adam_step alone on the tower's flat buffers" % (args.size, args.size, args.batch),
        "csrc_fingerprint": _lib.csrc_fingerprint(), "dtype": _lib.STORAGE, "device": torch.cuda.get_device_name(0),
        "steps": args.steps, "static_ms_per_step": round(ms_s, 4), "dynamic_ms_per_step": round(ms_d, 4),
        "dynamic_minus_static_ms": round(ms_d - ms_s, 4), "dynamic_over_static": round(ms_d / ms_s, 5),
        "static_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "dynamic_ms_min_max": [round(min(td), 4), round(max(td), 4)],
        "parameters_bit_identical_after_run": same,
        "flat_elements": n, "ring_of_buffer_sets": ring,
        "grad_check_us": round(t_check * 1e3, 2), "grad_check_bytes_per_s": round(rate_check, 0),
        "adam_us": round(t_adam * 1e3, 2), "adam_bytes_per_s": round(rate_adam, 0), "adam_dyn_us": round(t_adam_dyn * 1e3, 2),
        "grad_check_rate_over_adam_rate": round(rate_check / rate_adam, 4),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
