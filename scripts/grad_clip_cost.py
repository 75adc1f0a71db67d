#!/usr/bin/env python3
"""What global-norm gradient clipping (AdamOptimizer(clip_norm=...)) costs on the headline configuration: VGG-16
`model_vgg` + dice loss, 512 x 512, batch 32, one GPU.

    python scripts/grad_clip_cost.py [--steps 40] [--warmup 6] [--batch 32] [--size 512] [--out profiles/grad_clip.json]

In ONE process four towers take turns, four replayed steps each, every block between a pair of HIP events: static
(loss_scale=1024), dynamic (init_scale=1024), static + clip and dynamic + clip, the clipped ones with clip_norm=1e30 (the
same arithmetic: coef == 1, parameters stay bit-identical).  The differences of the medians are the price of the mode: one
more launch with a numeric loss scale (ocr_grad_clip_f32), none with a dynamic one (ocr_grad_check_clip_f32 in the place of
ocr_grad_check_f32).  Then the fused pass, the static clip pass and ocr_grad_check_f32 are event-timed alone over a ring of
gradient buffers larger than the 256 MB infinity cache: the check kernel's bytes/s on the same buffers in the same process
is the yardstick for the passes that sum the norm beside it.  The result is written with the fingerprint of the kernel
sources it was measured on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_step(device, loss_scale, clip_norm, batch, size):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=loss_scale, seed=1)
    data = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), batch, size)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, data, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, clip_norm=clip_norm))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.json"))
    args = ap.parse_args()
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd.graph import DynamicLossScale
    dev = torch.device("cuda", 0)
    dyn = lambda: DynamicLossScale(init_scale=1024.0, growth_interval=1 << 30)
    arms = [("static", 1024.0, None), ("dynamic", dyn(), None), ("static_clip", 1024.0, 1e30), ("dynamic_clip", dyn(), 1e30)]
    towers = {name: make_step(dev, ls, c, args.batch, args.size) for name, ls, c in arms}
    for _ in range(3 + args.warmup):
        for g, d, s in towers.values():
            s(*d)
    torch.cuda.synchronize()
    ms = {name: [] for name in towers}
    B = 4                                         # steps per timed block: the queue stays full inside a block
    for _ in range(max(1, args.steps // B)):      # the four arms in turn: drift hits all alike
        for name, (g, d, s) in towers.items():
            ms[name].append(timed(lambda i: [s(*d) for _ in range(B)], 1) / B)
    ref = towers["static"][0].store.flat
    same = all(bool(torch.equal(ref, g.store.flat)) for g, _, _ in towers.values())
    for name in ("static_clip", "dynamic_clip"):
        opt = towers[name][2].opt
        assert opt.clipped_steps() == 0 and opt.nonfinite_steps() == 0
    norm = towers["dynamic_clip"][2].opt.grad_norm()

    # the passes alone, on a ring of gradient buffers that does not fit the infinity cache
    gd = towers["dynamic_clip"][0]
    st = gd.store
    n = st.flat.numel()
    ring = max(2, -(-(768 << 20) // (4 * n)))
    grads = [st.flat_grad.clone() for _ in range(ring)]
    sc = gd.loss_scaler
    state = sc.state.clone()
    cstate = torch.zeros(ops.GRAD_CLIP_WORDS, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.grad_clip_workspace(n) // 8, dtype=torch.float64, device=dev)
    reps = 10 * ring

    def check(i):
        ops.grad_check(grads[i % ring], state, sc.growth_factor, sc.backoff_factor, 1 << 30, sc.min_scale, sc.max_scale)

    def fused(i):
        ops.grad_check_clip(grads[i % ring], state, sc.growth_factor, sc.backoff_factor, 1 << 30, sc.min_scale, sc.max_scale,
                            cstate, 1e30, 1.0, ws)

    def static_clip(i):
        ops.grad_clip(grads[i % ring], cstate, 1e30, 1.0 / 1024, ws)
    for f in (check, fused, static_clip):
        timed(f, ring)                            # warm
    # check, fused, static, and check again: the yardstick's own spread is part of the record
    t_check, t_fused, t_static, t_check2 = timed(check, reps), timed(fused, reps), timed(static_clip, reps), timed(check, reps)
    rate = lambda t: 4.0 * n / (t * 1e-3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "what": "global-norm clipping vs none: model_vgg + dice, %d x %d, batch %d, replayed steps of four towers taking turns "
                "in one process; then ocr_grad_check_clip_f32, ocr_grad_clip_f32 and ocr_grad_check_f32 alone on a ring of "
                "flat gradient buffers" % (args.size, args.size, args.batch),
        "csrc_fingerprint": _lib.csrc_fingerprint(), "dtype": _lib.STORAGE, "device": torch.cuda.get_device_name(0),
        "steps": args.steps,
        "ms_per_step": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "static_clip_minus_static_ms": round(med["static_clip"] - med["static"], 4),
        "dynamic_clip_minus_dynamic_ms": round(med["dynamic_clip"] - med["dynamic"], 4),
        "parameters_bit_identical_after_run": same, "grad_norm_last_step": norm,
        "flat_elements": n, "ring_of_buffers": ring,
        "grad_check_us": round(t_check * 1e3, 2), "grad_check_again_us": round(t_check2 * 1e3, 2),
        "grad_check_clip_us": round(t_fused * 1e3, 2), "grad_clip_us": round(t_static * 1e3, 2),
        "grad_check_bytes_per_s": round(rate(t_check), 0), "grad_check_clip_bytes_per_s": round(rate(t_fused), 0),
        "grad_clip_bytes_per_s": round(rate(t_static), 0),
        "fused_rate_over_grad_check_rate": round(t_check / t_fused, 4),
        "static_clip_rate_over_grad_check_rate": round(t_check / t_static, 4),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
