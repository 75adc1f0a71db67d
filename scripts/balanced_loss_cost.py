#!/usr/bin/env python3
"""What PixelLink's instance-balanced loss (train_pixellink.py --pixel_loss instance_balanced) costs against the mean loss
on the PixelLink training configuration: VGG-16 `PixelLinkNet`, 512 x 512, batch 32, one GPU.

    python scripts/balanced_loss_cost.py [--steps 40] [--warmup 6] [--batch 32] [--size 512] [--out profiles/balanced_loss.json]

In ONE process two towers of the same seed take turns, four replayed steps each, every block between a pair of HIP
events: `mean` (build_loss as the reference has it) and `instance_balanced` (build_loss(pixel_weights=...)).  Each arm is
held twice (mean, balanced, mean_again, balanced_again): the distance between the two copies of an arm is the spread a
difference between the arms has to be read against.  Then the two forward entries and the two backward entries are
event-timed alone on the towers' own logits and labels, and the weight-map entry alone on a label-resolution cover.  The
result is written with the fingerprint of the kernel sources it was measured on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_step(device, balanced, batch, size):
    import train_pixellink
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.train import MomentumOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=1)
    im, px, lk, _, ids = synthetic.make_batch(np.random.default_rng(100), batch, size, return_ids=True)
    data = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (im, px[..., 0], lk)]
    if balanced:
        data.append(train_pixellink.synthetic_weights(ids, device))
    nets = []

    def fl(gr, im, px, lk, wt=None):
        net = pixellink.PixelLinkNet(im, graph=gr, input_norm=train_pixellink.INPUT_NORM)
        nets[:] = [net]
        return net.build_loss(px, lk, pixel_weights=wt)
    step = TrainStep(g, fl, lambda gr: MomentumOptimizer(gr, base_lr=0.01, momentum=0.9, weight_decay=5e-4))
    return g, data, step, nets, ids


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "balanced_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("balanced_loss_cost.py measures on the GPU: none found")
    from tensorflow_ocr_amd import _lib, ops
    from tensorflow_ocr_amd._lib import BalancedLossDesc, SoftmaxLossDesc
    dev = torch.device("cuda", 0)
    arms = [("mean", False), ("instance_balanced", True), ("mean_again", False), ("instance_balanced_again", True)]
    towers = {name: make_step(dev, bal, args.batch, args.size) for name, bal in arms}
    for _ in range(3 + args.warmup):
        for g, d, s, _, _ in towers.values():
            s(*d)
    torch.cuda.synchronize()
    assert all(s.plan is not None for _, _, s, _, _ in towers.values())
    ms = {name: [] for name in towers}
    B = 4                                         # steps per timed block: the queue stays full inside a block
    for _ in range(max(1, args.steps // B)):      # the arms in turn: drift hits all alike
        for name, (g, d, s, _, _) in towers.items():
            ms[name].append(timed(lambda i: [s(*d) for _ in range(B)], 1) / B)
    losses = {name: float(s.loss.item()) for name, (_, _, s, _, _) in towers.items()}

    # the loss entries alone, on the balanced tower's logits and labels
    g, d, s, nets, ids = towers["instance_balanced"]
    pl, ll = nets[0].pixel_cls.data, nets[0].link_cls.data
    n, h, w, _ = pl.shape
    _, px, lk, wt = d
    thr, sums, out = (torch.empty(k, dtype=torch.float32, device=dev) for k in (n, 34, 10))
    dpl, dll = torch.empty_like(pl), torch.empty_like(ll)
    bd = BalancedLossDesc(n, h * w, 0, 3.0, 0.25, 2.0)
    md = SoftmaxLossDesc(n, h * w, 2, 1, 0, 0, 3.0, 0.25, 2.0)
    cover = torch.from_numpy(ids * 257).to(device=dev, dtype=torch.int32)
    ign = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    area = torch.empty((n, 8), dtype=torch.int32, device=dev)
    wmap = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    alone = {
        "balanced_loss_fwd": lambda i: ops.balanced_loss_fwd(bd, pl, ll, px, lk, wt, thr, sums, out, g.workspace()),
        "softmax_loss_fwd_mean": lambda i: ops.softmax_loss_fwd(md, pl, ll, px, lk, thr, sums, out, g.workspace()),
        "balanced_loss_bwd": lambda i: ops.balanced_loss_bwd(bd, pl, ll, px, lk, wt, thr, sums, 1024.0, dpl, dll),
        "softmax_loss_bwd_mean": lambda i: ops.softmax_loss_bwd(md, pl, ll, px, lk, thr, sums, 1024.0, dpl, dll),
        "pixellink_instance_weights": lambda i: ops.pixellink_instance_weights(cover, ign, h, w, area, wmap),
    }
    us = {}
    for name in ("balanced_loss_fwd", "balanced_loss_bwd", "softmax_loss_fwd_mean", "softmax_loss_bwd_mean",
                 "pixellink_instance_weights"):
        timed(alone[name], 10)                    # warm
        us[name] = round(timed(alone[name], 200) * 1e3, 2)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "what": "PixelLinkNet VGG-16 %d x %d, batch %d, Momentum: --pixel_loss mean vs instance_balanced, replayed steps of "
                "four towers (each arm twice) taking turns in one process; then the loss entries and the weight-map entry "
                "alone, median of 200 event-timed calls" % (args.size, args.size, args.batch),
        "csrc_fingerprint": _lib.csrc_fingerprint(), "dtype": _lib.STORAGE, "device": torch.cuda.get_device_name(0),
        "steps": args.steps,
        "ms_per_step": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "balanced_minus_mean_ms": round(med["instance_balanced"] - med["mean"], 4),
        "balanced_again_minus_mean_again_ms": round(med["instance_balanced_again"] - med["mean_again"], 4),
        "same_arm_spread_ms": {"mean": round(abs(med["mean_again"] - med["mean"]), 4),
                               "instance_balanced": round(abs(med["instance_balanced_again"] - med["instance_balanced"]), 4)},
        "last_loss": losses,
        "entries_alone_us": us,
    }
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
