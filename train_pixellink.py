#!/usr/bin/env python3
"""Counterpart of the reference's train_pixellink.py (flags :17-79, clone/optimiser assembly
:196-283) on the MI355X path: one process per GPU ("clone")

    python train_pixellink.py --dataset_dir /data/icdar2015/train --batch_size 32 --num_gpus 1
    python train_pixellink.py --num_gpus 2 ...        (starts the two clones itself)
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 train_pixellink.py --num_gpus 2 ...

Same flag names and defaults where they bear on the step: `PixelLinkNet` + `build_loss`
(nets/pixellink.py), each clone's loss divided by num_clones (:264) and the gradients SUMMED
(`sum_gradients`, :179-194: `TrainStep(grad_op="sum")` seeds the backward pass with 1/num_clones and
all-reduces with SUM), Momentum 0.9,
`tf.case` staircase on --lr_breakpoints / --lr_decays (:222-237), weight decay 5e-4.

Data: the reference reads TFRecords through `datasets.dataset_factory` / `ssd_vgg_preprocessing`,
neither of which is in its tree (not runnable as shipped).  Here --dataset_dir is an
ICDAR directory (images + gt_*.txt); every image is resized to the train size on the GPU and its
quads go, normalised, through `pixellink_fn.generate_rbox` (tool/pixellink_fn.py:53-110) — the label
generator this script's `tf_pixellink_get_rbox` wraps.  Without --dataset_dir: synthetic batches.

Not in the reference: `--eval_data_path DIR --eval_steps N` evaluates a held-out directory (images + gt_*.txt) between steps
every N optimiser steps, on the device and outside the recorded step (tensorflow_ocr_amd/evaluate.py: LinkEvaluator), and
reports precision / recall / hmean; `--eval_map_scales 0.5,1,2 [--eval_flip]` makes every such pass a multi-scale / flip
test by score-map fusion."""
import argparse
import os
import time

import numpy as np
import torch

from tensorflow_ocr_amd import cli
from tensorflow_ocr_amd.cli import window as _window


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--train_with_ignored', action='store_true')
    ap.add_argument('--train_dir', type=str, default=None)
    ap.add_argument('--checkpoint_path', type=str, default=None)
    ap.add_argument('--batch_size', type=int, default=32, help='global batch over all clones')
    ap.add_argument('--num_gpus', type=int, default=1)
    ap.add_argument('--max_number_of_steps', type=int, default=60000)
    ap.add_argument('--log_every_n_steps', type=int, default=10)
    ap.add_argument('--learning_rate', type=float, default=0.01)
    ap.add_argument('--lr_policy', type=str, default='staircase')
    ap.add_argument('--lr_breakpoints', type=str, default='20000,40000,60000')
    ap.add_argument('--lr_decays', type=str, default='0.1,0.01,0.001')
    ap.add_argument('--momentum', type=float, default=0.9)
    ap.add_argument('--weight_decay', type=float, default=0.0005)
    ap.add_argument('--using_moving_average', action='store_true')
    ap.add_argument('--moving_average_decay', type=float, default=0.9999)
    ap.add_argument('--num_readers', type=int, default=32)
    ap.add_argument('--dataset_dir', type=str, default=None)
    ap.add_argument('--train_image_width', type=int, default=512)
    ap.add_argument('--train_image_height', type=int, default=512)
    # not a reference flag (the reference's slim.learning.train writes its summaries on a timer): every N optimiser steps
    # rank 0 adds the loss, the learning rate and the input image to a TensorBoard event file in --train_dir (and what
    # --summary_variables adds).  0 = off: no event file.
    ap.add_argument('--save_summary_steps', type=int, default=0)
    cli.add_step_flags(ap, '--batch_size')
    # not a reference flag: the pixel loss.  'mean' is what the reference's build_loss computes (nets/pixellink.py:160, the
    # mean CE over all pixels); 'instance_balanced' is the paper's loss the reference left commented out (:138-168,
    # :191-192): every text instance weighs the same, --max_neg_pos_ratio hardest negatives per positive are mined, `###`
    # regions train nothing (losses.balanced_loss; build-defined).
    ap.add_argument('--pixel_loss', choices=('mean', 'instance_balanced'), default='mean')
    # config.max_neg_pos_ratio (nets/pixellink.py:116); read by --pixel_loss instance_balanced only
    ap.add_argument('--max_neg_pos_ratio', type=_neg_ratio_arg, default=3.0)
    # between-steps evaluation on a LinkEvaluator: the images are resized to --eval_image_height x --eval_image_width and go
    # through forward -> link components -> boxes -> matching; --eval_weights ema needs --using_moving_average; --eval_sweep's
    # order key is the component's mean pixel score, in [0, 1]
    cli.add_train_eval_flags(ap)
    ap.add_argument('--eval_image_width', type=int, default=1280)
    ap.add_argument('--eval_image_height', type=int, default=768)
    # --eval_map_scales S1,S2,... [--eval_flip]: multi-scale / flip testing of every pass by score-map fusion (the flags
    # --map_scales / --flip of eval_pixellink_fast.py: evaluate.LinkEvaluator's map_scales / flip; build-defined, its effect
    # on the F-measure unmeasured; activation memory grows with the square of the largest scale)
    ap.add_argument('--eval_map_scales', type=cli.map_scales_arg, default=None, metavar='S1,S2,...')
    ap.add_argument('--eval_flip', action='store_true')
    # --eval_grid_pixel LIST --eval_grid_link LIST: every pass also decodes and matches every (pixel, link) threshold pair of
    # the two lists behind its one forward (evaluate.LinkEvaluator's grid; the flags of eval_pixellink_fast.py) and reports
    # the best pair: eval/grid_best_hmean, eval/grid_best_pixel_threshold, eval/grid_best_link_threshold in the event file
    cli.add_grid_flags(ap)
    FLAGS = ap.parse_args(argv)
    if (FLAGS.eval_map_scales is not None or FLAGS.eval_flip) and not cli.eval_on(FLAGS):
        ap.error('--eval_map_scales and --eval_flip need --eval_data_path and --eval_steps')
    if cli.check_grid_flags(ap, FLAGS) is not None and not cli.eval_on(FLAGS):
        ap.error('--eval_grid_pixel and --eval_grid_link need --eval_data_path and --eval_steps')
    cli.check_train_eval_flags(ap, FLAGS, FLAGS.using_moving_average, '--eval_weights ema needs --using_moving_average')
    return FLAGS


def _neg_ratio_arg(text):
    v = float(text)
    if not v >= 0.0:
        raise argparse.ArgumentTypeError('--max_neg_pos_ratio must be a number >= 0, got %r' % text)
    return v


def staircase_lr(step, base, breakpoints, decays):
    """train_pixellink.py:222-237: tf.case over (step < breakpoint_i -> decay_i), default 1.0."""
    for bp, dc in zip(breakpoints, decays):
        if step < bp:
            return base * dc
    return base * 1.0


# The input normalisation of the reference's pipeline (train_pixellink.py:150-154 hands the queue
# `ssd_vgg_preprocessing` output): (x - 120) / 60, applied by the net's image-preparation kernel
INPUT_NORM = (120.0, 60.0)


def dataset_batches(FLAGS, g, batch, rank):
    """ICDAR directory -> (images [B,H,W,3] f32, pixel labels [B,H/4,W/4], link labels [B,H/4,W/4,8]) and, with
    --pixel_loss instance_balanced, the weight map [B,H/4,W/4] (the `###` tags zero their instances there)."""
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.tool import pixellink_fn
    H, W = FLAGS.train_image_height, FLAGS.train_image_width
    files = sorted(icdar.get_images(FLAGS.dataset_dir))
    rng = np.random.RandomState(1000 + rank)
    while True:
        rng.shuffle(files)
        ims, xs_l, ys_l, bb_l, ig_l = [], [], [], [], []
        for fn in files:
            tf = icdar.txt_name(fn)
            if not os.path.exists(tf):
                continue
            im = icdar.read_image_rgb(fn)
            h, w, _ = im.shape
            polys, tags = icdar.load_annoataion(tf)
            polys, tags = icdar.check_and_validate_polys(polys, tags, (h, w))
            if len(polys) == 0:
                continue
            xs, ys = polys[:, :, 0] / w, polys[:, :, 1] / h
            ims.append(im)
            xs_l.append(xs)
            ys_l.append(ys)
            bb_l.append(np.stack([ys.min(1), xs.min(1), ys.max(1), xs.max(1)], 1))
            ig_l.append(tags.astype(np.int32))
            if len(ims) == batch:
                if H == W:
                    images = icdar.resize_images(ims, H, graph=g)
                else:
                    raise SystemExit('square train size only (resize_images)')
                if FLAGS.pixel_loss == 'instance_balanced':
                    score, link, _, weight = pixellink_fn.generate_rbox_batch(H, W, xs_l, ys_l, bb_l, ig_l, graph=g,
                                                                              weights=True)
                    yield images, score, link, weight
                else:
                    score, link, _ = pixellink_fn.generate_rbox_batch(H, W, xs_l, ys_l, bb_l, ig_l, graph=g)
                    yield images, score, link
                ims, xs_l, ys_l, bb_l, ig_l = [], [], [], [], []


def synthetic_weights(ids, device, rects=8):
    """The instance-balanced weight map of a synthetic batch: `ids` (synthetic.make_batch(return_ids=True)) is its own
    label-resolution owner map, so `ids * 257` is a cover raster (first = last = owner) and the weights entry runs on it
    without resampling."""
    from tensorflow_ocr_amd import ops
    n, h, w = ids.shape
    cover = torch.from_numpy(ids * 257).to(device=device, dtype=torch.int32)
    area = torch.empty((n, rects), dtype=torch.int32, device=device)
    weight = torch.empty((n, h, w), dtype=torch.float32, device=device)
    ops.pixellink_instance_weights(cover, torch.zeros((n, rects), dtype=torch.uint8, device=device), h, w, area, weight)
    return weight


def make_train_eval(FLAGS, g, step):
    """The between-steps evaluation of --eval_data_path / --eval_steps (None when off): PixelLinkNet on the training graph
    (it has no batch norm: the inference forward is the training forward without a loss) with the weights --eval_weights
    names, its logits decoded by evaluate.LinkEvaluator."""
    if not (FLAGS.eval_steps > 0 and FLAGS.eval_data_path):
        return None
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.nets import pixellink

    def network(gr, im):
        net = pixellink.PixelLinkNet(im, graph=gr, input_norm=INPUT_NORM)
        return net.pixel_cls, net.link_cls
    return evaluate.TrainEval(g, step, network, FLAGS.eval_data_path, FLAGS.eval_steps, max_images=FLAGS.eval_max_images,
                              weights=FLAGS.eval_weights, batch_size=max(1, int(FLAGS.batch_size / FLAGS.num_gpus)),
                              evaluator=evaluate.LinkEvaluator, eval_image_height=FLAGS.eval_image_height,
                              eval_image_width=FLAGS.eval_image_width, protocol=FLAGS.eval_protocol,
                              sweep=FLAGS.eval_sweep, map_scales=FLAGS.eval_map_scales, flip=FLAGS.eval_flip,
                              grid=cli.grid_option(FLAGS))


def _evaluate(train_eval, summaries, opt):
    cli.report_eval(train_eval, summaries, opt, 'global step {:d}: ')       # ... and the line eval_pixellink_fast.py prints


def main():
    FLAGS = parse()
    from tensorflow_ocr_amd import launch
    rc = launch.self_launch(FLAGS.num_gpus)          # plain start with --num_gpus N: become the launcher
    if rc is not None:
        raise SystemExit(rc)
    from tensorflow_ocr_amd import checkpoint, dist, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.train import MomentumOptimizer, TrainStep
    rank, world, local = dist.init_process_group_from_env()
    if world != FLAGS.num_gpus:
        raise SystemExit('--num_gpus %d but WORLD_SIZE=%d' % (FLAGS.num_gpus, world))
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    batch_size_per_gpu = int(FLAGS.batch_size / FLAGS.num_gpus)          # :92
    bps = [int(o) for o in FLAGS.lr_breakpoints.split(',')]
    dcs = [float(o) for o in FLAGS.lr_decays.split(',')]
    assert len(bps) == len(dcs)
    if FLAGS.lr_policy != 'staircase':
        raise SystemExit('Unkonw lr_policy: {}'.format(FLAGS.lr_policy))

    g = Graph(device, loss_scale=FLAGS.loss_scale, seed=1)

    balanced = FLAGS.pixel_loss == 'instance_balanced'

    def forward_loss(gr, im, pixel_labels, link_labels, pixel_weights=None):
        net = pixellink.PixelLinkNet(im, graph=gr, input_norm=INPUT_NORM)   # raw images in
        return net.build_loss(pixel_labels, link_labels, pixel_weights=pixel_weights,   # 2*pixel + link (two LOSSES, :263)
                              neg_ratio=FLAGS.max_neg_pos_ratio)

    def make_opt(gr):
        opt = MomentumOptimizer(gr, base_lr=FLAGS.learning_rate, momentum=FLAGS.momentum,
                                weight_decay=FLAGS.weight_decay,
                                moving_average_decay=FLAGS.moving_average_decay if FLAGS.using_moving_average else None,
                                clip_norm=FLAGS.clip_norm)
        opt.learning_rate = lambda: staircase_lr(opt.global_step, FLAGS.learning_rate, bps, dcs)
        return opt
    step = TrainStep(g, forward_loss, make_opt, world_size=world, grad_op="sum", accumulate_steps=FLAGS.accumulate_steps)

    feeder = None
    if FLAGS.dataset_dir and os.path.isdir(FLAGS.dataset_dir):
        from tensorflow_ocr_amd.feeder import DeviceFeeder
        feeder = DeviceFeeder(lambda: dataset_batches(FLAGS, g, batch_size_per_gpu, rank), device, depth=2)
    rng = np.random.default_rng(1000 + rank)
    if FLAGS.train_dir and rank == 0:
        os.makedirs(FLAGS.train_dir, exist_ok=True)
    if FLAGS.save_summary_steps > 0 and not FLAGS.train_dir:
        raise SystemExit('--save_summary_steps needs --train_dir (where the event file goes)')
    start = time.time()
    last = [None]
    def next_batch():
        if feeder is not None:
            last[0] = next(feeder)
        else:
            im, px, lk, _, ids = synthetic.make_batch(rng, batch_size_per_gpu, FLAGS.train_image_height, return_ids=True)
            last[0] = [torch.from_numpy(a).to(device, non_blocking=True) for a in (im, px[..., 0], lk)]
            if balanced:
                last[0].append(synthetic_weights(ids, device))
        return last[0]
    summaries = None
    train_eval = make_train_eval(FLAGS, g, step) if rank == 0 else None
    for it in range(FLAGS.max_number_of_steps):
        loss = _window(step, FLAGS.accumulate_steps, next_batch)
        if rank == 0 and FLAGS.save_summary_steps > 0 and it % FLAGS.save_summary_steps == 0:
            if summaries is None:            # (the flat buffers exist once the first step has run)
                from tensorflow_ocr_amd.summary import TrainingSummaries
                summaries = TrainingSummaries(FLAGS.train_dir, step, variables=FLAGS.summary_variables)
            scalars = {'total_loss': loss.item(), 'learning_rate': step.opt.learning_rate()}
            scalars.update(cli.grad_factor_scalars(step.opt))
            summaries.write(step.opt.global_step, scalars, [('input', last[0][0][0])])
        if train_eval is not None and train_eval.due(it + 1):
            _evaluate(train_eval, summaries, step.opt)
        if it % FLAGS.log_every_n_steps == 0:
            v = loss.item()
            dt = (time.time() - start) / FLAGS.log_every_n_steps
            start = time.time()
            if rank == 0:
                print('global step %d: loss = %.4f (%.3f sec/step), lr %.6f' % (
                    it, v, dt, staircase_lr(it, FLAGS.learning_rate, bps, dcs)), flush=True)
                cli.log_grad_factor(step.opt)
            if dist.any_rank(bool(np.isnan(v))):     # collective: no rank leaves the all-reduce alone
                break
        if FLAGS.train_dir and rank == 0 and it > 0 and it % 1000 == 0:
            checkpoint.save_training_state(FLAGS.train_dir, g, step.opt)
    if summaries is not None:
        summaries.close()
    if feeder is not None:
        feeder.close()


if __name__ == '__main__':
    main()
