#!/usr/bin/env python3
"""Counterpart of the reference's multigpu_train.py (flags :6-17, tower/step assembly :27-142, hot
loop :169-194) on the MI355X path: one process per GPU

    python multigpu_train.py --gpu_list 0 --batch_size_per_gpu 14 --input_size 512
    python multigpu_train.py --gpu_list 0,1           (starts one rank per listed GPU itself)
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 multigpu_train.py --gpu_list 0,1

Same flag names and defaults; `--net` selects the graph (`model` = nets/model.py ResNet-50 +
PixelLink heads + OHNM loss, the one the reference script imports; `model_vgg` / `east` /
`pixellink` the others).  Data: `--training_data_path` (the reference's icdar.py flag) feeds ICDAR
images + gt_*.txt through datasets/icdar.get_batch — host decode in `--num_readers` processes,
upload + resize + label maps on the feeder's HIP stream, overlapped with the step; without it (or
with an empty directory) batches are synthetic (`tensorflow_ocr_amd.synthetic`).  Every
`--save_summary_steps` optimiser steps rank 0 adds scalars and images (and, with
`--summary_variables`, per-variable histograms) to a TensorBoard event file in `--checkpoint_path`.  `--augment east`
`--net east --geometry RBOX` trains EAST's RBOX heads (`model_vgg_16.model_rbox` / `loss_rbox`, distances x `--text_scale`)
on RBOX label maps made on the device from the same ICDAR polygons (or `synthetic.rbox_labels` without data) — the head
`test.py --geometry RBOX` runs; with `--eval_data_path DIR --eval_steps N` rank 0 evaluates that directory (images +
gt_*.txt) between steps every N optimiser steps, on the device and outside the recorded step (tensorflow_ocr_amd/evaluate.py),
and reports precision / recall / hmean.  `--augment east`
(or `pixellink`, or key=value,...) turns on the augmentation the reference keeps disabled
(datasets/icdar.py:576-615), warped on the device in one launch per batch.  The stdout line
format is the reference's (:183-184)."""
import argparse
import os
import time

import numpy as np
import torch

from tensorflow_ocr_amd import cli
from tensorflow_ocr_amd.cli import window as _window


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--input_size', type=int, default=512)
    ap.add_argument('--batch_size_per_gpu', type=int, default=14)
    ap.add_argument('--num_readers', type=int, default=16)
    ap.add_argument('--learning_rate', type=float, default=0.0001)
    ap.add_argument('--max_steps', type=int, default=100000)
    ap.add_argument('--moving_average_decay', type=float, default=0.997)
    ap.add_argument('--gpu_list', type=str, default='1')
    ap.add_argument('--checkpoint_path', type=str, default='/tmp/east_resnet_v1_50_rbox/')
    ap.add_argument('--restore', action='store_true')
    ap.add_argument('--save_checkpoint_steps', type=int, default=1000)
    ap.add_argument('--save_summary_steps', type=int, default=20)
    ap.add_argument('--pretrained_model_path', type=str, default=None)
    ap.add_argument('--training_data_path', type=str, default='/data/ocr/icdar2015/')
    ap.add_argument('--net', choices=['model', 'model_vgg', 'east', 'pixellink'], default='model')
    cli.add_step_flags(ap, '--batch_size_per_gpu')
    # the augmentation the reference keeps disabled (datasets/icdar.py:576-615), on the device: none | east | pixellink |
    # key=value,... (datasets/augment.py: Augment.parse).  Only with --training_data_path; synthetic batches have none.
    ap.add_argument('--augment', type=_augment_arg, default=None, metavar='SPEC')
    # not a flag of this reference script (EAST's own has the head built in): link = the PixelLink-style 8 link maps the
    # reference trains; RBOX = EAST's score + four distances + angle (--net east only), labels from the same polygons
    ap.add_argument('--geometry', choices=['link', 'RBOX'], default='link')
    ap.add_argument('--text_scale', type=int, default=512, help="RBOX only: the distance scale of the geometry head "
                    "(the reference's nets/model.py flag)")
    # between-steps evaluation, --net east --geometry RBOX only; --eval_sweep's order key is LANMS's merged score (a sum of
    # pixel scores, not a probability)
    cli.add_train_eval_flags(ap)
    # --eval_scales 0.5,1,2: multi-scale testing in every pass — one forward per scale, the per-scale detections pooled and
    # fused on the device (evaluate.Evaluator's scales); --eval_fuse: nms = score-ordered suppression, vote = score-weighted
    # coordinates.  The detection score (and --eval_sweep's threshold) is then the mean pixel score, in [0, 1]
    ap.add_argument('--eval_scales', type=cli.scales_arg, default=None, metavar='S1,S2,..')
    ap.add_argument('--eval_fuse', choices=['nms', 'vote'], default='nms')
    FLAGS = ap.parse_args(argv)
    if FLAGS.eval_scales is not None and not cli.eval_on(FLAGS):
        ap.error('--eval_scales needs --eval_data_path and --eval_steps')
    if FLAGS.eval_fuse != 'nms' and FLAGS.eval_scales is None:
        ap.error('--eval_fuse needs --eval_scales')
    rbox = FLAGS.net == 'east' and FLAGS.geometry == 'RBOX'
    cli.check_train_eval_flags(
        ap, FLAGS, FLAGS.moving_average_decay, '--eval_weights ema needs a --moving_average_decay',
        after_sweep=[(FLAGS.eval_protocol != 'raster' and not cli.eval_on(FLAGS),
                      '--eval_protocol needs --eval_data_path and --eval_steps'),
                     (FLAGS.geometry == 'RBOX' and FLAGS.net != 'east',
                      '--geometry RBOX needs --net east (the RBOX heads sit on the EAST merge branch)')],
        before_ema=[((FLAGS.eval_steps > 0 or FLAGS.eval_data_path) and not rbox,
                     '--eval_data_path / --eval_steps need --net east --geometry RBOX (the evaluation decodes RBOX maps)')])
    return FLAGS


def _augment_arg(text):
    from tensorflow_ocr_amd.datasets.augment import Augment
    try:
        return Augment.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def build_forward_loss(net, geometry='link', text_scale=512):
    from tensorflow_ocr_amd.nets import model, model_vgg_16, pixellink
    if geometry == 'RBOX':
        if net != 'east':
            raise ValueError("geometry 'RBOX' needs net 'east'")

        def f(g, im, sm, gm, tm):
            a, b = model_vgg_16.model_rbox(im, is_training=True, text_scale=text_scale, graph=g)
            return model_vgg_16.loss_rbox(sm, a, gm, b, tm, graph=g)
    elif net == 'model':
        def f(g, im, sm, gm, tm):
            a, b = model.model(im, is_training=True, graph=g)
            return model.loss(sm, a, gm, b, tm, graph=g)
    elif net == 'model_vgg':
        def f(g, im, sm, gm, tm):
            a, b = model_vgg_16.model_vgg(im, is_training=True, graph=g)
            return model_vgg_16.loss(sm, a, gm, b, tm, graph=g)
    elif net == 'east':
        def f(g, im, sm, gm, tm):
            a, b = model_vgg_16.model(im, is_training=True, graph=g)
            return model_vgg_16.loss(sm, a, gm, b, tm, graph=g)
    else:
        def f(g, im, sm, gm, tm):
            # raw images in; the pipeline's (x - 120) / 60 runs inside the image-preparation kernel
            n = pixellink.PixelLinkNet(im, graph=g, input_norm=(120.0, 60.0))
            return n.build_loss(sm[..., 0], gm)
    return f


def main():
    FLAGS = parse()
    gpus = FLAGS.gpu_list.split(',')
    # os.environ['CUDA_VISIBLE_DEVICES'] = FLAGS.gpu_list (multigpu_train.py:90) + one tower per entry
    # (:118-130).  Started plainly, this process either IS the single tower or becomes the launcher of
    # len(gpus) ranks; nothing has touched HIP yet.
    from tensorflow_ocr_amd import launch
    if 'WORLD_SIZE' not in os.environ:
        if len(gpus) > 1:
            raise SystemExit(launch.self_launch(len(gpus), visible=FLAGS.gpu_list))
        os.environ.setdefault('HIP_VISIBLE_DEVICES', FLAGS.gpu_list)
    from tensorflow_ocr_amd import checkpoint, dist, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    rank, world, local = dist.init_process_group_from_env()
    if world not in (1, len(gpus)):
        raise SystemExit("gpu_list has %d entries but WORLD_SIZE=%d" % (len(gpus), world))
    device = torch.device('cuda', local)     # the launcher maps LOCAL_RANK -> visible GPU
    torch.cuda.set_device(device)
    if rank == 0:
        os.makedirs(FLAGS.checkpoint_path, exist_ok=True)

    g = Graph(device, loss_scale=FLAGS.loss_scale, seed=1)
    step = TrainStep(g, build_forward_loss(FLAGS.net, FLAGS.geometry, FLAGS.text_scale),
                     lambda gr: AdamOptimizer(gr, learning_rate=FLAGS.learning_rate,
                                              moving_average_decay=FLAGS.moving_average_decay,
                                              clip_norm=FLAGS.clip_norm),
                     world_size=world, accumulate_steps=FLAGS.accumulate_steps)
    rng = np.random.default_rng(1000 + rank)
    feeder = None
    if os.path.isdir(FLAGS.training_data_path):
        from tensorflow_ocr_amd.datasets import icdar
        if icdar.get_images(FLAGS.training_data_path):
            # multigpu_train.py:164-167: icdar.get_batch(num_workers, input_size, batch_size)
            feeder = icdar.get_batch(num_workers=FLAGS.num_readers, training_data_path=FLAGS.training_data_path,
                                     input_size=FLAGS.input_size, batch_size=FLAGS.batch_size_per_gpu,
                                     graph=g, seed=1000 + rank, augment=FLAGS.augment, geometry=FLAGS.geometry)
    start = time.time()
    try:
        _train_loop(FLAGS, g, step, feeder, rng, rank, world, device, start)
    finally:
        if feeder is not None:
            feeder.close()


def _next_batch(FLAGS, feeder, rng, device):
    from tensorflow_ocr_amd import synthetic
    if feeder is not None:
        images, _, score_maps, geo_maps, training_masks = next(feeder)
        return [images, score_maps, geo_maps, training_masks]
    data = synthetic.make_batch(rng, FLAGS.batch_size_per_gpu, FLAGS.input_size)
    if FLAGS.geometry == 'RBOX':
        data = [data[0]] + list(synthetic.rbox_labels(FLAGS.batch_size_per_gpu, FLAGS.input_size, rng))
    return [torch.from_numpy(a).to(device, non_blocking=True) for a in data]


def _train_loop(FLAGS, g, step, feeder, rng, rank, world, device, start):
    from tensorflow_ocr_amd import checkpoint, dist
    batch = _next_batch(FLAGS, feeder, rng, device)
    # variables, optimiser slots and EMA shadows exist before the first update, so a checkpoint is
    # restored (:153-158) / the pretrained backbone loaded (:149-151,161-162) BEFORE it, as in the reference
    step.build(*batch)
    opt = step.opt
    src = FLAGS.checkpoint_path if FLAGS.restore else FLAGS.pretrained_model_path
    if src:
        if not (os.path.isdir(src) and os.path.exists(os.path.join(src, 'checkpoint')) or os.path.exists(src + '.index')
                or os.path.isfile(src)):
            raise FileNotFoundError('no checkpoint at %s' % src)
        if FLAGS.restore:
            checkpoint.restore_training_state(src, g, opt)
            if opt.restored_variables == 0:
                raise ValueError('no variable of this graph found in %s' % src)
            if rank == 0:
                print('continue training from previous checkpoint (%d variables)' % opt.restored_variables)
        else:
            sd, _ = checkpoint.load_tf_checkpoint(src)        # variables only (slim.assign_from_checkpoint_fn)
            g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, sd), strict=False)
            if opt.ema is not None:
                opt.ema.copy_(g.store.flat)
            if rank == 0:
                print('loaded ' + src)
    # `for step in range(FLAGS.max_steps)` (multigpu_train.py:168): the loop counter is separate from the restored
    # `global_step` (which the optimiser continues from), so a resumed run takes max_steps MORE steps
    K = FLAGS.accumulate_steps
    first = [batch]
    last = [batch]

    def next_batch():
        last[0] = first.pop() if first else _next_batch(FLAGS, feeder, rng, device)
        return last[0]
    summaries = None
    if rank == 0 and FLAGS.save_summary_steps > 0:
        # summary_writer = tf.summary.FileWriter(FLAGS.checkpoint_path, ...) (multigpu_train.py:145)
        from tensorflow_ocr_amd.summary import TrainingSummaries
        summaries = TrainingSummaries(FLAGS.checkpoint_path, step, variables=FLAGS.summary_variables)
    train_eval = make_train_eval(FLAGS, g, step) if rank == 0 else None
    try:
        _steps(FLAGS, g, step, opt, K, next_batch, last, summaries, rank, world, start, train_eval)
    finally:
        if summaries is not None:
            summaries.close()


def _write_summaries(summaries, g, opt, loss, batch):
    """multigpu_train.py:49-65,105-106,135-136 on the step just taken (the reference runs a second train step for it,
    :189-194): behind the window's closing call, so store.flat_grad holds that optimiser step's gradients."""
    ml = loss.item()
    scalars = {'model_loss': ml, 'total_loss': ml + opt.regularization_loss().item(), 'learning_rate': opt.learning_rate()}
    scalars.update(cli.grad_factor_scalars(opt))
    images, score_maps, geo_maps = batch[0], batch[1], batch[2]
    summaries.write(opt.global_step, scalars, [('input', images[0]), ('score_map', score_maps[0]),
                                               ('geo_map_0', geo_maps[0][..., 0:1])])


def make_train_eval(FLAGS, g, step, blocks=None):
    """The between-steps evaluation of --eval_data_path / --eval_steps (None when off): model_rbox in inference mode on
    the training graph — batch norm on the moving statistics — with the weights --eval_weights names.  `blocks`: a smaller
    trunk (tests)."""
    if not (FLAGS.eval_steps > 0 and FLAGS.eval_data_path):
        return None
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.nets import model_vgg_16

    def network(gr, im):
        return model_vgg_16.model_rbox(im, is_training=False, text_scale=FLAGS.text_scale, graph=gr, blocks=blocks)
    return evaluate.TrainEval(g, step, network, FLAGS.eval_data_path, FLAGS.eval_steps, max_images=FLAGS.eval_max_images,
                              weights=FLAGS.eval_weights, batch_size=FLAGS.batch_size_per_gpu,
                              protocol=FLAGS.eval_protocol, sweep=FLAGS.eval_sweep, scales=FLAGS.eval_scales,
                              fuse=FLAGS.eval_fuse)


def _evaluate(train_eval, summaries, opt):
    cli.report_eval(train_eval, summaries, opt, 'Step {:06d}, ')       # ... and the line test.py prints


def _steps(FLAGS, g, step, opt, K, next_batch, last, summaries, rank, world, start, train_eval=None):
    from tensorflow_ocr_amd import checkpoint, dist
    for it in range(FLAGS.max_steps):
        loss = _window(step, K, next_batch)
        if summaries is not None and it % FLAGS.save_summary_steps == 0:
            _write_summaries(summaries, g, opt, loss, last[0])
        if train_eval is not None and train_eval.due(it + 1):
            _evaluate(train_eval, summaries, opt)
        if it % 10 == 0:
            ml = loss.item()
            # the stop decision is collective: a rank leaving alone would strand the others in the
            # next gradient all-reduce
            if dist.any_rank(bool(np.isnan(ml))):
                if rank == 0:
                    print('Loss diverged, stop training')
                break
            avg_time_per_step = (time.time() - start) / 10
            avg_examples_per_second = (10 * K * FLAGS.batch_size_per_gpu * world) / (time.time() - start)
            start = time.time()
            if rank == 0:
                # total_loss = model_loss + sum(REGULARIZATION_LOSSES) (multigpu_train.py:36)
                tl = ml + opt.regularization_loss().item()
                print('Step {:06d}, model loss {:.4f}, total loss {:.4f}, {:.2f} seconds/step, {:.2f} examples/second'.format(
                    it, ml, tl, avg_time_per_step, avg_examples_per_second), flush=True)
                cli.log_grad_factor(opt)
        if rank == 0 and it % FLAGS.save_checkpoint_steps == 0:     # step 0 included (multigpu_train.py:185-186)
            # saver.save(sess, FLAGS.checkpoint_path + 'model.ckpt', global_step=global_step) (:186-187):
            # a TensorFlow V2 bundle of Saver(tf.global_variables()) — variables, EMA shadows, Adam slots
            checkpoint.save_training_state(FLAGS.checkpoint_path, g, opt)


if __name__ == '__main__':
    main()
