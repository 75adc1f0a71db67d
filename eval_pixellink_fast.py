#!/usr/bin/env python3
"""Held-out evaluation of the decode test_pixellink_fast.py runs (not in the reference, which writes boxes and never
scores them): the images of --test_data_path go through PixelLinkNet at --eval_image_height x --eval_image_width, link-gated
connected components at 1/4 resolution, one box per component with the component's mean pixel score, and the reference's
raster-IoU matching (tool/bboxes.py:171-240; not the official ICDAR-2015 protocol) against the `gt_<name>.txt` files of
--gt_path (ICDAR layout, `###` = ignored) — per batch one chain on the device, one read of the counters at its end
(tensorflow_ocr_amd.evaluate.LinkEvaluator).  One line is printed:

    precision .. recall .. hmean .. (gt .. det ..)

    python eval_pixellink_fast.py --checkpoint_path /tmp/pixellink/ --test_data_path ./images --gt_path ./gt
    python eval_pixellink_fast.py --synthetic 2 --gt_path ./gt         (random images named synthetic_<i>)
    python eval_pixellink_fast.py ... --map_scales 0.5,1,2 --flip      (multi-scale and flip testing: the passes' score maps
                                                                        are fused on the device and decoded once; build-defined,
                                                                        its effect on the F-measure is unmeasured)
    python eval_pixellink_fast.py ... --eval_grid_pixel 0.5:0.9:5 --eval_grid_link 0.5:0.9:5
                                                                       (search the two decode thresholds: every pair is decoded
                                                                        and matched behind the one forward, one line per pair)

Flag names and defaults are test_pixellink_fast.py's where the two scripts share them; that script itself is unchanged and
writes the same `res_<name>.txt` files as before.  Unlike it, images of any size are taken: each is resized on the device
and the boxes are matched in original-image pixels.  --min_side / --min_area drop small boxes (0: nothing, as the
reference)."""
import argparse
import os
import tempfile

import numpy as np

from tensorflow_ocr_amd import cli

MAP_SCALES_HELP = ("multi-scale testing by score-map fusion: the network runs at each of these scales of the eval size (sides "
                   "rounded to multiples of 32), the pixel and link probabilities of all passes are resampled onto the 1/4 "
                   "eval-size grid and averaged on the device, and the link decode runs once (1 to 8 numbers, e.g. 0.5,1,2; "
                   "1 need not be among them).  Build-defined; whether it raises the F-measure is unmeasured.  Activation "
                   "memory grows with the square of the largest scale")
FLIP_HELP = ("also run every scale on the images mirrored left to right and fuse those maps too (alone: scale 1 plus its "
             "mirror)")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--checkpoint_path', type=str, default=None)
    ap.add_argument('--test_data_path', type=str, default='/tmp/images/')
    ap.add_argument('--gt_path', type=str, default=None, metavar='DIR', help="a directory of gt_<name>.txt files (ICDAR "
                    "layout, ### = ignored); default: beside the images")
    ap.add_argument('--pixel_conf_threshold', type=float, default=0.8)
    ap.add_argument('--link_conf_threshold', type=float, default=0.9)
    ap.add_argument('--eval_image_width', type=int, default=1280)
    ap.add_argument('--eval_image_height', type=int, default=768)
    ap.add_argument('--min_side', type=float, default=0.0, help="drop boxes whose shorter side is below this (image pixels).  "
                    "Default 0: nothing is dropped, as in the reference")
    ap.add_argument('--min_area', type=float, default=0.0, help="drop boxes whose area is below this")
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--synthetic', type=int, default=0, help='evaluate N synthetic images instead of files')
    ap.add_argument('--precision', choices=['f16', 'f32'], default='f16', help="as test_pixellink_fast.py's flag")
    ap.add_argument('--eval_protocol', choices=['raster', 'icdar15'], default='raster', help="raster = the reference's "
                    "matching rule; icdar15 = the official ICDAR-2015 protocol (polygon IoU, ### as don't-care regions), the "
                    "line then ends in [icdar15]")
    ap.add_argument('--eval_sweep', type=cli.sweep_arg, default=None, metavar='LO:HI:N',
                    help=cli.sweep_help("the component's mean pixel score, in [0, 1]"))
    ap.add_argument('--map_scales', type=cli.map_scales_arg, default=None, metavar='S1,S2,...', help=MAP_SCALES_HELP)
    ap.add_argument('--flip', action='store_true', help=FLIP_HELP)
    cli.add_grid_flags(ap)
    FLAGS = ap.parse_args(argv)
    cli.check_grid_flags(ap, FLAGS)
    if FLAGS.min_side < 0 or FLAGS.min_area < 0:
        ap.error('--min_side and --min_area must not be negative')
    if FLAGS.batch_size < 1:
        ap.error('--batch_size must be positive')
    if FLAGS.synthetic and FLAGS.gt_path is None:
        ap.error('--synthetic needs --gt_path (there is no image directory to look beside)')
    return FLAGS


def main(argv=None):
    FLAGS = parse(argv)
    import torch
    from tensorflow_ocr_amd import checkpoint, evaluate
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import pixellink
    g = Graph('cuda:0', precision=FLAGS.precision)
    H, W = FLAGS.eval_image_height, FLAGS.eval_image_width

    def logits(gr, im):       # test_pixellink_fast.py's normalisation, (im - 120) / 60 in f32 ahead of the net, on the device
        net = pixellink.PixelLinkNet((im - 120.0) / 60.0, graph=gr)
        return net.pixel_cls, net.link_cls
    tmp = None
    if FLAGS.synthetic:       # random images, written where the evaluator reads images from
        tmp = tempfile.TemporaryDirectory()
        rng = np.random.default_rng(0)
        for i in range(FLAGS.synthetic):
            np.save(os.path.join(tmp.name, 'synthetic_%d.npy' % i), rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        data = tmp.name
    else:
        data = FLAGS.test_data_path
    forward = GraphedForward(g, logits)
    if FLAGS.checkpoint_path:
        forward(torch.zeros((1, H, W, 3), dtype=torch.float32, device=g.device))       # the variables exist after one forward
        if FLAGS.checkpoint_path.endswith('.npz'):
            sd = dict(np.load(FLAGS.checkpoint_path))
        else:       # a TF checkpoint directory / prefix; EMA shadows restored like test.py:149-150
            sd, _ = checkpoint.load_tf_checkpoint(FLAGS.checkpoint_path, use_moving_averages=True)
        g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, sd), strict=False)
    ev = evaluate.LinkEvaluator(g, forward, data, batch_size=FLAGS.batch_size, gt_path=FLAGS.gt_path,
                                pixel_conf_threshold=FLAGS.pixel_conf_threshold,
                                link_conf_threshold=FLAGS.link_conf_threshold, min_side=FLAGS.min_side,
                                min_area=FLAGS.min_area, eval_image_height=H, eval_image_width=W,
                                protocol=FLAGS.eval_protocol, sweep=FLAGS.eval_sweep, map_scales=FLAGS.map_scales,
                                flip=FLAGS.flip, grid=cli.grid_option(FLAGS))
    try:
        res = ev.run()
        print(evaluate.format_line(res), flush=True)
        if FLAGS.eval_sweep is not None:
            print(evaluate.format_sweep(res), flush=True)
        if 'grid' in res:
            print(evaluate.format_grid(res), flush=True)
    finally:
        if tmp is not None:
            tmp.cleanup()


if __name__ == '__main__':
    main()
