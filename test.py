#!/usr/bin/env python3
"""Counterpart of the reference's test.py (flags :3-7, helpers :24-121, main :124-218) — BASELINE
config 0's script — on the MI355X path: `model.model(is_training=False)` (ResNet-v1-50 + PixelLink
heads), softmax scores, the script's own `pixel_detect`, one `cv2.minAreaRect` box per
`cv2.findContours` contour, `order_points`, `res_<name>.txt`.

`--geometry RBOX` runs the geometry the default checkpoint path is named for instead: `model_vgg_16.model_rbox`
(score, four distances x `--text_scale`, angle), per-pixel quads in raster order, locality-aware NMS, all on the device
(`main_rbox`); the default `--geometry link` is the path described above, unchanged.  With `--gt_path DIR` (RBOX only) the
detections are then matched against the `gt_<name>.txt` files there on the device (tensorflow_ocr_amd/evaluate.py) and one
line `precision .. recall .. hmean .. (gt .. det ..)` is printed.  `--scales 0.5,1,2 [--fuse nms|vote]` (RBOX only) is
multi-scale testing: one forward per scale, the per-scale detections pooled and fused on the device
(tool/rbox.detect_multiscale); without it the script is what it was.

    python test.py --test_data_path ./exhibition --checkpoint_path /tmp/east_icdar2015_resnet_v1_50_rbox/ --output_dir /tmp/res/

Same flag names / defaults.  Everything per-pixel runs on the GPU (network, cv2.resize, softmaxes,
mask, region labelling, convex hulls + rotating calipers); the per-box integer arithmetic of
:191-199 and `order_points` stay on the host as in the reference.  Forced differences: images are
decoded with PIL (or .npy) and no visualisation images are written (`cv2.imwrite` of score_map.jpg /
img.jpg / the annotated photo).  Boxes come out in the order of OpenCV's contour list."""
import argparse
import os
import time

import numpy as np
import torch

from tensorflow_ocr_amd import cli


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--input_size', type=int, default=512)
    ap.add_argument('--gpu_list', type=str, default='1')
    ap.add_argument('--test_data_path', type=str, default='./exhibition')
    ap.add_argument('--checkpoint_path', type=str, default='/tmp/east_icdar2015_resnet_v1_50_rbox/')
    ap.add_argument('--output_dir', type=str, default='/tmp/res/')
    ap.add_argument('--precision', choices=['f16', 'f32', 'f16x2'], default='f16', help="f32: the forward pass in the f32 inference "
                    "precision (f32 storage, matrix-core f32 convolutions): score maps within 1e-3 of the f32 reference, ~10x the time; "
                    "f16x2: the same f32 graph with split-f16 operands (hi + scaled residual) on the 16-bit matrix cores: "
                    "the accuracy of f32, faster")
    ap.add_argument('--fold-bn', dest='fold_bn', action=argparse.BooleanOptionalAction, default=None,
                    help="f32 / f16x2 only (ignored with f16): run each convolution, its frozen batch norm, the residual add and the "
                    "ReLU as one kernel (Graph(fold_bn=True)).  Default per precision: FOLD_BN_DEFAULT")
    ap.add_argument('--geometry', choices=['link', 'RBOX'], default='link', help="link: the PixelLink heads and the contour "
                    "decode of this script; RBOX: EAST's score + four distances + angle heads (model_vgg_16.model_rbox), decoded "
                    "per pixel into quads and merged by locality-aware NMS on the device (tool/rbox.detect)")
    ap.add_argument('--text_scale', type=int, default=512, help="RBOX only: the distance scale of the geometry head "
                    "(the reference's nets/model.py flag)")
    ap.add_argument('--box_thresh', type=float, default=None, help="RBOX only: after the NMS keep only the quads whose mean "
                    "score over their raster is above this (EAST's eval.py uses 0.1).  Default: no filter")
    ap.add_argument('--gt_path', type=str, default=None, metavar='DIR', help="RBOX only: a directory of gt_<name>.txt files "
                    "(ICDAR layout, ### = ignored).  After the run the detections are matched against them on the device "
                    "(tensorflow_ocr_amd.evaluate: the reference's raster-IoU rule, not the official ICDAR protocol) and one "
                    "line `precision .. recall .. hmean .. (gt .. det ..)` is printed")
    ap.add_argument('--eval_protocol', choices=['raster', 'icdar15'], default='raster', help="with --gt_path: raster = the "
                    "reference's rule above; icdar15 = the official ICDAR-2015 protocol (polygon IoU, ### as don't-care "
                    "regions), the line then ends in [icdar15]")
    ap.add_argument('--eval_sweep', type=cli.sweep_arg, default=None, metavar='LO:HI:N', help="with --gt_path: " + cli.sweep_help(
                    "LANMS's merged score, a sum of pixel scores (not a probability, not --box_thresh's mean)"))
    ap.add_argument('--scales', type=cli.scales_arg, default=None, metavar='S1,S2,..', help="RBOX only: multi-scale testing, e.g. "
                    "0.5,1,2 — the image is resized from the original to each scale (then by the sizing rule), one forward per "
                    "scale, the per-scale detections are pooled in original-image pixels and fused on the device "
                    "(tool/rbox.detect_multiscale).  The fused quads carry the mean pixel score, in [0, 1]; with --gt_path "
                    "the evaluator runs the same way.  Default: one scale, the script as it was")
    ap.add_argument('--fuse', choices=['nms', 'vote'], default='nms', help="with --scales: nms = score-ordered suppression "
                    "across the scales; vote = a kept quad's corners become the score-weighted mean of the quads it claimed")
    FLAGS = ap.parse_args(argv)
    if FLAGS.scales is not None and FLAGS.geometry != 'RBOX':
        ap.error('--scales needs --geometry RBOX (multi-scale fusion is built for the RBOX quads only)')
    if FLAGS.fuse != 'nms' and FLAGS.scales is None:
        ap.error('--fuse needs --scales')
    if FLAGS.eval_sweep is not None and FLAGS.gt_path is None:
        ap.error('--eval_sweep needs --gt_path')
    if FLAGS.gt_path is not None and FLAGS.geometry != 'RBOX':
        ap.error('--gt_path needs --geometry RBOX (the link geometry\'s contour decode ends on the host)')
    if FLAGS.eval_protocol != 'raster' and FLAGS.gt_path is None:
        ap.error('--eval_protocol needs --gt_path')
    return FLAGS


# --fold-bn when the flag is not given: on where the folded graph measured faster than the unfolded one at this script's
# case (512^2, batch 1) by more than the spread of the alternating repeats (profiles/fold_bn_forward.json)
FOLD_BN_DEFAULT = {'f32': True, 'f16x2': True}


def graph_kwargs(precision, fold_bn):
    """Graph(...) keywords of this script: no fold_bn at all with f16."""
    kw = {'precision': precision}
    if precision != 'f16':
        kw['fold_bn'] = FOLD_BN_DEFAULT[precision] if fold_bn is None else bool(fold_bn)
    return kw


def order_points(pts):
    """test.py:24-35: top-left, top-right, bottom-right, bottom-left."""
    from scipy.spatial import distance as dist
    x_sorted = pts[np.argsort(pts[:, 0]), :]
    left_most = x_sorted[:2, :]
    right_most = x_sorted[2:, :]
    left_most = left_most[np.argsort(left_most[:, 1]), :]
    (tl, bl) = left_most
    D = dist.cdist(tl[np.newaxis], right_most, 'euclidean')[0]
    (br, tr) = right_most[np.argsort(D)[::-1], :]
    return np.array([tl, tr, br, bl], dtype='int32')


def sort_poly(p):
    """test.py:37-43 (unused by main, kept for parity)."""
    min_axis = np.argmin(np.sum(p, axis=1))
    p = p[[min_axis, (min_axis + 1) % 4, (min_axis + 2) % 4, (min_axis + 3) % 4]]
    if abs(p[0, 0] - p[1, 0]) > abs(p[0, 1] - p[1, 1]):
        return p
    return p[[0, 3, 2, 1]]


def pixel_detect(score_map, geo_map, score_map_thresh=0.8, link_thresh=0.8, graph=None):
    """test.py:45-74 (see tool/pixellink_fn.east_pixel_detect)."""
    from tensorflow_ocr_amd.tool import pixellink_fn
    return pixellink_fn.east_pixel_detect(score_map, geo_map, score_map_thresh, link_thresh, graph=graph)


def get_images(test_data_path):
    """test.py:76-90 (+ .npy arrays)."""
    files = []
    exts = ['jpg', 'png', 'jpeg', 'JPG', 'npy']
    for parent, dirnames, filenames in os.walk(test_data_path):
        for filename in sorted(filenames):
            for ext in exts:
                if filename.endswith(ext):
                    files.append(os.path.join(parent, filename))
                    break
    print('Find {} images'.format(len(files)))
    return files


def resize_image(im, max_side_len=3000, graph=None):
    """test.py:92-121: limit the longer side, round both sides to multiples of 32 (the reference's
    rule: already-multiples stay, others become (x // 32 - 1) * 32), cv2.resize.  Returns the resized
    image as a DEVICE float32 [H,W,3] tensor and (ratio_h, ratio_w)."""
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.graph import get_default_graph
    g = graph or get_default_graph()
    h, w, _ = im.shape
    resize_h, resize_w = evaluate.resize_rule(h, w, max_side_len)          # the sizing rule and the resize are the evaluator's
    out = evaluate.resize_batch([evaluate.to_device(im, g.device)], resize_h, resize_w)[0]
    return out, (resize_h / float(h), resize_w / float(w))


def boxes_from_mask(score_map_res, ratio_h, ratio_w, graph=None):
    """test.py:182-199: contours -> minAreaRect -> boxPoints -> np.int0 -> x4 -> / ratio (integer
    array: the division result is truncated on assignment)."""
    from tensorflow_ocr_amd.tool import pixellink_fn
    _, boxes = pixellink_fn.find_contour_boxes(score_map_res, graph=graph)
    out = []
    for box in boxes:
        box = box.copy()
        box[:, 0] = box[:, 0] * 4
        box[:, 1] = box[:, 1] * 4
        box[:, 0] = box[:, 0] / ratio_w
        box[:, 1] = box[:, 1] / ratio_h
        out.append(box)
    return out


def _restore(FLAGS, g):
    """variable_averages.variables_to_restore(): the EMA shadows (test.py:149-158)."""
    from tensorflow_ocr_amd import checkpoint
    if not (os.path.exists(os.path.join(FLAGS.checkpoint_path, 'checkpoint')) or os.path.exists(FLAGS.checkpoint_path + '.index')):
        # the reference dies here too (`ckpt_state.model_checkpoint_path` on None, test.py:155-157):
        # never write boxes produced by randomly initialised weights
        raise FileNotFoundError('no checkpoint under --checkpoint_path %r' % FLAGS.checkpoint_path)
    sd, _ = checkpoint.load_tf_checkpoint(FLAGS.checkpoint_path, use_moving_averages=True)
    g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, sd), strict=False)
    print('Restore from {}'.format(FLAGS.checkpoint_path))


def main_rbox(FLAGS):
    """--geometry RBOX: model_rbox -> per-pixel quads -> locality-aware NMS, all on the device; the kept quads, divided
    by the resize ratios and truncated to integers, in the res_<name>.txt format of the link path.  --box_thresh adds the
    mean-score filter over each quad's raster that EAST's eval script applies after the NMS."""
    from tensorflow_ocr_amd import evaluate
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import model_vgg_16
    from tensorflow_ocr_amd.tool import rbox
    os.makedirs(FLAGS.output_dir, exist_ok=True)
    g = Graph('cuda:0', **graph_kwargs(FLAGS.precision, FLAGS.fold_bn))
    restored = False

    def network(gr, im):
        return model_vgg_16.model_rbox(im, is_training=False, text_scale=FLAGS.text_scale, graph=gr)
    forward = GraphedForward(g, network)
    for im_fn in get_images(FLAGS.test_data_path):
        im = icdar.read_image_rgb(im_fn)
        start_time = time.time()
        if FLAGS.scales is not None:
            # one resize (from the original) and one forward per scale, pooled and fused on the device: the quads come
            # back in original-image pixels, so nothing is divided below
            xs, ratios = evaluate.multiscale_inputs([evaluate.to_device(im, g.device)], FLAGS.scales)
            if not restored:
                forward(xs[0])
                _restore(FLAGS, g)
                restored = True
            quads = rbox.detect_multiscale((forward(x) for x in xs), ratios, box_thresh=FLAGS.box_thresh, fuse=FLAGS.fuse,
                                           graph=g)[0]
            print('net + fusion time:' + str((time.time() - start_time) * 1000) + 'ms')
            ratio_h = ratio_w = 1.0
        else:
            im_resized, (ratio_h, ratio_w) = resize_image(im, graph=g)
            x = im_resized[None]
            f_score, f_geometry = forward(x)
            if not restored:
                _restore(FLAGS, g)
                f_score, f_geometry = forward(x)
                restored = True
            torch.cuda.synchronize()
            print('net time:' + str((time.time() - start_time) * 1000) + 'ms')
            quads = rbox.detect(f_score, f_geometry, graph=g, box_thresh=FLAGS.box_thresh)[0]
        res_file = os.path.join(FLAGS.output_dir, 'res_{}.txt'.format(os.path.basename(im_fn).split('.')[0]))
        with open(res_file, 'w') as f:
            for q in quads:
                box = q[:8].reshape(4, 2).astype(np.float64)
                if FLAGS.scales is None:
                    box[:, 0] /= ratio_w
                    box[:, 1] /= ratio_h
                box = box.astype(np.int32)
                f.write('{},{},{},{},{},{},{},{}\r\n'.format(box[0, 0], box[0, 1], box[1, 0], box[1, 1],
                                                            box[2, 0], box[2, 1], box[3, 0], box[3, 1]))
    if FLAGS.gt_path is not None:
        # a second pass over the same images with the restored weights: forward -> decode -> LANMS -> filter -> match
        # per batch on the device, one read of the counters at its end
        ev = evaluate.Evaluator(g, forward, FLAGS.test_data_path, gt_path=FLAGS.gt_path, box_thresh=FLAGS.box_thresh,
                                protocol=FLAGS.eval_protocol, sweep=FLAGS.eval_sweep, scales=FLAGS.scales, fuse=FLAGS.fuse)
        res = ev.run()
        print(evaluate.format_line(res), flush=True)
        if FLAGS.eval_sweep is not None:
            print(evaluate.format_sweep(res), flush=True)


def main():
    FLAGS = parse()
    if FLAGS.geometry == 'RBOX':
        return main_rbox(FLAGS)
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import model
    from tensorflow_ocr_amd.tool import pixellink_fn
    os.makedirs(FLAGS.output_dir, exist_ok=True)
    g = Graph('cuda:0', **graph_kwargs(FLAGS.precision, FLAGS.fold_bn))
    restored = False

    def network(gr, im):      # sess.run([f_score, f_geometry]) + the two softmaxes: one HIP graph per image shape
        f_score, f_geometry = model.model(im, is_training=False, graph=gr)
        fg = f_geometry.data if hasattr(f_geometry, 'data') and not isinstance(f_geometry, torch.Tensor) else f_geometry
        return (pixellink_fn.pixel_scores(f_score, graph=gr),
                pixellink_fn.pixel_scores(fg.reshape(-1, 2), graph=gr).reshape(fg.shape))
    forward = GraphedForward(g, network)
    for im_fn in get_images(FLAGS.test_data_path):
        im = icdar.read_image_rgb(im_fn)                      # cv2.imread(im_fn)[:, :, ::-1]
        start_time = time.time()
        im_resized, (ratio_h, ratio_w) = resize_image(im, graph=g)
        x = im_resized[None]
        scores, pixel_score = forward(x)
        if not restored:
            _restore(FLAGS, g)
            scores, pixel_score = forward(x)
            restored = True
        cls_score = scores[:, :, :, 1:2].contiguous()           # softmax(f_score)[..., 1:2]; pixel_score: softmax over the pairs
        torch.cuda.synchronize()
        print('net time:' + str((time.time() - start_time) * 1000) + 'ms')
        score_map_res = pixel_detect(score_map=cls_score, geo_map=pixel_score, graph=g)
        boxes = boxes_from_mask(score_map_res, ratio_h, ratio_w, graph=g)
        res_file = os.path.join(FLAGS.output_dir, 'res_{}.txt'.format(os.path.basename(im_fn).split('.')[0]))
        with open(res_file, 'w') as f:
            for box in boxes:
                box = order_points(box)
                f.write('{},{},{},{},{},{},{},{}\r\n'.format(box[0, 0], box[0, 1], box[1, 0], box[1, 1],
                                                            box[2, 0], box[2, 1], box[3, 0], box[3, 1]))


if __name__ == '__main__':
    main()
