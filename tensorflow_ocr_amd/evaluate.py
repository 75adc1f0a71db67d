"""Held-out evaluation on the device: precision / recall / F-measure of a detector over a directory of images and
`gt_*.txt` files (the ICDAR layout datasets/icdar.py reads).  One pass driver, `Evaluator`, runs per batch

    upload -> detector.detect (resize, forward, decode) -> ocr_eval_collect -> matcher (-> curve)

with the counters of tool/metrics.py on the device, and reads the device once at its end.  What lies between the upload
and the collect step is one of four detectors: `RboxSingleScale` / `RboxMultiScale` (`Evaluator`, the EAST RBOX
geometry) and `LinkSingleScale` / `LinkFused` (`LinkEvaluator`, the PixelLink geometry of test_pixellink_fast.py; test.py's
own link path, the contour decode, still ends on the host and is not evaluated here).  Ground truths are matched in
ORIGINAL image coordinates; `###` (or `*`) marks an ignored (don't-care) ground truth (icdar.load_annoataion)."""
import os

import numpy as np
import torch

from . import ops
from .graph import get_default_graph

IMAGE_EXTS = ('jpg', 'png', 'jpeg', 'JPG', 'npy')


def resize_rule(h, w, max_side_len=3000):
    """test.py:92-121: the size an h x w image is resized to — the longer side limited to max_side_len, both sides
    multiples of 32 (already-multiples stay, others become (x // 32 - 1) * 32).  Returns (resize_h, resize_w)."""
    resize_w, resize_h = w, h
    if max(resize_h, resize_w) > max_side_len:
        ratio = float(max_side_len) / resize_h if resize_h > resize_w else float(max_side_len) / resize_w
    else:
        ratio = 1.
    resize_h = int(resize_h * ratio)
    resize_w = int(resize_w * ratio)
    resize_h = resize_h if resize_h % 32 == 0 else (resize_h // 32 - 1) * 32
    resize_w = resize_w if resize_w % 32 == 0 else (resize_w // 32 - 1) * 32
    if resize_h <= 0 or resize_w <= 0:
        raise ValueError('image too small for the reference sizing rule: %dx%d' % (h, w))
    return int(resize_h), int(resize_w)


def list_images(data):
    """The images under `data` (test.py:76-90 plus .npy arrays), in name order."""
    files = []
    for parent, _, filenames in os.walk(data):
        for filename in sorted(filenames):
            if filename.endswith(IMAGE_EXTS):
                files.append(os.path.join(parent, filename))
    return sorted(files)


def load_ground_truth(im_fn, gt_path=None):
    """(polys int32 [k,4,2], ignored bool [k]) of gt_<stem>.txt — beside the image, or under `gt_path` — in original image
    pixels (coordinates truncated as the reference's matcher casts them), or None when the file does not exist."""
    from .datasets import icdar
    p = icdar.txt_name(im_fn)
    if gt_path is not None:
        p = os.path.join(gt_path, os.path.basename(p))
    if not os.path.exists(p):
        return None
    polys, tags = icdar.load_annoataion(p)
    polys = np.asarray(polys, np.float32).reshape(-1, 4, 2)
    return polys.astype(np.int32), np.asarray(tags, bool).reshape(-1)


PROTOCOLS = ('raster', 'icdar15')


def _check_protocol(protocol):
    if protocol not in PROTOCOLS:
        raise ValueError("protocol must be 'raster' or 'icdar15', got %r" % (protocol,))


def quad_is_bow_tie(poly):
    """ocr_eval_ic15_match_batch's classification of one int quad [4,2]: counter-clockwise by the sign of the integer
    shoelace sum, then two or more negative turns = self-intersecting."""
    p = [(int(x), int(y)) for x, y in np.asarray(poly).reshape(4, 2)]
    if sum(p[i][0] * p[(i + 1) % 4][1] - p[(i + 1) % 4][0] * p[i][1] for i in range(4)) < 0:
        p[1], p[3] = p[3], p[1]
    turns = [(p[i][0] - p[i - 1][0]) * (p[(i + 1) % 4][1] - p[i][1]) - (p[i][1] - p[i - 1][1]) * (p[(i + 1) % 4][0] - p[i][0])
             for i in range(4)]
    return sum(t < 0 for t in turns) >= 2


def format_line(result):
    line = 'precision %.4f recall %.4f hmean %.4f (gt %d det %d)' % (
        result['precision'], result['recall'], result['hmean'], result['num_gt'], result['num_det'])
    return line + ' [icdar15]' if result.get('protocol') == 'icdar15' else line


def parse_sweep(text):
    """--eval_sweep: 'LO:HI:N' = N evenly spaced thresholds from LO to HI (both included), or a comma list of numbers ->
    a list of 1..64 floats; ValueError otherwise."""
    text = str(text).strip()
    if ':' in text:
        parts = text.split(':')
        if len(parts) != 3:
            raise ValueError('a sweep range is LO:HI:N, got %r' % (text,))
        lo, hi, n = float(parts[0]), float(parts[1]), int(parts[2])
        if n < 1 or (n == 1 and lo != hi):
            raise ValueError('a sweep range needs N >= 2 thresholds (or LO = HI), got %r' % (text,))
        values = [lo] if n == 1 else [lo + (hi - lo) * k / (n - 1) for k in range(n)]
    else:
        values = [float(v) for v in text.split(',') if v.strip()]
    return check_sweep(values)


SWEEP_HELP = ("also report precision / recall / hmean with only the detections of score >= each threshold kept, the best "
              "of them and AP, counted from the one matching pass: LO:HI:N = N evenly spaced thresholds, or a comma list "
              "(at most 64).  The threshold is on the matcher's order key: %s")


def sweep_arg(text):
    """`parse_sweep` as an argparse type"""
    import argparse
    try:
        return parse_sweep(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def check_sweep(sweep):
    values = [float(v) for v in sweep]
    if not 1 <= len(values) <= ops.EVAL_MAX_T:
        raise ValueError('a sweep takes 1 to %d thresholds, got %d' % (ops.EVAL_MAX_T, len(values)))
    return values


def sweep_rows(thresholds, rows):
    """curve rows [T][4] -> the 'sweep' list of a result, and its 'best' row (highest hmean, ties to the lowest index)"""
    from .tool import metrics
    out = []
    for thr, (num_gt, tp, fp, n_det) in zip(thresholds, rows):
        precision, recall = metrics.precision_recall(num_gt, tp, fp)
        hmean = metrics.fmean(precision, recall) if precision + recall > 0 else 0.0
        out.append({'threshold': thr, 'precision': precision, 'recall': recall, 'hmean': hmean, 'tp': tp, 'fp': fp,
                    'num_det': n_det})
    best = out[0]
    for row in out[1:]:
        if row['hmean'] > best['hmean']:
            best = row
    return out, best


def format_sweep(result):
    """the lines of a result's sweep: one per threshold, the best one marked, and AP"""
    lines = []
    for row in result['sweep']:
        lines.append('  score >= %-10.6g precision %.4f recall %.4f hmean %.4f (tp %d fp %d det %d)%s' % (
            row['threshold'], row['precision'], row['recall'], row['hmean'], row['tp'], row['fp'], row['num_det'],
            ' *' if row is result['best'] else ''))
    lines.append('  AP %.4f, best hmean %.4f at score >= %.6g' % (result['ap'], result['best']['hmean'],
                                                                result['best']['threshold']))
    return '\n'.join(lines)


# -- the decode-threshold grid of the link geometry ----------------------------------------
GRID_MAX_POINTS = 64                    # the most (pixel, link) pairs one grid takes; the evaluator's own pair is a 65th
GRID_MAX_SLICES = 512                   # default grid_chunk: the most points x images decoded in one launch sequence
GRID_HELP = ("search the decode thresholds in ONE pass: with the other --%sgrid_* flag, every (pixel, link) pair of the two "
             "lists (LO:HI:N = N evenly spaced values, or a comma list; at most 64 pairs) is decoded and matched on the device "
             "behind the same forward, and one line per pair is printed, the best hmean marked.  The line of the run itself "
             "stays that of --pixel_conf_threshold / --link_conf_threshold")


def check_grid(grid):
    """grid = (pixel_list, link_list), two non-empty sequences of finite numbers whose product has 1..64 points -> the
    points [(pixel, link)] in pixel-major order; ValueError otherwise."""
    import math
    try:
        pixel_list, link_list = grid
        pixel_list, link_list = [float(v) for v in pixel_list], [float(v) for v in link_list]
    except (TypeError, ValueError):
        raise ValueError('grid is (pixel thresholds, link thresholds), two sequences of numbers, got %r' % (grid,))
    if not pixel_list or not link_list:
        raise ValueError('a grid needs at least one pixel threshold and one link threshold')
    for v in pixel_list + link_list:
        if not math.isfinite(v):
            raise ValueError('a grid threshold must be finite, got %r' % (v,))
    if len(pixel_list) * len(link_list) > GRID_MAX_POINTS:
        raise ValueError('a grid takes at most %d points, got %d x %d' % (GRID_MAX_POINTS, len(pixel_list), len(link_list)))
    return [(p, l) for p in pixel_list for l in link_list]


def check_grid_flags(ap, pixel_list, link_list, sweep, prefix=''):
    """the cross-checks of --<prefix>grid_pixel / --<prefix>grid_link as argparse errors -> the `grid=` option or None"""
    names = ('--%sgrid_pixel' % prefix, '--%sgrid_link' % prefix)
    if (pixel_list is None) != (link_list is None):
        ap.error('%s and %s come together' % names)
    if pixel_list is None:
        return None
    if sweep is not None:
        ap.error('%s / %s and the score sweep are separate passes: give one of them' % names)
    try:
        check_grid((pixel_list, link_list))
    except ValueError as e:
        ap.error(str(e))
    return (pixel_list, link_list)


def grid_rows(points, records, overflow):
    """records [G] of (num_gt, tp, fp, n_det) and overflow [G] (> 0: that point lost candidates) -> the rows of a result,
    one per point in the order given.  A point that overflowed reports 'overflow' and None for its metrics."""
    from .tool import metrics
    out = []
    for (pixel, link), (num_gt, tp, fp, n_det), over in zip(points, records, overflow):
        row = {'pixel_conf_threshold': pixel, 'link_conf_threshold': link}
        if over > 0:
            row.update(dict.fromkeys(('precision', 'recall', 'hmean', 'tp', 'fp', 'num_det', 'num_gt')), overflow=int(over))
        else:
            precision, recall = metrics.precision_recall(num_gt, tp, fp)
            hmean = metrics.fmean(precision, recall) if precision + recall > 0 else 0.0
            row.update(precision=precision, recall=recall, hmean=hmean, tp=tp, fp=fp, num_det=n_det, num_gt=num_gt)
        out.append(row)
    return out


def grid_best(rows):
    """the row of highest hmean, ties to the lowest index; a row that overflowed cannot be it (None if all did)"""
    best = None
    for row in rows:
        if 'overflow' not in row and (best is None or row['hmean'] > best['hmean']):
            best = row
    return best


def format_grid(result):
    """the lines of a result's grid: one per point (row 0 is the run's own pair), the best one marked"""
    lines = []
    for row in result['grid']:
        head = '  pixel > %-8.6g link > %-8.6g ' % (row['pixel_conf_threshold'], row['link_conf_threshold'])
        if 'overflow' in row:
            lines.append(head + 'overflow: %d candidates more than the limits hold' % row['overflow'])
        else:
            lines.append(head + 'precision %.4f recall %.4f hmean %.4f (tp %d fp %d det %d)%s' % (
                row['precision'], row['recall'], row['hmean'], row['tp'], row['fp'], row['num_det'],
                ' *' if row is result['grid_best'] else ''))
    best = result['grid_best']
    lines.append('  best hmean %.4f at pixel > %.6g, link > %.6g' % (
        best['hmean'], best['pixel_conf_threshold'], best['link_conf_threshold']))
    return '\n'.join(lines)


# -- resizing on the device: the evaluator's detectors and test.py ---------------------------------------------
def to_device(im, device):
    """an image uint8 [h,w,3] on the device"""
    return torch.from_numpy(np.ascontiguousarray(im, dtype=np.uint8)).to(device)


def resize_batch(srcs, rh, rw):
    """device originals (uint8 [h,w,3] each) -> x f32 [n,rh,rw,3], every one resized to rh x rw on the device"""
    x = torch.empty((len(srcs), rh, rw, 3), dtype=torch.float32, device=srcs[0].device)
    for i, src in enumerate(srcs):
        ops.resize_linear_u8(src, x[i])
    return x


def ratio_rows(n, ratio_w=1.0, ratio_h=1.0, device=None):
    """f32 [n,2] rows (ratio_w, ratio_h): what ocr_eval_collect divides the detections by (test.py:127).  The default,
    (1, 1), is for detections that are in original-image pixels already."""
    return torch.from_numpy(np.tile(np.array([ratio_w, ratio_h], np.float32), (n, 1))).to(device)


def multiscale_inputs(srcs, scales, max_side_len=3000):
    """device originals of ONE shape -> (xs, ratios): per scale one f32 [n,H_s,W_s,3] batch, every image resized from the
    ORIGINAL to rbox.scale_sizes' size, and one f32 [n,2] (ratio_w, ratio_h) tensor"""
    from .tool import rbox
    h, w = srcs[0].shape[:2]
    xs, ratios = [], []
    for rh, rw in rbox.scale_sizes(h, w, scales, max_side_len):
        xs.append(resize_batch(srcs, rh, rw))
        ratios.append(ratio_rows(len(srcs), rw / float(w), rh / float(h), srcs[0].device))
    return xs, ratios


# -- the detectors ---------------------------------------------------------------------------------------------
# detect(batch, srcs): batch = [(image uint8 [h,w,3], polys, ignored)] of one ORIGINAL shape, srcs = its images on the
# device -> the rows ops.eval_collect reads (merged, keep, n_keep, passed or None, inv_ratio f32 [n,2]) and `overflow`
# int32 [n,m], one column per limit the detector can exceed (> 0: candidates were lost).  A pure launch sequence.
# `overflow_messages`: m formatters, one per column, in the order the columns are reported.
class RboxSingleScale:
    """EAST RBOX at one scale: `forward(x)` takes a device f32 [n,H,W,3] batch (0..255, RGB) and returns the (score
    [n,H/4,W/4,1], geometry [n,H/4,W/4,5]) maps of model_rbox (tensors or head handles) as a pure launch sequence.  Images
    are resized by test.py's rule, then forward -> rbox.detect_device (decode, LANMS, the mean-score mask of box_thresh);
    the quads are in resized pixels, which the collect step divides by the resize ratios as test.py divides them.  A
    detection's score, the matcher's order key, is LANMS's merged score: a SUM of the merged pixels' scores."""

    def __init__(self, graph, forward, score_map_thresh, nms_thres, box_thresh, max_k, max_side_len):
        self.g, self.forward = graph, forward
        self.score_map_thresh, self.nms_thres, self.box_thresh = float(score_map_thresh), float(nms_thres), box_thresh
        self.max_k, self.max_side_len = max_k, max_side_len
        self.overflow_messages = (
            lambda worst: 'an image selected %d pixels more than max_k: raise max_k or the score threshold' % worst,)

    def resized(self, h, w):
        """the size an h x w image enters the network at"""
        return resize_rule(h, w, self.max_side_len)

    def ratio(self, h, w, rh, rw):
        """(ratio_w, ratio_h) of test.py:127"""
        return rw / float(w), rh / float(h)

    def detect(self, batch, srcs):
        from .tool import rbox
        h, w = batch[0][0].shape[:2]
        rh, rw = self.resized(h, w)
        x = resize_batch(srcs, rh, rw)
        inv_ratio = ratio_rows(len(srcs), *self.ratio(h, w, rh, rw), self.g.device)
        f_score, f_geometry = self.forward(x)
        merged, keep, n_keep, passed, total = rbox.detect_device(f_score, f_geometry, self.score_map_thresh, self.nms_thres,
                                                                 self.max_k, graph=self.g, box_thresh=self.box_thresh)
        return merged, keep, n_keep, passed, inv_ratio, (total - merged.shape[1])[:, None]


class RboxMultiScale(RboxSingleScale):
    """EAST RBOX, multi-scale testing: every image is resized from the ORIGINAL to rbox.scale_sizes' size
    at each of 1..8 scales, `forward` runs once per scale, and rbox.detect_multiscale_device pools the per-scale LANMS results
    in original-image pixels and fuses them (fuse = 'nms' or 'vote', at most max_pool <= 4096 pooled quads per image:
    include/ocr_multiscale.h).  The fused quads are in original pixels already, so the collect step divides by 1; their
    score, the matcher's order key, is the MEAN pixel score, in [0, 1].  Overflow columns: the worst total - max_k over
    the scales, pool_total - max_pool, the non-finite pooled rows."""

    def __init__(self, *single_scale, scales, fuse, max_pool):
        from .tool import rbox
        super().__init__(*single_scale)
        self.scales, self.fuse, self.max_pool = scales, fuse, int(max_pool)
        # rbox.overflow_error's three messages, each for its own column
        self.overflow_messages = tuple(
            (lambda worst, c=c: rbox.overflow_error(*[worst if k == c else 0 for k in range(3)], max_pool=self.max_pool))
            for c in range(3))

    @staticmethod
    def check(scales, fuse, max_pool):
        """the options as the constructor is given them -> the scale list, or None for one scale"""
        from .tool import rbox
        if fuse not in rbox.FUSE_MODES:
            raise ValueError("fuse must be 'nms' or 'vote', got %r" % (fuse,))
        if not 1 <= int(max_pool) <= ops.FUSE_MAX_POOL:
            raise ValueError('max_pool must be in [1, %d]' % ops.FUSE_MAX_POOL)
        if scales is None:
            return None
        return rbox.check_scales(scales)              # count, sign and finiteness; the sizes are checked per image shape

    def detect(self, batch, srcs):
        from .tool import rbox
        xs, ratios = multiscale_inputs(srcs, self.scales, self.max_side_len)
        maps = (self.forward(x) for x in xs)          # a scale's forward runs when detect_multiscale_device asks for it
        fused, keep, n_keep, overflow = rbox.detect_multiscale_device(
            maps, ratios, self.score_map_thresh, self.nms_thres, self.box_thresh, fuse=self.fuse, max_pool=self.max_pool,
            max_k=self.max_k, graph=self.g)
        return fused, keep, n_keep, None, ratio_rows(len(srcs), device=self.g.device), overflow


class LinkSingleScale:
    """The link geometry at one scale: `forward(x)` returns the (pixel_cls [n,H/4,W/4,2], link_cls [n,H/4,W/4,16]) LOGITS of
    `PixelLinkNet` (tensors or head handles) as a pure launch sequence.  Every image is resized on the device to the fixed
    eval_image_height x eval_image_width (test_pixellink_fast.py's flags), then forward -> softmaxes ->
    pixellink_fn.detect_device (link_cc, min-area rectangles, component scores, boxes).  ocr_min_area_rects takes one scale
    per call (hence the batches of one ORIGINAL shape): a component pixel (x, y) of the 1/4-resolution maps becomes the point
    (int(x * scale_x), int(y * scale_y)), so the boxes land in original-image pixels and the collect step divides by 1.
    A detection's score is its component's mean pixel score, in [0, 1] (ocr_component_scores; build-defined).  min_side /
    min_area filter the boxes (0: nothing, as the reference scripts).  Overflow column: ncomp - max_comps."""
    map_scales = scale_weights = None                 # (what `LinkFused` holds: one pass at the eval size, not mirrored)
    flip = False

    def __init__(self, graph, forward, eval_hw, pixel_conf_threshold, link_conf_threshold, min_size, max_comps, min_side,
                 min_area):
        self.g, self.forward = graph, forward
        self.eval_hw = (int(eval_hw[0]), int(eval_hw[1]))
        if min(self.eval_hw) < 4 or self.eval_hw[0] % 4 or self.eval_hw[1] % 4:
            raise ValueError('the eval size must be positive multiples of 4, got %dx%d' % self.eval_hw)
        if int(max_comps) < 1:
            raise ValueError('max_comps must be positive')
        self.pixel_conf_threshold, self.link_conf_threshold = float(pixel_conf_threshold), float(link_conf_threshold)
        self.min_size, self.max_comps = int(min_size), int(max_comps)
        self.min_side, self.min_area = float(min_side), float(min_area)
        self.overflow_messages = (
            lambda worst: 'an image holds %d components more than max_comps = %d' % (worst, self.max_comps),)

    def scales(self, h, w):
        """(scale_x, scale_y) of an h x w original: 1/4-resolution map cell -> original-image pixels.  An original side
        below a quarter of the eval side (a scale below 1) is refused."""
        sx, sy = w / float(self.eval_hw[1] // 4), h / float(self.eval_hw[0] // 4)
        if sx < 1.0 or sy < 1.0:
            raise ValueError('a %dx%d image is smaller than the %dx%d score maps: lower the eval size'
                             % (h, w, self.eval_hw[0] // 4, self.eval_hw[1] // 4))
        return sx, sy

    def _decode(self, decode, maps, box_scales):
        """`decode` = pixellink_fn.detect_device or detect_device_multiscale, on its leading arguments `maps`"""
        merged, keep, n_keep, passed, total = decode(
            *maps, self.pixel_conf_threshold, self.link_conf_threshold, self.min_size, *box_scales,
            max_comps=self.max_comps, min_side=self.min_side, min_area=self.min_area, graph=self.g)
        inv_ratio = ratio_rows(merged.shape[0], device=self.g.device)
        return merged, keep, n_keep, passed, inv_ratio, (total - merged.shape[1])[:, None]

    def maps(self, srcs):
        """(pixel_score [n,h,w], link_score) of a batch: what the decode reads, at any thresholds"""
        from .tool import pixellink_fn
        pixel_cls, link_cls = self.forward(resize_batch(srcs, *self.eval_hw))
        pixel_score = pixellink_fn.pixel_scores(pixel_cls, graph=self.g)[..., 1].contiguous()
        link_score = pixellink_fn.link_scores(link_cls, graph=self.g)
        return pixel_score, link_score

    def detect(self, batch, srcs):
        from .tool import pixellink_fn
        box_scales = self.scales(*batch[0][0].shape[:2])
        return self._decode(pixellink_fn.detect_device, self.maps(srcs), box_scales)

    def detect_grid(self, batch, srcs, points, chunk):
        """`detect` at every (pixel, link) pair of `points` behind ONE `maps`: yields per chunk of at most `chunk` points
        (merged, keep, n_keep, passed, inv_ratio, overflow) with leading dimension len(chunk) * n, point-major —
        pixellink_fn.detect_device_grid's slices.  A generator: a chunk's tensors can go before the next is decoded."""
        from .tool import pixellink_fn
        box_scales = self.scales(*batch[0][0].shape[:2])
        pixel_score, link_score = self.maps(srcs)
        for lo in range(0, len(points), chunk):
            part = points[lo:lo + chunk]
            merged, keep, n_keep, passed, total = pixellink_fn.detect_device_grid(
                pixel_score, link_score, [p for p, _ in part], [l for _, l in part], self.min_size, *box_scales,
                max_comps=self.max_comps, min_side=self.min_side, min_area=self.min_area, graph=self.g)
            inv_ratio = ratio_rows(merged.shape[0], device=self.g.device)
            yield merged, keep, n_keep, passed, inv_ratio, (total - merged.shape[1])[:, None]


class LinkFused(LinkSingleScale):
    """The link geometry, multi-scale and flip testing by SCORE-MAP fusion (include/ocr_map_fuse.h; the
    min-area-rectangle vertices of a component have no fixed correspondence across scales for a box-level vote).
    map_scales: 1 to 8 positive finite scales (1 need not be among them): every batch is resized from the ORIGINALS to each
    pixellink_fn.map_scale_sizes entry of the eval size and forwarded once, with flip=True a second time mirrored left to
    right; each pass's pixel and link probabilities are resampled onto the eval_hw / 4 grid and averaged with scale_weights
    (a scale's two passes share its weight), and the link decode runs once on the fused maps.  The fusion grid is the
    single-scale one, so the box scales and everything behind them are what they were.  Activation memory grows with the
    square of the largest scale.  Whether any of this raises the F-measure is unmeasured: no dataset or trained checkpoint
    is on any machine that built it."""

    def __init__(self, *single_scale, map_scales, scale_weights, flip):
        super().__init__(*single_scale)
        self.map_scales, self.scale_weights, self.flip = map_scales, scale_weights, flip

    def _passes(self, srcs):
        """the forward passes of a batch, one at a time.  A generator: fuse_score_maps uses a pass's logits up before it
        asks for the next forward, which may return the same buffers."""
        from .tool import pixellink_fn
        for rh, rw in pixellink_fn.map_scale_sizes(self.eval_hw[0], self.eval_hw[1], self.map_scales):
            x = resize_batch(srcs, rh, rw)
            pixel_cls, link_cls = self.forward(x)
            yield pixel_cls, link_cls, False
            if self.flip:
                pixel_cls, link_cls = self.forward(torch.flip(x, dims=[2]))
                yield pixel_cls, link_cls, True

    def _fusion(self, srcs):
        """fuse_score_maps' leading arguments: the passes, their weights, the fusion grid"""
        weights = np.repeat(np.asarray(self.scale_weights, np.float64), 2 if self.flip else 1)
        return self._passes(srcs), weights, (self.eval_hw[0] // 4, self.eval_hw[1] // 4)

    def maps(self, srcs):
        """the fused maps: views of fuse_score_maps' accumulator, which the decode reads as they are"""
        from .tool import pixellink_fn
        return pixellink_fn.fuse_score_maps(*self._fusion(srcs), graph=self.g)

    def detect(self, batch, srcs):
        from .tool import pixellink_fn
        return self._decode(pixellink_fn.detect_device_multiscale, self._fusion(srcs), self.scales(*batch[0][0].shape[:2]))


# -- the pass driver -------------------------------------------------------------------------------------------
class Evaluator:
    """Evaluator(graph, forward, data): the pass driver, and the EAST RBOX geometry's options.  `data` is a directory of
    images with gt_<stem>.txt beside them, or under `gt_path` (an image without one is skipped).  Images are batched by
    ORIGINAL shape, at most `batch_size` per chain; per chain `self.detector.detect` is all that knows the geometry
    (`RboxSingleScale`, or with scales=[...] `RboxMultiScale`; fuse / max_pool are the latter's).  `run()` makes one
    pass and returns {'precision', 'recall', 'hmean', 'num_gt', 'tp', 'fp', 'num_det', 'images'}; it reads the device once
    at its end: the record, and the column maxima of the chains' overflow counts — the detector's columns, then the
    detections over max_d — the first positive of which raises ValueError.

    protocol: 'raster' (the default) is the reference's matching rule (tool/bboxes.py:171-240, rasterised IoU).
    'icdar15' is the official ICDAR-2015 Task-1 localisation protocol (polygon IoU, `###` ground truths as don't-care
    regions, ground-truth-major greedy matching: bboxes.ic15_matching_batch), the figure that papers and the leaderboard
    report, up to the three build-defined points of DESIGN.md §3.3.17.  matching_threshold is its IoU threshold, the
    area-precision threshold is 0.5; self-intersecting ground truths are dropped when the files are read and counted in
    the result as 'invalid_gt', 'tp' / 'fp' / 'num_gt' / 'num_det' are matched / care detections - matched / care ground
    truths / detections before the don't-care filter, and the result names its 'protocol'.

    sweep: None, or a sequence of 1..64 score thresholds.  Then the pass also counts, from the SAME matching (no walk is
    repeated: include/ocr_eval_curve.h), what the matcher gives with only the detections of score >=
    threshold kept, and the result gains 'sweep' (a list of {'threshold', 'precision', 'recall', 'hmean', 'tp', 'fp',
    'num_det'}), 'best' (its row of highest hmean, ties to the lowest index) and 'ap' (average precision over the pooled
    detection scores of the pass); still one device read.  The threshold is on the MATCHER'S ORDER KEY, ocr_eval_collect's
    det_score, which each detector's docstring names.  Sweeping box_thresh, score_map_thresh or the link threshold would
    change the detection set or its order and is not what this does; for the link geometry's two decode thresholds that
    search is `LinkEvaluator(grid=...)`, which this geometry refuses.

    A detector's options read as attributes of the evaluator (`ev.max_k`, `ev.eval_hw`, `ev.scales(h, w)`)."""

    def __init__(self, graph, forward, data, batch_size=8, max_images=None, matching_threshold=0.5, score_map_thresh=0.8,
                 nms_thres=0.2, box_thresh=None, max_k=None, max_d=ops.EVAL_MAX_D, max_side_len=3000, gt_path=None,
                 protocol='raster', sweep=None, scales=None, fuse='nms', max_pool=1024, grid=None):
        _check_protocol(protocol)                     # (its error comes before the scale options', as it always did)
        if grid is not None:
            raise ValueError('the decode-threshold grid (grid=...) is built for the link geometry only: LinkEvaluator')
        scales = RboxMultiScale.check(scales, fuse, max_pool)
        self._init_pass(graph, data, batch_size, max_images, matching_threshold, max_d, gt_path, protocol, sweep)
        options = (self.g, forward, score_map_thresh, nms_thres, box_thresh, max_k, max_side_len)
        self.detector = RboxSingleScale(*options) if scales is None else \
            RboxMultiScale(*options, scales=scales, fuse=fuse, max_pool=max_pool)

    def _init_pass(self, graph, data, batch_size, max_images, matching_threshold, max_d, gt_path, protocol, sweep,
                   grid_points=None, grid_chunk=None):
        """the driver's own state: the samples, the matcher's options, the record and the curve — or, with grid_points
        (the base pair, then check_grid's points), one record per point"""
        from .tool import metrics
        _check_protocol(protocol)
        self.protocol, self.area_prec_thr, self.invalid_gt = protocol, 0.5, 0
        self.sweep = None if sweep is None else check_sweep(sweep)
        self.grid_points = grid_points
        if grid_chunk is not None and int(grid_chunk) < 1:
            raise ValueError('grid_chunk must be positive')
        self.grid_chunk = None if grid_chunk is None else int(grid_chunk)
        self.g = graph or get_default_graph()
        if not os.path.isdir(data):
            raise FileNotFoundError('no evaluation directory %r' % (data,))
        files = [(f, load_ground_truth(f, gt_path)) for f in list_images(data)]
        self.samples = [(f, gt) for f, gt in files if gt is not None]
        if max_images:
            self.samples = self.samples[:int(max_images)]
        if not self.samples:
            raise FileNotFoundError('no image with a gt_*.txt under %r' % (data,))
        if protocol == 'icdar15':
            kept = []
            for f, (polys, ignored) in self.samples:
                ok = np.array([not quad_is_bow_tie(q) for q in polys], bool).reshape(-1)
                self.invalid_gt += int((~ok).sum())
                kept.append((f, (polys[ok], ignored[ok])))
            self.samples = kept
        too_many = [f for f, (polys, _) in self.samples if len(polys) > ops.EVAL_MAX_G]
        if too_many:
            raise ValueError('more than %d ground truths in %s' % (ops.EVAL_MAX_G, too_many[0]))
        if not 1 <= int(max_d) <= ops.EVAL_MAX_D:
            raise ValueError('max_d must be in [1, %d]' % ops.EVAL_MAX_D)
        self.batch_size = max(1, int(batch_size))
        self.matching_threshold, self.max_d = float(matching_threshold), int(max_d)
        self.acc = metrics.DeviceTpFp(self.g) if grid_points is None else metrics.DeviceGrid(len(grid_points), self.g)
        self.curve = None if self.sweep is None else metrics.DeviceCurve(self.sweep, len(self.samples), self.max_d, self.g)
        self.last = None          # the device tensors of the last chain (tests and the cost script look at them)

    def __getattr__(self, name):
        if name == 'detector':    # (asked for before the constructor made it)
            raise AttributeError(name)
        return getattr(self.detector, name)

    # -- one chain -------------------------------------------------------------------------------
    def _sources(self, batch):
        """the original images of a batch on the device (uint8 [h,w,3] each)"""
        return [to_device(im, self.g.device) for im, _, _ in batch]

    def _ground_truths(self, batch):
        """-> gts int32 [n,max_g,4,2], ng int32 [n], gignored uint8 [n,max_g] on the device, and the matcher's mask size"""
        dev = self.g.device
        n = len(batch)
        max_g = max([len(p) for _, p, _ in batch] + [1])
        gts = np.zeros((n, max_g, 4, 2), np.int32)
        ng = np.zeros((n,), np.int32)
        gign = np.zeros((n, max_g), np.uint8)
        extent = 1
        for i, (im, polys, ignored) in enumerate(batch):
            h, w, _ = im.shape
            k = len(polys)
            gts[i, :k], ng[i], gign[i, :k] = polys, k, ignored
            extent = max(extent, h, w, int(polys.max()) + 1 if k else 1)
        # any mask that holds every vertex gives the reference's counts; twice the extent leaves room for detections that
        # overhang the image, and bounds what a wild quad can cost
        side = int(min(32768, 2 * extent + 10))
        up = lambda a: torch.from_numpy(a).to(dev)
        return up(gts), up(ng), up(gign), (side, side)

    def _chain(self, batch):
        """one batch -> its overflow counts int32 [n,m+1]: the detector's columns, then nd_total - max_d"""
        srcs = self._sources(batch)
        ground_truths = self._ground_truths(batch)
        if self.grid_points is not None:
            return self._grid_chain(batch, srcs, ground_truths)
        *rows, overflow = self.detector.detect(batch, srcs)
        return torch.cat([overflow, self._match(*rows, *ground_truths)[:, None]], dim=1)

    def _grid_chain(self, batch, srcs, ground_truths):
        """one batch at every grid point -> the points' overflow maxima over the batch, int32 [G,m+1] (columns as
        `_chain`'s).  Per chunk of points one decode and one collect on points x images slices; then the matcher runs
        once per point on that point's n contiguous slices, with the batch's own ground truths, into that point's record:
        every row is the plain pass's arithmetic."""
        n = len(batch)
        chunk = self.grid_chunk or max(1, GRID_MAX_SLICES // n)
        worst, lo = [], 0
        for *rows, overflow in self.detector.detect_grid(batch, srcs, self.grid_points, chunk):
            dets, det_score, nd, nd_total = self._collect(*rows)
            over = torch.cat([overflow, (nd_total - self.max_d)[:, None]], dim=1)
            points = over.shape[0] // n
            for k in range(points):
                s = slice(k * n, (k + 1) * n)
                self._count(dets[s], det_score[s], nd[s], nd_total[s], *ground_truths, self.acc.records[lo + k])
            worst.append(over.view(points, n, -1).max(dim=1).values)
            lo += points
        return torch.cat(worst)

    def _collect(self, merged, keep, n_keep, passed, inv_ratio):
        """detection rows -> the ordered detection lists (dets, det_score, nd, nd_total) of ocr_eval_collect"""
        g = self.g
        n = merged.shape[0]
        dets = torch.empty((n, self.max_d, 4, 2), dtype=torch.int32, device=g.device)
        det_score = torch.empty((n, self.max_d), dtype=torch.float32, device=g.device)
        nd = torch.empty((n,), dtype=torch.int32, device=g.device)
        nd_total = torch.empty_like(nd)
        ops.eval_collect(merged, keep, n_keep, None if passed is None else passed.to(torch.uint8), inv_ratio, dets,
                         det_score, nd, nd_total)
        return dets, det_score, nd, nd_total

    def _count(self, dets, det_score, nd, nd_total, gts, ng, gign, mask_hw, record):
        """ordered detection lists -> matching, the counters added to `record` (-> the curve)"""
        from .tool import bboxes
        g = self.g
        if self.protocol == 'icdar15':
            det_match, gt_match, _ = bboxes.ic15_matching_batch(dets, nd, gts, ng, gign, self.matching_threshold,
                                                                self.area_prec_thr, record=record, graph=g)
            self.last = dict(dets=dets, det_score=det_score, nd=nd, nd_total=nd_total, det_match=det_match,
                             gt_match=gt_match, gts=gts, ng=ng, gdontcare=gign)
            if self.curve is not None:
                self.curve.add_ic15(det_match, gt_match, det_score, nd, ng)
            return
        tp, fp, _ = bboxes.bboxes_matching_batch(dets, nd, gts, ng, gign, self.matching_threshold, record=record,
                                                 graph=g, mask_hw=mask_hw)
        self.last = dict(dets=dets, det_score=det_score, nd=nd, nd_total=nd_total, tp=tp, fp=fp, gts=gts, ng=ng)
        if self.curve is not None:
            self.last['gignored'] = gign
            self.curve.add_raster(tp, fp, det_score, nd, ng, gign if gign.dtype == torch.uint8 else gign.to(torch.uint8))

    def _match(self, merged, keep, n_keep, passed, inv_ratio, gts, ng, gign, mask_hw):
        """detection rows -> ordered detection list -> matching, the counters added to the record (-> the curve).  Returns
        nd_total - max_d (> 0: detections were lost), a device tensor like everything here."""
        dets, det_score, nd, nd_total = self._collect(merged, keep, n_keep, passed, inv_ratio)
        self._count(dets, det_score, nd, nd_total, gts, ng, gign, mask_hw, self.acc.record)
        return nd_total - self.max_d

    # -- one pass --------------------------------------------------------------------------------
    def run(self):
        from .datasets import icdar
        self.acc.reset()
        if self.curve is not None:
            self.curve.reset()
        overflow, buckets = [], {}
        for im_fn, (polys, ignored) in self.samples:
            im = icdar.read_image_rgb(im_fn)
            key = tuple(im.shape[:2])
            items = buckets.setdefault(key, [])
            items.append((im, polys, ignored))
            if len(items) == self.batch_size:
                overflow.append(self._chain(buckets.pop(key)))
        for key in sorted(buckets):
            overflow.append(self._chain(buckets[key]))
        messages = self.detector.overflow_messages + (
            lambda over: 'an image kept %d detections more than max_d = %d' % (over, self.max_d),)
        if self.grid_points is not None:
            return self._grid_result(torch.stack(overflow).max(dim=0).values, messages)
        # the single read of the pass: the record and the overflow columns' maxima in one device-to-host copy
        worst = torch.cat(overflow).max(dim=0).values
        if self.curve is None:
            (num_gt, tp, fp, n_det), worst = self.acc.value_with(worst)
        else:       # ... and the curve, the order flag and AP in the same copy
            self.curve.finish(self.acc.record)
            (num_gt, tp, fp, n_det), worst, rows, unsorted, ap = self.curve.value_with(self.acc, worst)
        for over, message in zip(worst, messages):
            if over > 0:
                raise ValueError(message(over))
        result = self._result(num_gt, tp, fp, n_det)
        if self.curve is not None:
            if unsorted:
                raise ValueError('the detection scores of an image are not in descending order (NaNs last): the sweep '
                                 'and AP count score prefixes of the matching order')
            sweep, best = sweep_rows(self.curve.thresholds_host, rows)
            result.update(sweep=sweep, best=best, ap=ap)
        return result

    def _result(self, num_gt, tp, fp, n_det):
        """a record -> the result's own fields"""
        from .tool import metrics
        precision, recall = metrics.precision_recall(num_gt, tp, fp)
        hmean = metrics.fmean(precision, recall) if precision + recall > 0 else 0.0
        result = {'precision': precision, 'recall': recall, 'hmean': hmean, 'num_gt': num_gt, 'tp': tp, 'fp': fp,
                  'num_det': n_det, 'images': len(self.samples)}
        if self.protocol == 'icdar15':
            result.update(invalid_gt=self.invalid_gt, protocol=self.protocol)
        return result

    def _grid_result(self, worst, messages):
        """the single read of a grid pass — every point's record and its overflow maxima (worst int32 [G,m+1]) in one
        device-to-host copy — and the result: row 0's fields, 'grid' and 'grid_best'.  An overflow at row 0 raises what a
        plain pass raises; at another row it is that row's 'overflow' (the first positive column, in the order the limits
        are reported), and the pass goes on."""
        m = worst.shape[1]
        records, flat = self.acc.value_with(worst)
        columns = [flat[k * m:(k + 1) * m] for k in range(len(records))]
        for over, message in zip(columns[0], messages):
            if over > 0:
                raise ValueError(message(over))
        result = self._result(*records[0])
        rows = grid_rows(self.grid_points, records, [next((v for v in c if v > 0), 0) for c in columns])
        result.update(grid=rows, grid_best=grid_best(rows))
        return result


class LinkEvaluator(Evaluator):
    """The pass driver with the link geometry's detectors: `LinkSingleScale`, or with map_scales / flip `LinkFused` (flip
    without map_scales is scale 1 plus its mirror; scale_weights default to equal).  The options are
    test_pixellink_fast.py's flags and the detectors' docstrings describe them; `scales=` (box-level fusion) is refused
    for this geometry.  `protocol`, `sweep`, max_d and the single device read per pass are `Evaluator`'s.

    grid=(pixel_list, link_list): the DECODE-THRESHOLD grid (include/ocr_decode_grid.h) — two sequences
    of finite numbers whose product has 1 to 64 points.  The pass then runs every forward once and decodes, collects and
    matches every (pixel, link) pair on the device behind the same score maps (fused ones with map_scales / flip), one record
    per point, still one device read.  Row 0 is always the constructor's own (pixel_conf_threshold, link_conf_threshold)
    pair: the result's own fields are row 0's, equal to a run without `grid`, and it gains 'grid' — a list of
    {'pixel_conf_threshold', 'link_conf_threshold', 'precision', 'recall', 'hmean', 'tp', 'fp', 'num_det', 'num_gt'}, row 0
    then the pairs in pixel-major order — and 'grid_best', the row of highest hmean (ties to the lowest index).  Overflow is
    per point: at row 0 it raises what it raises without a grid; at another row that row reports 'overflow': k and None for
    its metrics, cannot be the best, and the pass goes on.  grid_chunk: the most grid points decoded in one launch sequence
    (default: points x batch images <= 512; memory grows with it, the result does not depend on it).  `grid` with `sweep`
    is refused: the sweep thresholds the matcher's order key of ONE detection set, the grid changes the set."""

    def __init__(self, graph, forward, data, batch_size=8, max_images=None, matching_threshold=0.5, pixel_conf_threshold=0.8,
                 link_conf_threshold=0.9, min_size=10, max_comps=4096, min_side=0.0, min_area=0.0, max_d=ops.EVAL_MAX_D,
                 eval_image_height=768, eval_image_width=1280, gt_path=None, protocol='raster', sweep=None, scales=None,
                 map_scales=None, flip=False, scale_weights=None, grid=None, grid_chunk=None):
        if scales is not None:
            raise ValueError('multi-scale evaluation (scales=...) is built for the RBOX geometry only')
        grid_points = None
        if grid is not None:
            if sweep is not None:
                raise ValueError('grid and sweep are separate passes: the sweep thresholds the scores of one detection set, '
                                 'the grid changes the set')
            grid_points = [(float(pixel_conf_threshold), float(link_conf_threshold))] + check_grid(grid)
        elif grid_chunk is not None:
            raise ValueError('grid_chunk comes with grid')
        from .tool import pixellink_fn
        flip = bool(flip)
        if map_scales is None and scale_weights is not None:
            raise ValueError('scale_weights come with map_scales')
        if map_scales is None and flip:
            map_scales = [1.0]                       # flip alone: scale 1 and its mirror
        if map_scales is not None:
            map_scales, scale_weights = pixellink_fn.check_map_scales(map_scales, scale_weights)
        self._init_pass(graph, data, batch_size, max_images, matching_threshold, max_d, gt_path, protocol, sweep,
                        grid_points, grid_chunk)
        options = (self.g, forward, (eval_image_height, eval_image_width), pixel_conf_threshold, link_conf_threshold,
                   min_size, max_comps, min_side, min_area)
        self.detector = LinkSingleScale(*options) if map_scales is None else \
            LinkFused(*options, map_scales=map_scales, scale_weights=scale_weights, flip=flip)


class EmaWeights:
    """Context manager: the optimiser's EMA shadows stand in the variable store for the duration (the weights test.py
    restores), the raw weights come back bit for bit afterwards.  The store's version moves both times, so every pack
    follows (a recorded TrainStep re-packs before its next replay).  Nothing of this is part of the recorded step."""

    def __init__(self, graph, opt):
        self.st, self.ema = graph.store, getattr(opt, 'ema', None)
        if self.ema is None:
            raise ValueError('the optimiser keeps no moving averages (moving_average_decay): evaluate the raw weights')
        self.saved = None

    def __enter__(self):
        self.saved = self.st.flat.clone()
        self.st.flat.copy_(self.ema)
        self.st.version += 1
        return self

    def __exit__(self, *exc):
        self.st.flat.copy_(self.saved)
        self.saved = None
        self.st.version += 1
        return False


class TrainEval:
    """Evaluation inside a training run (multigpu_train.py --eval_data_path / --eval_steps): every `every` optimiser steps
    one `Evaluator` pass BETWEEN steps — nothing of it is part of the recorded step plan, whose call list is the same with
    and without it.  The network runs in inference mode on the training graph (batch norm on the moving statistics, eager
    launches) with the EMA shadows (`weights='ema'`, what test.py restores) or the raw weights; the raw weights are back
    bit for bit before the next step.  `network(graph, images)` -> (score, geometry), or with `evaluator=LinkEvaluator`
    (train_pixellink.py) -> (pixel_cls, link_cls); `opt` is read when a pass runs (the optimiser exists only after the
    step was built).  `last` holds the latest result.  sweep: None, or the score thresholds of the evaluator's `sweep`
    (the pass still reads the device once; `write` then adds eval/ap, eval/best_hmean, eval/best_threshold).
    scales / fuse / max_pool: the evaluator's multi-scale options (None = single scale; the RBOX `Evaluator` only).
    `LinkEvaluator`'s map_scales / flip / scale_weights and its grid / grid_chunk (the decode-threshold grid: `write` then
    adds eval/grid_best_hmean, eval/grid_best_pixel_threshold, eval/grid_best_link_threshold) travel in **evaluator_kw."""

    def __init__(self, graph, step, network, data, every, max_images=None, weights='ema', batch_size=8, evaluator=Evaluator,
                 sweep=None, scales=None, fuse='nms', max_pool=1024, **evaluator_kw):
        if weights not in ('ema', 'raw'):
            raise ValueError("weights must be 'ema' or 'raw'")
        if int(every) < 1:
            raise ValueError('every must be positive')
        self.g, self.step, self.network = graph, step, network
        self.every, self.weights = int(every), weights
        if sweep is not None:
            evaluator_kw['sweep'] = sweep
        if scales is not None:
            evaluator_kw.update(scales=scales, fuse=fuse, max_pool=max_pool)
        self.evaluator = evaluator(graph, self._forward, data, batch_size=batch_size, max_images=max_images, **evaluator_kw)
        self.last = None
        self.passes = 0

    def _forward(self, x):
        out = self.network(self.g, x)
        self.g.reset_tape()
        return out

    def due(self, optimiser_steps):
        return optimiser_steps > 0 and optimiser_steps % self.every == 0

    def run(self):
        from . import _lib
        if _lib.RECORDER is not None:
            raise RuntimeError('evaluation inside a recorded step')
        if self.weights == 'ema':
            with EmaWeights(self.g, self.step.opt):
                self.last = self.evaluator.run()
        else:
            self.last = self.evaluator.run()
            self.g.store.version += 1       # the inference forward refreshed lazy packs: none may count as current below
        # the packs are now where an optimiser step leaves them (TrainStep._eager): the batched ones re-packed from the
        # raw weights, the lazy ones out of date — so a step recorded next holds exactly the calls it holds without an
        # evaluation, and a replayed one finds nothing to re-pack
        self.step._repack()
        self.passes += 1
        return self.last

    def write(self, writer, global_step):
        """eval/precision, eval/recall, eval/hmean of the latest pass as one event of a summary.FileWriter; with a sweep
        also eval/ap, eval/best_hmean, eval/best_threshold; with a grid also eval/grid_best_hmean,
        eval/grid_best_pixel_threshold, eval/grid_best_link_threshold."""
        for k in ('precision', 'recall', 'hmean'):
            writer.add_scalar('eval/' + k, self.last[k])
        if 'sweep' in self.last:
            writer.add_scalar('eval/ap', self.last['ap'])
            writer.add_scalar('eval/best_hmean', self.last['best']['hmean'])
            writer.add_scalar('eval/best_threshold', self.last['best']['threshold'])
        if 'grid' in self.last:
            best = self.last['grid_best']
            writer.add_scalar('eval/grid_best_hmean', best['hmean'])
            writer.add_scalar('eval/grid_best_pixel_threshold', best['pixel_conf_threshold'])
            writer.add_scalar('eval/grid_best_link_threshold', best['link_conf_threshold'])
        writer.flush_step(global_step)
