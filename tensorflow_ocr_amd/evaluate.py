"""Held-out evaluation on the device: precision / recall / F-measure of a detector over a directory of images and
`gt_*.txt` files (the ICDAR layout datasets/icdar.py reads), one chain per batch

    forward -> rbox.detect_device (decode, LANMS, mean-score mask) -> ocr_eval_collect -> bboxes.bboxes_matching_batch

with the counters of tool/metrics.py on the device (`metrics.DeviceTpFp`): the host reads them once per pass.  Two
matching rules: `protocol='raster'` (the default) is the reference's (tool/bboxes.py:171-240, rasterised IoU);
`protocol='icdar15'` is the official ICDAR-2015 Task-1 localisation protocol (polygon IoU, `###` ground truths as
don't-care regions, ground-truth-major greedy matching: bboxes.ic15_matching_batch), the figure
that papers and the leaderboard report — up to three build-defined points stated there (detection order, orientation,
self-intersecting quads), since no run of the official script pins it.  Ground truths are matched in ORIGINAL image
coordinates, detections are divided by the resize ratios as test.py divides them; `###` (or `*`) marks an ignored
(don't-care) ground truth (icdar.load_annoataion).

`Evaluator` is the EAST RBOX geometry.  `LinkEvaluator` is the PixelLink (link) geometry of test_pixellink_fast.py, the same
pass with another middle:

    forward -> softmaxes -> pixellink_fn.detect_device (link_cc, min-area rectangles, component scores, boxes) -> ...

(test.py's own link path, the contour decode of pixellink_fn.find_contour_boxes, still ends on the host and is not
evaluated here).

`sweep=[...]` (`--eval_sweep`) adds the precision / recall curve over detection scores, its best row and average
precision, counted on the device from the same matching pass (include/ocr_eval_curve.h).

`Evaluator(scales=[...])` (`--scales`, `--eval_scales`) is multi-scale testing: one forward per scale, the per-scale LANMS
results pooled in original-image pixels and fused on the device (rbox.detect_multiscale_device, include/ocr_multiscale.h,
DESIGN.md §3.3.19), then the same matcher.  `LinkEvaluator(map_scales=[...], flip=...)` (`--map_scales`, `--flip`,
`--eval_map_scales`, `--eval_flip`) is multi-scale and flip testing for the link geometry: the passes' score maps are
fused on the device (pixellink_fn.fuse_score_maps, include/ocr_map_fuse.h) and decoded once."""
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


class Evaluator:
    """Evaluator(graph, forward, data): `forward(x)` takes a device f32 [n,H,W,3] batch (0..255, RGB) and returns the
    (score [n,H/4,W/4,1], geometry [n,H/4,W/4,5]) maps of model_rbox (tensors or head handles) as a pure launch sequence;
    `data` is a directory of images with gt_<stem>.txt beside them, or under `gt_path` (an image without one is skipped).
    Images are resized by test.py's rule and batched by resized shape, at most `batch_size` per chain.  `run()` makes one pass and returns
    {'precision', 'recall', 'hmean', 'num_gt', 'tp', 'fp', 'num_det', 'images'}; it reads the device once at its end: the
    record, and the two overflow counts (pixels over max_k, detections over max_d), either of which raises ValueError.
    protocol='icdar15' swaps the matcher for the official ICDAR-2015 one (matching_threshold is its IoU threshold, the
    area-precision threshold is 0.5): self-intersecting ground truths are dropped when the files are read and counted in
    the result as 'invalid_gt', 'tp' / 'fp' / 'num_gt' / 'num_det' are matched / care detections - matched / care ground
    truths / detections before the don't-care filter, and the result names its 'protocol'.

    sweep: None, or a sequence of 1..64 score thresholds.  Then the pass also counts, from the SAME matching (no walk is
    repeated: DESIGN.md §3.3.18), what the matcher gives with only the detections of score >= threshold kept, and the
    result gains 'sweep' (a list of {'threshold', 'precision', 'recall', 'hmean', 'tp', 'fp', 'num_det'}), 'best' (its
    row of highest hmean, ties to the lowest index) and 'ap' (average precision over the pooled detection scores of the
    pass); still one device read.  The threshold is on the MATCHER'S ORDER KEY, ocr_eval_collect's det_score: for this
    geometry that is LANMS's merged score, a SUM of the merged pixels' scores — not a probability and not EAST's
    box_thresh mean; for `LinkEvaluator` it is the component's mean pixel score, in [0, 1].  Sweeping box_thresh,
    score_map_thresh or the link threshold would change the detection set or its order and is not what this does.
    With `scales` (below) the order key, and so the sweep's threshold, is instead the fused quad's MEAN pixel score, in
    [0, 1].

    scales: None = the single-scale pass above, bit for bit.  A sequence of 1..8 scales = multi-scale testing (DESIGN.md
    §3.3.19): every image is resized from the ORIGINAL to rbox.scale_sizes' size at each scale, `forward` runs once per
    scale, and rbox.detect_multiscale_device pools the per-scale LANMS results in original-image pixels and fuses them
    (fuse = 'nms' or 'vote', at most max_pool <= 4096 pooled quads per image); the fused list goes to the same matcher.
    The pass still reads the device once; a pool overflow or a non-finite pooled quad raises ValueError there too."""

    def __init__(self, graph, forward, data, batch_size=8, max_images=None, matching_threshold=0.5, score_map_thresh=0.8,
                 nms_thres=0.2, box_thresh=None, max_k=None, max_d=ops.EVAL_MAX_D, max_side_len=3000, gt_path=None,
                 protocol='raster', sweep=None, scales=None, fuse='nms', max_pool=1024):
        from .tool import metrics
        if protocol not in PROTOCOLS:
            raise ValueError("protocol must be 'raster' or 'icdar15', got %r" % (protocol,))
        self.ms_scales = self._check_scales(scales, fuse, max_pool)
        self.fuse, self.max_pool = fuse, int(max_pool)
        self.protocol, self.area_prec_thr, self.invalid_gt = protocol, 0.5, 0
        self.sweep = None if sweep is None else check_sweep(sweep)
        self.g = graph or get_default_graph()
        self.forward = forward
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
        self.matching_threshold = float(matching_threshold)
        self.score_map_thresh, self.nms_thres, self.box_thresh = float(score_map_thresh), float(nms_thres), box_thresh
        self.max_k, self.max_d, self.max_side_len = max_k, int(max_d), max_side_len
        self.acc = metrics.DeviceTpFp(self.g)
        self.curve = None if self.sweep is None else metrics.DeviceCurve(self.sweep, len(self.samples), self.max_d, self.g)
        self.last = None          # the device tensors of the last chain (tests and the cost script look at them)

    # -- one chain -------------------------------------------------------------------------------
    def _resized(self, h, w):
        """the size an h x w image enters the network at"""
        return resize_rule(h, w, self.max_side_len)

    def _ratio(self, h, w, rh, rw):
        """what ocr_eval_collect divides the detections by: (ratio_w, ratio_h) of test.py:127"""
        return rw / float(w), rh / float(h)

    def _upload(self, batch):
        """batch: [(image uint8 [h,w,3], polys, ignored)] of one resized shape -> x, inv_ratio, gts, ng, gignored, mask_hw"""
        rh, rw = self._resized(batch[0][0].shape[0], batch[0][0].shape[1])
        srcs = self._sources(batch)
        x, ratio = self._resize_batch(batch, srcs, rh, rw)
        return (x, ratio) + self._ground_truths(batch)

    def _sources(self, batch):
        """the original images of a batch on the device (uint8 [h,w,3] each)"""
        return [torch.from_numpy(np.ascontiguousarray(im, dtype=np.uint8)).to(self.g.device) for im, _, _ in batch]

    def _resize_batch(self, batch, srcs, rh, rw):
        """-> x f32 [n,rh,rw,3] (every original resized to rh x rw on the device), ratio f32 [n,2] = (ratio_w, ratio_h)"""
        dev = self.g.device
        n = len(batch)
        x = torch.empty((n, rh, rw, 3), dtype=torch.float32, device=dev)
        ratio = np.zeros((n, 2), np.float32)
        for i, (im, _, _) in enumerate(batch):
            h, w, _ = im.shape
            ops.resize_linear_u8(srcs[i], x[i])
            ratio[i] = self._ratio(h, w, rh, rw)
        return x, torch.from_numpy(ratio).to(dev)

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

    # -- the multi-scale chain (scales=...): beside the single-scale one, which it leaves as it is ----------------
    @staticmethod
    def _check_scales(scales, fuse, max_pool):
        from .tool import rbox
        if fuse not in rbox.FUSE_MODES:
            raise ValueError("fuse must be 'nms' or 'vote', got %r" % (fuse,))
        if not 1 <= int(max_pool) <= ops.FUSE_MAX_POOL:
            raise ValueError('max_pool must be in [1, %d]' % ops.FUSE_MAX_POOL)
        if scales is None:
            return None
        return rbox.check_scales(scales)              # count, sign and finiteness; the sizes are checked per image shape

    def _upload_multiscale(self, batch):
        """batch of one ORIGINAL shape -> xs (one resized batch per scale, each made from the original images), ratios (one f32
        [n,2] per scale), gts, ng, gignored, mask_hw"""
        from .tool import rbox
        h, w = batch[0][0].shape[:2]
        srcs = self._sources(batch)
        xs, ratios = [], []
        for rh, rw in rbox.scale_sizes(h, w, self.ms_scales, self.max_side_len):
            x, ratio = self._resize_batch(batch, srcs, rh, rw)
            xs.append(x)
            ratios.append(ratio)
        return (xs, ratios) + self._ground_truths(batch)

    def _chain_multiscale(self, batch):
        from .tool import rbox
        xs, ratios, gts, ng, gign, mask_hw = self._upload_multiscale(batch)
        maps = (self.forward(x) for x in xs)          # a scale's forward runs when detect_multiscale_device asks for it
        fused, keep, n_keep, overflow = rbox.detect_multiscale_device(
            maps, ratios, self.score_map_thresh, self.nms_thres, self.box_thresh, fuse=self.fuse, max_pool=self.max_pool,
            max_k=self.max_k, graph=self.g)
        self._over_pool.append(overflow[:, 1:])
        # the fused quads are in original-image pixels already: the collect pass divides by 1.  `total` is given so that
        # _match's `total - rows` is the worst per-scale overflow over max_k
        ones = torch.ones((len(batch), 2), dtype=torch.float32, device=self.g.device)
        return self._match(fused, keep, n_keep, None, overflow[:, 0] + fused.shape[1], ones, gts, ng, gign, mask_hw)

    def _chain(self, batch):
        from .tool import rbox
        x, inv_ratio, gts, ng, gign, mask_hw = self._upload(batch)
        f_score, f_geometry = self.forward(x)
        merged, keep, n_keep, passed, total = rbox.detect_device(f_score, f_geometry, self.score_map_thresh, self.nms_thres,
                                                                 self.max_k, graph=self.g, box_thresh=self.box_thresh)
        return self._match(merged, keep, n_keep, passed, total, inv_ratio, gts, ng, gign, mask_hw)

    def _match(self, merged, keep, n_keep, passed, total, inv_ratio, gts, ng, gign, mask_hw):
        """detection rows -> ordered detection list -> matching, the counters added to the record"""
        from .tool import bboxes
        g = self.g
        n, max_k = merged.shape[:2]
        dets = torch.empty((n, self.max_d, 4, 2), dtype=torch.int32, device=g.device)
        det_score = torch.empty((n, self.max_d), dtype=torch.float32, device=g.device)
        nd = torch.empty((n,), dtype=torch.int32, device=g.device)
        nd_total = torch.empty_like(nd)
        ops.eval_collect(merged, keep, n_keep, None if passed is None else passed.to(torch.uint8), inv_ratio, dets,
                         det_score, nd, nd_total)
        if self.protocol == 'icdar15':
            det_match, gt_match, _ = bboxes.ic15_matching_batch(dets, nd, gts, ng, gign, self.matching_threshold,
                                                                self.area_prec_thr, record=self.acc.record, graph=g)
            self.last = dict(dets=dets, det_score=det_score, nd=nd, nd_total=nd_total, det_match=det_match,
                             gt_match=gt_match, gts=gts, ng=ng, gdontcare=gign)
            if self.curve is not None:
                self.curve.add_ic15(det_match, gt_match, det_score, nd, ng)
            return total - max_k, nd_total - self.max_d
        tp, fp, _ = bboxes.bboxes_matching_batch(dets, nd, gts, ng, gign, self.matching_threshold, record=self.acc.record,
                                                 graph=g, mask_hw=mask_hw)
        self.last = dict(dets=dets, det_score=det_score, nd=nd, nd_total=nd_total, tp=tp, fp=fp, gts=gts, ng=ng)
        if self.curve is not None:
            self.last['gignored'] = gign
            self.curve.add_raster(tp, fp, det_score, nd, ng, gign if gign.dtype == torch.uint8 else gign.to(torch.uint8))
        return total - max_k, nd_total - self.max_d          # > 0: overflow (device tensors, read at the end of the pass)

    def _pick_chain(self):
        """the chain a pass runs per batch"""
        return self._chain if self.ms_scales is None else self._chain_multiscale

    def _overflow(self, worst):
        return 'an image selected %d pixels more than max_k: raise max_k or the score threshold' % worst

    # -- one pass --------------------------------------------------------------------------------
    def run(self):
        from .datasets import icdar
        from .tool import metrics
        self.acc.reset()
        if self.curve is not None:
            self.curve.reset()
        over_k, over_d, buckets = [], [], {}
        self._over_pool = []      # multi-scale only: per chain, int32 [n,2] = (pool_total - max_pool, non-finite rows)
        chain = self._pick_chain()

        def flush(items):
            a, b = chain(items)
            over_k.append(a)
            over_d.append(b)
        for im_fn, (polys, ignored) in self.samples:
            im = icdar.read_image_rgb(im_fn)
            key = tuple(im.shape[:2])
            items = buckets.setdefault(key, [])
            items.append((im, polys, ignored))
            if len(items) == self.batch_size:
                flush(buckets.pop(key))
        for key in sorted(buckets):
            flush(buckets[key])
        # the single read of the pass: the record and the two overflow maxima in one device-to-host copy
        worst = torch.stack([torch.cat(over_k).max(), torch.cat(over_d).max()])
        if self.ms_scales is not None:     # ... and the pool's two counts
            worst = torch.cat([worst, torch.cat(self._over_pool).max(dim=0).values.to(worst.dtype)])
        if self.curve is None:
            (num_gt, tp, fp, n_det), (worst_k, worst_d, *worst_pool) = self.acc.value_with(worst)
        else:       # ... and the curve, the order flag and AP in the same copy
            self.curve.finish(self.acc.record)
            (num_gt, tp, fp, n_det), (worst_k, worst_d, *worst_pool), rows, unsorted, ap = self.curve.value_with(self.acc, worst)
        if worst_pool:
            from .tool import rbox
            msg = rbox.overflow_error(worst_k, worst_pool[0], worst_pool[1], self.max_pool)
            if msg:
                raise ValueError(msg)
        if worst_k > 0:
            raise ValueError(self._overflow(worst_k))
        if worst_d > 0:
            raise ValueError('an image kept %d detections more than max_d = %d' % (worst_d, self.max_d))
        precision, recall = metrics.precision_recall(num_gt, tp, fp)
        hmean = metrics.fmean(precision, recall) if precision + recall > 0 else 0.0
        result = {'precision': precision, 'recall': recall, 'hmean': hmean, 'num_gt': num_gt, 'tp': tp, 'fp': fp,
                  'num_det': n_det, 'images': len(self.samples)}
        if self.protocol == 'icdar15':
            result.update(invalid_gt=self.invalid_gt, protocol=self.protocol)
        if self.curve is not None:
            if unsorted:
                raise ValueError('the detection scores of an image are not in descending order (NaNs last): the sweep '
                                 'and AP count score prefixes of the matching order')
            sweep, best = sweep_rows(self.curve.thresholds_host, rows)
            result.update(sweep=sweep, best=best, ap=ap)
        return result


class LinkEvaluator(Evaluator):
    """The link geometry: `forward(x)` returns the (pixel_cls [n,H/4,W/4,2], link_cls [n,H/4,W/4,16]) LOGITS of
    `PixelLinkNet` (tensors or head handles) as a pure launch sequence.  Every image is resized on the device to the
    fixed eval_image_height x eval_image_width (test_pixellink_fast.py's flags) and batched by its ORIGINAL shape, because
    ocr_min_area_rects takes one scale per call: a component pixel (x, y) of the 1/4-resolution maps becomes the point
    (int(x * scale_x), int(y * scale_y)) with scale_x = orig_w / (eval_w / 4), scale_y = orig_h / (eval_h / 4), so the
    boxes land in original-image pixels and ocr_eval_collect runs with ratios (1, 1).  An original side below a quarter
    of the eval side (a scale below 1) is refused.  A detection's score is its component's mean pixel score
    (ocr_component_scores; build-defined).  min_side / min_area filter the boxes (0: nothing, as the reference scripts).
    `run()` reads the device once at its end: the record, and the two overflow counts (components over max_comps,
    detections over max_d), either of which raises ValueError.  `sweep` as for `Evaluator`: its thresholds are on the
    component's mean pixel score, in [0, 1].

    map_scales / flip / scale_weights: None / False / None = the single-scale pass above, bit for bit.  `scales=` (box-level
    fusion) stays refused for this geometry; multi-scale and flip testing fuse the SCORE MAPS instead (DESIGN.md §3.3.20,
    include/ocr_map_fuse.h).  map_scales: 1 to 8 positive finite scales (1 need not be among them): every batch is resized
    from the ORIGINALS to each pixellink_fn.map_scale_sizes entry of the eval size and forwarded once, with flip=True a
    second time mirrored left to right; each pass's pixel and link probabilities are resampled onto the eval_hw / 4 grid
    and averaged with scale_weights (default: equal; a scale's two passes share its weight), and the link decode runs
    once on the fused maps.  The fusion grid is the single-scale one, so the box scales, the matcher, `protocol`, `sweep`
    and the single device read per pass are what they were.  flip without map_scales is scale 1 plus its mirror.
    Activation memory grows with the square of the largest scale.  Whether any of this raises the F-measure is
    unmeasured: no dataset or trained checkpoint is on any machine that built it."""

    def __init__(self, graph, forward, data, batch_size=8, max_images=None, matching_threshold=0.5, pixel_conf_threshold=0.8,
                 link_conf_threshold=0.9, min_size=10, max_comps=4096, min_side=0.0, min_area=0.0, max_d=ops.EVAL_MAX_D,
                 eval_image_height=768, eval_image_width=1280, gt_path=None, protocol='raster', sweep=None, scales=None,
                 map_scales=None, flip=False, scale_weights=None):
        if scales is not None:
            # the min-area-rectangle vertices of a component have no fixed correspondence across scales for the vote
            raise ValueError('multi-scale evaluation (scales=...) is built for the RBOX geometry only')
        from .tool import pixellink_fn
        self.flip = bool(flip)
        if map_scales is None and scale_weights is not None:
            raise ValueError('scale_weights come with map_scales')
        if map_scales is None and self.flip:
            map_scales = [1.0]                       # flip alone: scale 1 and its mirror
        self.map_scales, self.scale_weights = (None, None) if map_scales is None else \
            pixellink_fn.check_map_scales(map_scales, scale_weights)
        super().__init__(graph, forward, data, batch_size=batch_size, max_images=max_images,
                         matching_threshold=matching_threshold, max_d=max_d, gt_path=gt_path, protocol=protocol, sweep=sweep)
        self.eval_hw = (int(eval_image_height), int(eval_image_width))
        if min(self.eval_hw) < 4 or self.eval_hw[0] % 4 or self.eval_hw[1] % 4:
            raise ValueError('the eval size must be positive multiples of 4, got %dx%d' % self.eval_hw)
        if int(max_comps) < 1:
            raise ValueError('max_comps must be positive')
        self.pixel_conf_threshold, self.link_conf_threshold = float(pixel_conf_threshold), float(link_conf_threshold)
        self.min_size, self.max_comps = int(min_size), int(max_comps)
        self.min_side, self.min_area = float(min_side), float(min_area)

    def _resized(self, h, w):
        return self.eval_hw

    def _ratio(self, h, w, rh, rw):
        return 1.0, 1.0

    def scales(self, h, w):
        """(scale_x, scale_y) of an h x w original: 1/4-resolution map cell -> original-image pixels"""
        sx, sy = w / float(self.eval_hw[1] // 4), h / float(self.eval_hw[0] // 4)
        if sx < 1.0 or sy < 1.0:
            raise ValueError('a %dx%d image is smaller than the %dx%d score maps: lower the eval size'
                             % (h, w, self.eval_hw[0] // 4, self.eval_hw[1] // 4))
        return sx, sy

    def _chain(self, batch):
        from .tool import pixellink_fn
        g = self.g
        scale_x, scale_y = self.scales(*batch[0][0].shape[:2])
        x, inv_ratio, gts, ng, gign, mask_hw = self._upload(batch)
        pixel_cls, link_cls = self.forward(x)
        pixel_score = pixellink_fn.pixel_scores(pixel_cls, graph=g)[..., 1].contiguous()
        link_score = pixellink_fn.link_scores(link_cls, graph=g)
        merged, keep, n_keep, passed, total = pixellink_fn.detect_device(
            pixel_score, link_score, self.pixel_conf_threshold, self.link_conf_threshold, self.min_size, scale_x, scale_y,
            max_comps=self.max_comps, min_side=self.min_side, min_area=self.min_area, graph=g)
        return self._match(merged, keep, n_keep, passed, total, inv_ratio, gts, ng, gign, mask_hw)

    # -- score-map fusion (map_scales=..., flip=...): beside the single-scale chain, which it leaves as it is ---------
    def _passes(self, batch, srcs):
        """the forward passes of a batch, one at a time: every original resized to each map_scale_sizes entry, forwarded,
        and with `flip` forwarded again mirrored left to right.  A generator: fuse_score_maps uses a pass's logits up
        before it asks for the next forward, which may return the same buffers."""
        from .tool import pixellink_fn
        for rh, rw in pixellink_fn.map_scale_sizes(self.eval_hw[0], self.eval_hw[1], self.map_scales):
            x, _ = self._resize_batch(batch, srcs, rh, rw)
            pixel_cls, link_cls = self.forward(x)
            yield pixel_cls, link_cls, False
            if self.flip:
                pixel_cls, link_cls = self.forward(torch.flip(x, dims=[2]))
                yield pixel_cls, link_cls, True

    def _chain_fused(self, batch):
        from .tool import pixellink_fn
        g = self.g
        scale_x, scale_y = self.scales(*batch[0][0].shape[:2])
        gts, ng, gign, mask_hw = self._ground_truths(batch)
        weights = np.repeat(np.asarray(self.scale_weights, np.float64), 2 if self.flip else 1)
        # the fusion grid is the single-scale pass's: eval_hw / 4, so the box scales and everything behind them stay
        merged, keep, n_keep, passed, total = pixellink_fn.detect_device_multiscale(
            self._passes(batch, self._sources(batch)), weights, (self.eval_hw[0] // 4, self.eval_hw[1] // 4),
            self.pixel_conf_threshold, self.link_conf_threshold, self.min_size, scale_x, scale_y, max_comps=self.max_comps,
            min_side=self.min_side, min_area=self.min_area, graph=g)
        ones = torch.ones((len(batch), 2), dtype=torch.float32, device=g.device)
        return self._match(merged, keep, n_keep, passed, total, ones, gts, ng, gign, mask_hw)

    def _pick_chain(self):
        return self._chain if self.map_scales is None else self._chain_fused

    def _overflow(self, worst):
        return 'an image holds %d components more than max_comps = %d' % (worst, self.max_comps)


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
    `LinkEvaluator`'s map_scales / flip / scale_weights travel in **evaluator_kw."""

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
        also eval/ap, eval/best_hmean, eval/best_threshold."""
        for k in ('precision', 'recall', 'hmean'):
            writer.add_scalar('eval/' + k, self.last[k])
        if 'sweep' in self.last:
            writer.add_scalar('eval/ap', self.last['ap'])
            writer.add_scalar('eval/best_hmean', self.last['best']['hmean'])
            writer.add_scalar('eval/best_threshold', self.last['best']['threshold'])
        writer.flush_step(global_step)
