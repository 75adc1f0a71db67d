"""EAST RBOX post-processing on the GPU: per-pixel quad decode (the inverse of the RBOX geometry, reference
datasets/icdar.py:410-483 `restore_rectangle_rbox`) chained into locality-aware NMS (tool/lanms.py).

Two deliberate deviations from the reference's NumPy routine: the quads stay in RASTER order (the reference returns the
theta >= 0 rows before the theta < 0 rows; LANMS needs raster order) and the whole chain runs on the device with one
host synchronisation at its end.  `detect(box_thresh=...)` adds the filter EAST's eval script applies after the NMS: a
kept quad stays when the mean of the score map over its raster is above the threshold (ocr_quad_mean_score).  The RBOX
ground-truth maps are datasets/icdar.generate_rbox_batch(geometry='RBOX')."""
import numpy as np
import torch

from .. import ops
from ..graph import F32, get_default_graph
from . import lanms

LANMS_MAX_K = 32768     # the largest quad list per image ocr_lanms accepts


def _maps(g, score_map, geo_map):
    def dev(t):
        if hasattr(t, "data") and not isinstance(t, (torch.Tensor, np.ndarray)):
            t = t.data                                          # a head handle of model_rbox
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t, np.float32))
        return t.to(device=g.device, dtype=F32).contiguous()
    score, geo = dev(score_map), dev(geo_map)
    if geo.dim() != 4 or geo.shape[-1] != 5:
        raise ValueError("geo_map must be [n, h, w, 5], got %s" % (tuple(geo.shape),))
    n, h, w, _ = geo.shape
    if score.numel() != n * h * w:
        raise ValueError("score_map %s does not cover geo_map %s" % (tuple(score.shape), tuple(geo.shape)))
    return score, geo, n, h, w


def decode(score_map, geo_map, score_map_thresh=0.8, scale=4.0, max_k=None, graph=None):
    """score_map [n,h,w(,1)], geo_map [n,h,w,5] (host arrays, device tensors or the handles of model_rbox) -> device
    (boxes f32 [n,max_k,9], counts int32 [n], total int32 [n]): per image the quads of the pixels with score >
    score_map_thresh in raster order, coordinates in units of `scale` pixels per map cell; total = the number selected,
    counts = min(total, max_k).  max_k defaults to min(h * w, 32768), the bound LANMS accepts.  No host sync."""
    g = graph or get_default_graph()
    score, geo, n, h, w = _maps(g, score_map, geo_map)
    if max_k is None:
        max_k = min(h * w, LANMS_MAX_K)
    max_k = int(max_k)
    if max_k < 1:
        raise ValueError("max_k must be positive")
    boxes = torch.empty((n, max_k, 9), dtype=F32, device=g.device)
    counts = torch.empty((n,), dtype=torch.int32, device=g.device)
    total = torch.empty((n,), dtype=torch.int32, device=g.device)
    ops.rbox_decode(score, geo, n, h, w, float(score_map_thresh), float(scale), boxes, counts, total, g.workspace())
    return boxes, counts, total


def quad_mean_scores(quads, valid, score, graph=None):
    """quads f32 [n,k,8] (image px), valid bool [n,k], score f32 [n,h,w], all on the device -> f32 [n,k]: per valid quad the
    mean of its image's score map over the fillPoly raster of `quad.astype(np.int32) // 4`; 0 for the others (their rows
    are handed to the kernel as NaN, which it answers without rasterising).  One launch per image, no host sync."""
    g = graph or get_default_graph()
    n, k, _ = quads.shape
    q = torch.where(valid[..., None], quads, torch.full((), float("nan"), dtype=F32, device=g.device)).contiguous()
    means = torch.empty((n, k), dtype=F32, device=g.device)
    for i in range(n):
        ops.quad_mean_score(q[i], score[i], 0.25, means[i])
    return means


def detect_device(score_map, geo_map, score_map_thresh=0.8, nms_thres=0.2, max_k=None, graph=None, box_thresh=None):
    """The device part of `detect`: decode + lanms.lanms_batch (+ the mean-score mask of box_thresh), NO synchronisation.
    Returns device tensors (merged f32 [n,max_k,9], keep int32 [n,max_k], n_keep int32 [n], passed bool [n,max_k] or None,
    total int32 [n]): image i's kept quads are merged[i][keep[i, :n_keep[i]]], of which passed[i, :n_keep[i]] survive the
    filter; total[i] > max_k means candidates were dropped, which the caller must turn into an error once it reads it."""
    g = graph or get_default_graph()
    boxes, counts, total = decode(score_map, geo_map, score_map_thresh, 4.0, max_k, graph=g)
    if boxes.shape[1] > LANMS_MAX_K:
        raise ValueError("max_k %d is beyond the %d quads per image LANMS accepts" % (boxes.shape[1], LANMS_MAX_K))
    merged, _, keep, n_keep = lanms.lanms_batch(boxes, counts, nms_thres, graph=g)
    passed = None
    if box_thresh is not None:
        valid, means = kept_mean_scores(score_map, geo_map, merged, keep, n_keep, graph=g)
        passed = valid & (means > float(box_thresh))
    return merged, keep, n_keep, passed, total


def kept_mean_scores(score_map, geo_map, merged, keep, n_keep, graph=None):
    """LANMS output -> (valid bool [n,max_k], means f32 [n,max_k]) per KEEP SLOT: slot j of image i is valid when j <
    n_keep[i], and its mean is quad_mean_scores of merged[i][keep[i, j]] on the image's score map (0 for the others).
    No host sync."""
    g = graph or get_default_graph()
    score, _, n, h, w = _maps(g, score_map, geo_map)
    k = merged.shape[1]
    valid = torch.arange(k, device=g.device)[None, :] < n_keep[:, None]
    idx = torch.where(valid, keep, torch.zeros_like(keep)).long().clamp_(0, k - 1)
    kept = torch.gather(merged[..., :8], 1, idx[..., None].expand(-1, -1, 8))
    return valid, quad_mean_scores(kept, valid, score.reshape(n, h, w), graph=g)


def detect(score_map, geo_map, score_map_thresh=0.8, nms_thres=0.2, max_k=None, graph=None, box_thresh=None):
    """decode + lanms.lanms_batch on the device, one synchronisation at the end.  Returns one [m, 9] array of kept quads
    (merged coordinates, summed scores) per image.  Raises ValueError when an image selects more than max_k pixels:
    candidates are never dropped silently.  box_thresh: None = no filter; a number = only the kept quads whose mean
    score over their raster (quad_mean_scores) is STRICTLY above it, EAST's `box_thresh` (0.1 there); the means are
    computed on the device in front of the same single synchronisation."""
    merged, keep, n_keep, passed, total = detect_device(score_map, geo_map, score_map_thresh, nms_thres, max_k, graph, box_thresh)
    total_h = total.cpu().numpy()                               # the single sync: everything below is already computed
    if (total_h > merged.shape[1]).any():
        raise ValueError("%s pixels above the threshold, max_k = %d: raise max_k or the threshold"
                         % (total_h.tolist(), merged.shape[1]))
    n_keep_h = n_keep.cpu().numpy()
    merged_h, keep_h = merged.cpu().numpy(), keep.cpu().numpy()
    out = [merged_h[i][keep_h[i, :n_keep_h[i]]] for i in range(len(total_h))]
    if passed is not None:
        passed_h = passed.cpu().numpy()
        out = [q[passed_h[i, :n_keep_h[i]]] for i, q in enumerate(out)]
    return out


# ------------------------------------------------------------------------------------------------ multi-scale inference
MAX_SCALES = 8
FUSE_MODES = ('nms', 'vote')


def check_scales(scales):
    """1 to 8 positive finite numbers -> a list of floats; ValueError otherwise"""
    try:
        values = [float(s) for s in scales]
    except TypeError:
        raise ValueError('scales must be a sequence of numbers, got %r' % (scales,))
    if not 1 <= len(values) <= MAX_SCALES:
        raise ValueError('multi-scale inference takes 1 to %d scales, got %d' % (MAX_SCALES, len(values)))
    for s in values:
        if not (np.isfinite(s) and s > 0):
            raise ValueError('a scale must be positive and finite, got %r' % (s,))
    return values


def scale_sizes(h, w, scales, max_side_len=3000):
    """The network input sizes of an h x w image at each scale: [(rh_s, rw_s)] with (rh_s, rw_s) =
    evaluate.resize_rule(int(round(h * s)), int(round(w * s)), max_side_len), every size made from the ORIGINAL image.
    ValueError unless `scales` holds 1 to 8 positive finite numbers that give distinct sizes; a scale at which the sizing
    rule fails is named in the error."""
    from ..evaluate import resize_rule
    values = check_scales(scales)
    sizes = []
    for s in values:
        try:
            size = resize_rule(int(round(h * s)), int(round(w * s)), max_side_len)
        except ValueError as e:
            raise ValueError('scale %g: %s' % (s, e))
        if size in sizes:
            raise ValueError('scale %g gives the size %dx%d of scale %g again' % ((s,) + size + (values[sizes.index(size)],)))
        sizes.append(size)
    return sizes


def parse_scales(text):
    """--scales / --eval_scales: a comma list of numbers -> a list of floats (checked again, against an image size, by
    `scale_sizes`); ValueError otherwise."""
    values = [float(v) for v in str(text).split(',') if v.strip()]
    if not 1 <= len(values) <= MAX_SCALES or not all(np.isfinite(v) and v > 0 for v in values) or \
            len(set(values)) != len(values):
        raise ValueError('scales are 1 to %d distinct positive numbers, got %r' % (MAX_SCALES, text))
    return values


def scales_arg(text):
    """`parse_scales` as an argparse type"""
    import argparse
    try:
        return parse_scales(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def detect_multiscale_device(maps, ratios, score_map_thresh=0.8, nms_thres=0.2, box_thresh=None, fuse='nms', fuse_thres=None,
                             max_pool=1024, max_k=None, graph=None):
    """Multi-scale detection of a batch, NO synchronisation.  `maps`: one (score_map, geo_map) per scale, as `detect_device`
    takes them — any iterable; it is consumed one scale at a time and a scale's maps are used up before the next item is
    asked for, so a generator may run each forward lazily into buffers the next one reuses.  `ratios`: one f32 [n,2]
    device tensor (ratio_w, ratio_h) per scale.  Per scale: `detect_device`, the mean pixel score of every kept quad on that
    scale's score map (always: it is the pooled score, in [0, 1] and comparable across scales, unlike LANMS's sum; with
    box_thresh it is also the filter, STRICTLY above), then ops.ms_pool_append in original-image pixels.  After the last
    scale one ops.quad_fuse over the pool: fuse = 'nms' (score-ordered suppression) or 'vote' (the kept quads' coordinates
    become the score-weighted mean of the quads they claimed), threshold fuse_thres (default: nms_thres).
    Returns (fused f32 [n,max_pool,9], keep int32 [n,max_pool], n_keep int32 [n], overflow int32 [n,3]): image i's quads are
    fused[i][keep[i, :n_keep[i]]] in descending score order — the layout ops.eval_collect reads — and overflow[i] =
    (the worst total - max_k over the scales, pool_total - max_pool, the non-finite rows dropped): any entry > 0 means
    candidates were lost, which the caller must turn into an error once it reads it."""
    g = graph or get_default_graph()
    if fuse not in FUSE_MODES:
        raise ValueError("fuse must be 'nms' or 'vote', got %r" % (fuse,))
    max_pool = int(max_pool)
    if not 1 <= max_pool <= ops.FUSE_MAX_POOL:
        raise ValueError('max_pool must be in [1, %d]' % ops.FUSE_MAX_POOL)
    ratios = list(ratios)
    if not 1 <= len(ratios) <= MAX_SCALES:
        raise ValueError('multi-scale inference takes 1 to %d scales, got %d' % (MAX_SCALES, len(ratios)))
    fuse_thres = float(nms_thres if fuse_thres is None else fuse_thres)
    pool = pool_scale = counters = worst_k = None
    n_scales = 0
    for s, (score_map, geo_map) in enumerate(maps):
        if s >= len(ratios):
            raise ValueError('more maps than ratios (%d)' % len(ratios))
        merged, keep, n_keep, _, total = detect_device(score_map, geo_map, score_map_thresh, nms_thres, max_k, graph=g)
        valid, means = kept_mean_scores(score_map, geo_map, merged, keep, n_keep, graph=g)
        passed = None if box_thresh is None else (valid & (means > float(box_thresh))).to(torch.uint8)
        n = merged.shape[0]
        if pool is None:
            pool = torch.empty((n, max_pool, 9), dtype=F32, device=g.device)
            pool_scale = torch.empty((n, max_pool), dtype=torch.int32, device=g.device)
            counters = torch.zeros((3, n), dtype=torch.int32, device=g.device)      # count, total, non-finite
        over = total - merged.shape[1]
        worst_k = over if worst_k is None else torch.maximum(worst_k, over)
        ratio = ratios[s].to(device=g.device, dtype=F32).contiguous()
        ops.ms_pool_append(merged, keep, n_keep, passed, means, ratio, s, pool, pool_scale, counters[0], counters[1],
                           counters[2])
        n_scales += 1
    if n_scales != len(ratios):
        raise ValueError('%d maps for %d ratios' % (n_scales, len(ratios)))
    fused = torch.empty_like(pool)
    keep = torch.empty_like(pool_scale)
    owner = torch.empty_like(pool_scale)
    n_keep = torch.empty((pool.shape[0],), dtype=torch.int32, device=g.device)
    ops.quad_fuse(pool, counters[0], fuse_thres, fuse, fused, keep, n_keep, owner, g.workspace())
    overflow = torch.stack([worst_k.to(torch.int32), counters[1] - max_pool, counters[2]], dim=1)
    return fused, keep, n_keep, overflow


def overflow_error(worst_k, worst_pool, nonfinite, max_pool):
    """the message for the overflow counts of `detect_multiscale_device`, or None when all are <= 0"""
    if worst_k > 0:
        return 'an image selected %d pixels more than max_k at one scale: raise max_k or the score threshold' % worst_k
    if worst_pool > 0:
        return 'an image pooled %d quads more than max_pool = %d over its scales' % (worst_pool, max_pool)
    if nonfinite > 0:
        return '%d pooled quads had a non-finite coordinate or score' % nonfinite
    return None


def detect_multiscale(maps, ratios, score_map_thresh=0.8, nms_thres=0.2, box_thresh=None, fuse='nms', fuse_thres=None,
                      max_pool=1024, max_k=None, graph=None):
    """`detect_multiscale_device` with the single synchronisation at its end.  Returns one [m, 9] array per image: the fused
    quads in ORIGINAL-image pixels, column 8 the mean pixel score, in descending score order.  Raises ValueError on any of
    the three overflow counts: candidates are never dropped silently."""
    fused, keep, n_keep, overflow = detect_multiscale_device(maps, ratios, score_map_thresh, nms_thres, box_thresh, fuse,
                                                             fuse_thres, max_pool, max_k, graph)
    over_h = overflow.cpu().numpy()                             # the single sync: everything below is already computed
    msg = overflow_error(*over_h.max(axis=0).tolist(), max_pool=int(max_pool))
    if msg:
        raise ValueError(msg)
    n_keep_h = n_keep.cpu().numpy()
    fused_h, keep_h = fused.cpu().numpy(), keep.cpu().numpy()
    return [fused_h[i][keep_h[i, :n_keep_h[i]]] for i in range(len(n_keep_h))]
