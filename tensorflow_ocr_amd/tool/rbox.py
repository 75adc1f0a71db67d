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
        score, _, n, h, w = _maps(g, score_map, geo_map)
        k = boxes.shape[1]
        valid = torch.arange(k, device=g.device)[None, :] < n_keep[:, None]
        idx = torch.where(valid, keep, torch.zeros_like(keep)).long().clamp_(0, k - 1)
        kept = torch.gather(merged[..., :8], 1, idx[..., None].expand(-1, -1, 8))
        passed = valid & (quad_mean_scores(kept, valid, score.reshape(n, h, w), graph=g) > float(box_thresh))
    return merged, keep, n_keep, passed, total


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
