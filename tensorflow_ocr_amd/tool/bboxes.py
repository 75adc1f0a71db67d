"""Mirror of the evaluation half of the reference's tool/bboxes.py: detection / ground-truth matching
with RASTERISED IoU (`bboxes_matching` :171-240, `bboxes_jaccard` :242-245, `np_bboxes_jaccard`
:246-283).  The reference draws each pair of quadrangles into 0/1 masks with cv2 and counts pixels on
the host, once per detection inside a tf.while_loop; here all pairs of an image are counted in one
launch (ocr_quad_iou) and the sequential greedy matching — O(detections) scalar work — stays on the
host exactly as written.  `bboxes_matching_batch` is the same rule for a whole batch with the greedy pass on the device
too (ocr_eval_match_batch: no synchronisation, the totals added to a device record)."""
import numpy as np
import torch

from .. import ops
from ..graph import get_default_graph


def _pair_counts(bboxes, gxs, gys, graph=None):
    """(inter, union) int32 [n_det, n_gt] pixel counts of the filled rasters."""
    g = graph or get_default_graph()
    dets = np.asarray(bboxes).reshape(len(bboxes), 4, 2).astype(np.int32)         # points_to_contours: int32
    gts = np.stack([np.asarray(gxs), np.asarray(gys)], axis=-1).astype(np.int32)  # [G,4,2]
    # the reference sizes its masks per detection as max coordinate + 10 (:252-256); any size that
    # keeps every vertex inside gives the same raster, so one size serves all pairs
    xmax = int(max(dets[:, :, 0].max(), gts[:, :, 0].max())) + 10
    ymax = int(max(dets[:, :, 1].max(), gts[:, :, 1].max())) + 10
    if xmax <= 0 or ymax <= 0:
        raise ValueError("negative dimensions are not allowed")                    # np.zeros in util.img.black
    d_d = torch.from_numpy(dets).to(g.device)
    d_g = torch.from_numpy(gts).to(g.device)
    inter = torch.empty((len(dets), len(gts)), dtype=torch.int32, device=g.device)
    uni = torch.empty_like(inter)
    ops.quad_iou(d_d, d_g, ymax, xmax, inter, uni)
    return inter.cpu().numpy(), uni.cpu().numpy()


def np_bboxes_jaccard(bbox, gxs, gys, graph=None):
    """tool/bboxes.py:246-283: IoU of one detection (8 numbers) with every ground truth -> float32 [G]."""
    inter, uni = _pair_counts(np.reshape(bbox, (1, 8)), gxs, gys, graph)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter[0] * 1.0 / uni[0]).astype(np.float32)


bboxes_jaccard = np_bboxes_jaccard          # :242-245 (the tf.py_func wrapper)


def bboxes_matching_batch(dets, nd, gts, ng, gignored, matching_threshold=0.5, record=None, graph=None, mask_hw=None):
    """`bboxes_matching` for a batch, on the device and without a synchronisation (ocr_eval_match_batch): one grid counts
    the pairs of every image, one workgroup per image walks its detections.  All operands are DEVICE tensors:
    dets int32 [n,max_d,4,2] with nd int32 [n] rows per image in matching order (descending score), gts int32
    [n,max_g,4,2] with ng int32 [n] rows, gignored uint8 / bool [n,max_g].  record: int64 [4] device tensor that {ground
    truths not ignored, tp, fp, detections} are ADDED to (`metrics.DeviceTpFp.record`); None: a fresh zeroed one.
    mask_hw: the (h, w) the rasters are clipped to; any mask holding every vertex gives the reference's counts
    (its own masks are `max coordinate + 10`); default 32768 x 32768, the largest — a pair costs its bounding box, not
    the mask.  An image without ground truths makes every detection a false positive (the reference raises there).
    Returns (tp, fp, record): uint8 [n,max_d] (zero beyond nd) and the record."""
    g = graph or get_default_graph()
    n, max_d = dets.shape[:2]
    if gignored.dtype == torch.bool:
        gignored = gignored.to(torch.uint8)
    if record is None:
        record = torch.empty((4,), dtype=torch.int64, device=g.device)
        ops.eval_record_init(record)
    mask_h, mask_w = (32768, 32768) if mask_hw is None else (int(mask_hw[0]), int(mask_hw[1]))
    tp = torch.empty((n, max_d), dtype=torch.uint8, device=g.device)
    fp = torch.empty_like(tp)
    ops.eval_match_batch(dets, nd, gts, ng, gignored, float(matching_threshold), mask_h, mask_w, tp, fp, record, g.workspace())
    return tp, fp, record


def ic15_matching_batch(dets, nd, gts, ng, gdontcare, iou_thr=0.5, area_prec_thr=0.5, record=None, graph=None, inter=None):
    """The official ICDAR-2015 Task-1 matching for a batch, on the device and without a synchronisation
    (ocr_eval_ic15_match_batch, include/ocr_eval_ic15.h): polygon IoU instead of rasters, `###` ground truths as don't-care
    regions (a detection more than area_prec_thr inside one is left out of the count), ground-truth-major greedy
    matching with a strict iou > iou_thr.  Operands as `bboxes_matching_batch`; no mask extent is needed.  record: int64
    [4] device tensor that {care ground truths, matched, care detections - matched, detections} are ADDED to
    (`metrics.DeviceTpFp.record`, the same slots: precision_recall / fmean apply unchanged); None: a fresh zeroed one.
    inter: optional float64 [n,max_g,max_d] that receives the pair intersection areas.
    Returns (det_match, gt_match, record): int32 [n,max_d] (gt index, -1 unmatched, -2 don't-care; -1 beyond nd), int32
    [n,max_g] (det index, -1 unmatched, -2 don't-care or bow-tie; -1 beyond ng) and the record."""
    g = graph or get_default_graph()
    n, max_d = dets.shape[:2]
    if gdontcare.dtype == torch.bool:
        gdontcare = gdontcare.to(torch.uint8)
    if record is None:
        record = torch.empty((4,), dtype=torch.int64, device=g.device)
        ops.eval_record_init(record)
    det_match = torch.empty((n, max_d), dtype=torch.int32, device=g.device)
    gt_match = torch.empty((n, gts.shape[1]), dtype=torch.int32, device=g.device)
    ops.eval_ic15_match_batch(dets, nd, gts, ng, gdontcare, float(iou_thr), float(area_prec_thr), det_match, gt_match, record,
                              g.workspace(), inter=inter)
    return det_match, gt_match, record


def bboxes_matching(bboxes, gxs, gys, gignored, matching_threshold=0.5, scope=None, graph=None):
    """tool/bboxes.py:171-240.  bboxes [N,8] detections sorted by score, gxs/gys [G,4], gignored [G].
    Returns (n_gbboxes, tp_match bool [N], fp_match bool [N]): a detection is a TP when its best
    ground truth (first argmax) has IoU > threshold, is not ignored and was not matched before; an FP
    when that ground truth is not ignored and (already matched or IoU too low); neither when ignored."""
    bboxes = np.asarray(bboxes).reshape(-1, 8)
    gignored = np.asarray(gignored).astype(bool)
    n_gbboxes = int(np.count_nonzero(~gignored))
    n = len(bboxes)
    tp = np.zeros(n, bool)
    fp = np.zeros(n, bool)
    if n == 0:
        return n_gbboxes, tp, fp
    inter, uni = _pair_counts(bboxes, gxs, gys, graph)
    with np.errstate(divide="ignore", invalid="ignore"):
        jac = (inter * 1.0 / uni).astype(np.float32)
    gmatch = np.zeros(gignored.shape, bool)
    for i in range(n):
        idxmax = int(np.argmax(jac[i]))
        match = jac[i, idxmax] > matching_threshold
        existing_match = gmatch[idxmax]
        not_ignored = not gignored[idxmax]
        tp[i] = not_ignored and match and not existing_match
        fp[i] = not_ignored and (existing_match or not match)
        gmatch[idxmax] = gmatch[idxmax] or (not_ignored and match)
    return n_gbboxes, tp, fp
