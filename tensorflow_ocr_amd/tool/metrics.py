"""Mirror of the reference's tool/metrics.py (precision / recall / F bookkeeping over a test set):
`streaming_tp_fp_arrays` :31-64 (running totals in TF local variables -> a small accumulator here),
`precision_recall` :67-79, `fmean` :81-85.  Scalar host work."""
import numpy as np


def safe_divide(numerator, denominator):
    """tf_extended.math.safe_divide: 0 where the denominator is not positive."""
    return float(numerator) / float(denominator) if denominator > 0 else 0.0


class streaming_tp_fp_arrays:
    """tool/metrics.py:31-64: accumulates (num_gbboxes, tp, fp) over images; `.value` is the
    reference's `val` tuple, `.update(...)` its `update_op`."""

    def __init__(self):
        self.v_num_gbboxes = 0
        self.v_tp = np.zeros((0,), bool)
        self.v_fp = np.zeros((0,), bool)

    def update(self, num_gbboxes, tp, fp):
        self.v_num_gbboxes += int(np.sum(num_gbboxes))
        self.v_tp = np.concatenate([self.v_tp, np.asarray(tp, bool).reshape(-1)])
        self.v_fp = np.concatenate([self.v_fp, np.asarray(fp, bool).reshape(-1)])
        return self.value

    @property
    def value(self):
        return self.v_num_gbboxes, self.v_tp, self.v_fp


class DeviceTpFp:
    """`streaming_tp_fp_arrays` with the running totals on the device: owns the int64 [4] record {ground truths not
    ignored, tp, fp, detections} that `bboxes.bboxes_matching_batch(..., record=acc.record)` adds to, batch after batch,
    without a synchronisation.  `value()` is the single host read of a pass: (num_gbboxes, tp, fp, n_det) as Python
    ints — `precision_recall(num_gbboxes, tp, fp)` and `fmean` apply to them unchanged (they only sum tp and fp).
    `reads` counts the calls of `value()` / `value_with()`."""

    def __init__(self, graph=None):
        import torch
        from .. import ops
        from ..graph import get_default_graph
        self.g = graph or get_default_graph()
        self.record = torch.empty((4,), dtype=torch.int64, device=self.g.device)
        self.reads = 0
        self._init = ops.eval_record_init
        self.reset()

    def reset(self):
        self._init(self.record)

    def value(self):
        self.reads += 1
        num_gt, tp, fp, n_det = (int(v) for v in self.record.cpu().tolist())
        return num_gt, tp, fp, n_det

    def value_with(self, extra):
        """`value()` and the integers of the device tensor `extra` in ONE device-to-host copy: ((num_gbboxes, tp, fp,
        n_det), [extra values]).  Counts as one read."""
        import torch
        self.reads += 1
        host = [int(v) for v in torch.cat([self.record, extra.reshape(-1).to(torch.int64)]).cpu().tolist()]
        return tuple(host[:4]), host[4:]


class DeviceGrid:
    """`DeviceTpFp` for a decode-threshold grid (evaluate.LinkEvaluator(grid=...)): owns the int64 [G,4] records, one
    `DeviceTpFp.record` per grid point — the matcher of point g adds to `records[g]`; `record` is row 0, the evaluator's own
    pair.  `value_with(extra)` is the single host read of a pass: ([(num_gbboxes, tp, fp, n_det)] * G, [extra values]) in
    ONE device-to-host copy, as `DeviceTpFp.value_with` makes it.  `reads` counts its calls."""

    def __init__(self, points, graph=None):
        import torch
        from .. import ops
        from ..graph import get_default_graph
        self.g = graph or get_default_graph()
        self.G = int(points)
        if self.G < 1:
            raise ValueError('a grid holds at least one point')
        self.records = torch.empty((self.G, 4), dtype=torch.int64, device=self.g.device)
        self.record = self.records[0]
        self.reads = 0
        self._init = ops.eval_record_init
        self.reset()

    def reset(self):
        for row in self.records:
            self._init(row)

    def value_with(self, extra):
        import torch
        self.reads += 1
        host = [int(v) for v in torch.cat([self.records.reshape(-1), extra.reshape(-1).to(torch.int64)]).cpu().tolist()]
        rows = [tuple(host[4 * k:4 * k + 4]) for k in range(self.G)]
        return rows, host[4 * self.G:]


class DeviceCurve:
    """The score-threshold sweep of a pass beside `DeviceTpFp` (include/ocr_eval_curve.h): owns, on the device, the int64
    [T,4] curve (row t = the record's four slots with only the detections of score >= thresholds[t] kept, so
    `precision_recall` / `fmean` apply per row), the `unsorted` flag, the AP pool of `n_images` x `max_d` slots and the
    AP scalar.  `add_raster` / `add_ic15` count one batch from the matcher's outputs, in the order the batches come
    (the image sequence of the pool); `finish(record)` computes AP once; `value_with(acc, extra)` is the single host
    read of a pass."""

    def __init__(self, thresholds, n_images, max_d, graph=None):
        import torch
        from .. import ops
        from ..graph import get_default_graph
        self.g = graph or get_default_graph()
        self.thresholds_host = [float(t) for t in thresholds]
        T = len(self.thresholds_host)
        if not 1 <= T <= ops.EVAL_MAX_T:
            raise ValueError('a sweep takes 1 to %d thresholds, got %d' % (ops.EVAL_MAX_T, T))
        if int(n_images) < 1 or not 1 <= int(max_d) <= ops.EVAL_MAX_D:
            raise ValueError('the AP pool needs n_images >= 1 and max_d in [1, %d]' % ops.EVAL_MAX_D)
        dev = self.g.device
        self.T, self.n_images, self.max_d = T, int(n_images), int(max_d)
        self.thresholds = torch.tensor(self.thresholds_host, dtype=torch.float32, device=dev)
        # one int64 buffer, so that the read is one slice: curve [T][4] | AP (f64 bit pattern) | unsorted (low int32)
        self.state = torch.empty((4 * T + 2,), dtype=torch.int64, device=dev)
        self.curve = self.state[:4 * T].view(T, 4)
        self.ap = self.state[4 * T:4 * T + 1].view(torch.float64)
        self.unsorted = self.state[4 * T + 1:].view(torch.int32)[:1]
        self.pool_score = torch.empty((self.n_images, self.max_d), dtype=torch.float32, device=dev)
        self.pool_cum = torch.empty((self.n_images, self.max_d, 2), dtype=torch.int32, device=dev)
        self.pool_nd = torch.empty((self.n_images,), dtype=torch.int32, device=dev)
        self._ops = ops
        self.reset()

    def reset(self):
        self.state[4 * self.T + 1:].zero_()         # (the flag's upper half; the entry zeroes the rest)
        self._ops.eval_curve_init(self.curve, self.unsorted, self.ap)
        self.pool_nd.zero_()
        self.seq = 0

    def _rows(self, n):
        if self.seq + n > self.n_images:
            raise ValueError('the AP pool holds %d images, batch rows %d..%d do not fit' % (self.n_images, self.seq, self.seq + n))
        s = slice(self.seq, self.seq + n)
        self.seq += n
        return self.pool_score[s], self.pool_cum[s], self.pool_nd[s]

    def add_raster(self, tp, fp, det_score, nd, ng, gignored):
        self._ops.eval_curve_batch(tp, fp, det_score, nd, ng, gignored, self.thresholds, self.curve, self.unsorted,
                                   pool=self._rows(tp.shape[0]))

    def add_ic15(self, det_match, gt_match, det_score, nd, ng):
        self._ops.eval_ic15_curve_batch(det_match, gt_match, det_score, nd, ng, self.thresholds, self.curve, self.unsorted,
                                        pool=self._rows(det_match.shape[0]))

    def finish(self, record):
        """AP over the pooled detections of the pass; G = record[0], read on the device"""
        self._ops.eval_ap(self.pool_score, self.pool_cum, self.pool_nd, record, self.ap, self.g.workspace())

    def value_with(self, acc, extra):
        """`acc.value_with(extra)` and the curve, the flag and AP in ONE device-to-host copy (the f64 travels as its int64
        bit pattern): ((num_gbboxes, tp, fp, n_det), [extra values], curve rows [T][4], unsorted, ap).  Counts as one
        read of `acc`."""
        import struct
        import torch
        acc.reads += 1
        n_extra = extra.numel()
        host = [int(v) for v in torch.cat([acc.record, extra.reshape(-1).to(torch.int64), self.state]).cpu().tolist()]
        rest = host[4 + n_extra:]
        rows = [rest[4 * t:4 * t + 4] for t in range(self.T)]
        ap = struct.unpack('<d', struct.pack('<q', rest[4 * self.T]))[0]
        return tuple(host[:4]), host[4:4 + n_extra], rows, rest[4 * self.T + 1] & 0xffffffff, ap


def precision_recall(num_gbboxes, tp, fp, scope=None):
    """tool/metrics.py:67-79 -> (precision, recall)."""
    tp = float(np.sum(np.asarray(tp, np.float32)))
    fp = float(np.sum(np.asarray(fp, np.float32)))
    recall = safe_divide(tp, float(num_gbboxes))
    precision = safe_divide(tp, tp + fp)
    return precision, recall


def fmean(pre, rec):
    """tool/metrics.py:81-85."""
    return 2 * pre * rec / (pre + rec)
