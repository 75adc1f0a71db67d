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
