"""Records tests/golden/ops_calls.json: for every decode / label / resize / evaluation / multi-scale / map-fusion / grid /
summary wrapper of `tensorflow_ocr_amd.ops`, the C-ABI calls one valid operand set makes — the entry's name and, per
argument, the ctypes type and the value; a pointer is written as the name of the operand it points to, "ws" or "null".
Nothing is launched: the stream is pinned, `_lib.call` / `call_size` / `call_int` are recorders (a size query answers
WS_BYTES), the operands are tiny CPU tensors and `ws` hands out a CPU buffer.  tests/test_ops_operands_host.py requires
the same table and derives its faults from the same operand sets: run this on the commit whose wrappers are to be kept,
BEFORE changing ops.py.  It uses only the wrappers' public signatures, so the same file runs on both sides.  No GPU needed.

    python tests/golden/make_ops_calls.py"""
import contextlib
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "ops_calls.json")
WS_BYTES = 256
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def operand_sets():
    """wrapper -> its arguments by parameter name.  Every tensor (and every tensor of a tuple) is an operand; the sizes
    are the smallest that keep the dimensions of one wrapper distinct."""
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt)
    i, u = (lambda *s: z(*s, dt=I32)), (lambda *s: z(*s, dt=U8))
    n, k, d, g, h, w, T, G, P, V, c, p = 2, 5, 3, 4, 6, 7, 3, 2, 3, 4, 5, 8    # k = max_k, d = max_d, g = max_g, c = max_comps, p = max_pool
    lanms_out = lambda m: dict(merged=z(n, m, 9), keep_idx=i(n, m), n_keep=i(n))
    curve = lambda: dict(det_score=z(n, d), nd=i(n), ng=i(n), thresholds=z(T), curve=z(T, 4, dt=I64), unsorted=i(1),
                         pool=(z(n, d), i(n, d, 2), i(n)))
    hulls = lambda: dict(hull_n=i(n, c), hull_head=i(n, c, 4), calipers=z(n, c, 6))
    cc = lambda: dict(pixel_score=z(n, h, w), link_score=z(8, n, h, w, 2), stride=2, offset=1, n=n, h=h, w=w, pixel_thresh=0.5,
                      link_thresh=0.25, min_size=1)
    return {
        "softmax_pairs": dict(logits=z(n, h, w, 2), probs=z(n, h, w, 2)),
        "link_softmax_stack": dict(link_logits=z(n, h, w, 16), out=z(8, n, h, w, 2)),
        "pixel_detect": dict(score_map=z(n, h, w, 1), link_scores=z(8, n, h, w, 2), n=n, h=h, w=w, score_thresh=0.5,
                             link_thresh=0.25, mask=u(h, w)),
        "link_cc": dict(cc(), labels=i(n, h, w), ncomp=i(n), comps=i(n, c, 2), ws=None),
        "link_cc_directed": dict(cc(), union_labels=i(n, h, w), union_ncomp=i(n), labels=i(n, h, w), ncomp=i(n), comps=i(n, c, 2),
                                 ws=None, seed_order=i(n, h * w)),
        "lanms": dict(boxes=z(n, k, 9), counts=i(n), iou_thresh=0.25, merged=z(n, k, 9), n_merged=i(n), keep_idx=i(n, k),
                      n_keep=i(n), ws=None),
        "rbox_decode": dict(score=z(n, h, w), geo=z(n, h, w, 5), n=n, h=h, w=w, score_thresh=0.5, scale=4.0, boxes=z(n, k, 9),
                            counts=i(n), total=i(n), ws=None),
        "quad_mean_score": dict(quads=z(k, 8), score=z(h, w), inv_scale=0.25, mean=z(k)),
        "min_area_rects": dict(labels=i(n, h, w), ncomp=i(n), max_comps=c, scale_x=4.0, scale_y=2.0, **hulls(), ws=None),
        "mask_cc": dict(mask=u(n, h, w), value=1, connectivity=8, labels=i(n, h, w), ncomp=i(n), comps=i(n, c, 2), ws=None),
        "hole_border_rects": dict(mask=u(n, h, w), zlabels=i(n, h, w), nregions=i(n), max_regions=c, scale_x=4.0, scale_y=2.0,
                                  **hulls(), ws=None),
        "east_pixel_detect": dict(score=z(h, w), link16=z(h, w, 16), h=h, w=w, score_thresh=0.5, link_thresh=0.25, mask=u(h, w),
                                  first_second=i(2, 8)),
        "contour_parents": dict(labels=i(1, h, w), zlabels=i(1, h, w), comps=i(1, c, 2), ncomp=3, zcomps=i(1, c, 2), nregions=2,
                                parent_c=i(3), parent_z=i(2)),
        "zero_pixels": dict(mask=u(h, w), idx=i(T)),
        "poly_cover": dict(polys=i(n, P, V, 2), counts=i(n), ignore=u(n, P), h=h, w=w, cover=i(n, h, w)),
        "icdar_labels": dict(cover=i(n, 8, 8), step=4, score=z(n, 2, 2, 1), geo=z(n, 2, 2, 8), mask=z(n, 2, 2, 1)),
        "rbox_labels": dict(cover_score=i(n, h, w), cover_full=i(n, h, w), rects=z(n, P, 5, 3), step=4, score=z(n, 2, 2, 1),
                            geo=z(n, 2, 2, 5), mask=z(n, 2, 2, 1)),
        "pixellink_labels": dict(cover=i(n, h, w), new_h=3, new_w=4, score=z(n, 3, 4), link=z(n, 3, 4, 8)),
        "pixellink_instance_weights": dict(cover=i(n, h, w), ignore=u(n, P), new_h=3, new_w=4, area=i(n, P), weight=z(n, 3, 4)),
        "resize_linear_u8": dict(src_u8=u(h, w, 3), dst_f32=z(4, 5, 3)),
        "augment_u8_batch": dict(slab=u(h * w * 3 * n), desc=u(112 * n), n=n, S=4, dst=z(n, 4, 4, 3)),
        "resize_cubic_f32": dict(src_f32=z(n, h, w), dst_f32=z(n, 4, 5), pre_scale=255.0, post_scale=0.5),
        "quad_iou": dict(dets=i(d, V, 2), gts=i(g, V, 2), mask_h=h, mask_w=w, inter=i(d, g), uni=i(d, g)),
        "eval_collect": dict(lanms_out(k), passed=u(n, k), inv_ratio=z(n, 2), dets=i(n, d, 4, 2), det_score=z(n, d), nd=i(n),
                             nd_total=i(n)),
        "eval_match_batch": dict(dets=i(n, d, 4, 2), nd=i(n), gts=i(n, g, 4, 2), ng=i(n), gignored=u(n, g), threshold=0.5,
                                 mask_h=h, mask_w=w, tp=u(n, d), fp=u(n, d), record=z(4, dt=I64), ws=None),
        "eval_ic15_match_batch": dict(dets=i(n, d, 4, 2), nd=i(n), gts=i(n, g, 4, 2), ng=i(n), gdontcare=u(n, g), iou_thr=0.5,
                                      area_prec_thr=0.25, det_match=i(n, d), gt_match=i(n, g), record=z(4, dt=I64), ws=None,
                                      inter=z(n, g, d, dt=F64)),
        "eval_record_init": dict(record=z(4, dt=I64)),
        "eval_curve_init": dict(curve=z(T, 4, dt=I64), unsorted=i(1), ap=z(1, dt=F64)),
        "eval_curve_batch": dict(tp=u(n, d), fp=u(n, d), gignored=u(n, g), **curve()),
        "eval_ic15_curve_batch": dict(det_match=i(n, d), gt_match=i(n, g), **curve()),
        "eval_ap": dict(pool_score=z(n, d), pool_cum=i(n, d, 2), pool_nd=i(n), record=z(4, dt=I64), ap=z(1, dt=F64), ws=None),
        "ms_pool_append": dict(lanms_out(k), passed=u(n, k), mean=z(n, k), ratio=z(n, 2), scale_id=1, pool=z(n, p, 9),
                               pool_scale=i(n, p), pool_count=i(n), pool_total=i(n), pool_nonfinite=i(n)),
        "quad_fuse": dict(pool=z(n, p, 9), pool_count=i(n), iou_thresh=0.25, mode="vote", fused=z(n, p, 9), keep_idx=i(n, p),
                          n_keep=i(n), owner=i(n, p), ws=None),
        "link_map_accumulate": dict(pixel_logits=z(n, 3, 4, 2), link_logits=z(n, 3, 4, 16), flip=True, weight=0.5, first=False,
                                    acc=z(9, n, h, w)),
        "component_scores": dict(labels=i(n, h, w), pixel_score=z(n, h, w), ncomp=i(n), comp_score=z(n, c), ws=None),
        "link_boxes": dict(hulls(), comp_score=z(n, c), ncomp=i(n), min_side=1.5, min_area=2.5, **lanms_out(c), passed=u(n, c),
                           total=i(n)),
        "link_cc_grid": dict(pixel_score=z(n, h, w), link_score=z(8, n, h, w, 2), stride=2, offset=1, pixel_thresholds=[0.5, 0.75],
                             link_thresholds=[0.25, 0.5], min_size=1, labels=i(G * n, h, w), ncomp=i(G * n), comps=i(G * n, c, 2),
                             ws=None),
        "component_scores_grid": dict(labels=i(G * n, h, w), pixel_score=z(n, h, w), ncomp=i(G * n), comp_score=z(G * n, c),
                                      ws=None),
        "tensor_stats": dict(x=z(h * w), table=z(16, dt=I64), n_segments=2, mul_host=0.5, mul_dev=z(1), records=u(2 * WS_BYTES),
                             ws=z(8, dt=F64)),
        "summary_image_u8": dict(x=z(h, w, 3), out=u(h, w, 3), ws=z(WS_BYTES // 4)),
    }


# what a test needs to know beyond the sets: the arguments that may be None; the operands whose element type is free (byte
# buffers); and, per operand, the dimension whose size + 1 is a fault of that operand ("rank": one dimension more, for an
# operand whose sizes are all free; a tuple: that shape, where a size is free but not every count is taken; None: every
# shape is taken).  Default: the last dimension.
OPTIONAL = {"link_cc_directed": ["seed_order"], "eval_collect": ["passed"], "eval_ic15_match_batch": ["inter"],
            "eval_curve_init": ["ap"], "eval_curve_batch": ["pool"], "eval_ic15_curve_batch": ["pool"], "ms_pool_append": ["passed"],
            "tensor_stats": ["mul_dev"]}
RAW = {"tensor_stats": ["table", "records", "ws"], "summary_image_u8": ["ws"]}
TUPLES = {"pool": ("pool_score", "pool_cum", "pool_nd")}
WS_TENSOR = ("tensor_stats", "summary_image_u8")           # their `ws` is an operand of the caller's, not an arena
DIM = {
    "softmax_pairs": {"logits": (3, 7, 1)}, "link_softmax_stack": {"link_logits": (2, 6, 7, 15)},
    "quad_mean_score": {"score": "rank"}, "min_area_rects": {"labels": "rank", "hull_n": 0},
    "mask_cc": {"mask": "rank"}, "hole_border_rects": {"mask": "rank", "hull_n": 0},
    "contour_parents": {"labels": None, "comps": None, "zcomps": None, "parent_c": None, "parent_z": None},
    "zero_pixels": {"mask": None, "idx": None}, "icdar_labels": {"cover": "rank"}, "rbox_labels": {"cover_score": "rank"},
    "pixellink_labels": {"cover": "rank"}, "pixellink_instance_weights": {"cover": "rank", "ignore": 0},
    "resize_linear_u8": {"src_u8": "rank"}, "augment_u8_batch": {"slab": None, "desc": None},
    "resize_cubic_f32": {"src_f32": "rank", "dst_f32": 0}, "quad_iou": {"inter": 0},
    "eval_match_batch": {"gignored": 0}, "eval_ic15_match_batch": {"gdontcare": 0, "gt_match": 0},
    "eval_curve_batch": {"tp": "rank", "gignored": 0, "thresholds": "rank"},
    "eval_ic15_curve_batch": {"det_match": "rank", "gt_match": 0, "thresholds": "rank"},
    "eval_ap": {"pool_score": "rank"}, "link_map_accumulate": {"acc": 0}, "component_scores": {"labels": "rank", "comp_score": 0},
    "link_boxes": {"hull_n": "rank"}, "link_cc_grid": {"pixel_score": "rank"},
    "component_scores_grid": {"labels": "rank", "pixel_score": 1, "comp_score": 0},
    "tensor_stats": {"x": None, "table": None, "records": None, "ws": None}, "summary_image_u8": {"x": "rank", "ws": None},
}


def operands(args):
    """operand name -> tensor, tuples taken apart"""
    out = {}
    for name, v in args.items():
        if isinstance(v, torch.Tensor):
            out[name] = v
        elif isinstance(v, tuple) and name in TUPLES:
            out.update(zip(TUPLES[name], v))
    return out


def replaced(args, operand, value):
    """`args` with one operand replaced"""
    new = dict(args)
    for name, members in TUPLES.items():
        if operand in members and name in args:
            new[name] = tuple(value if m == operand else t for m, t in zip(members, args[name]))
            return new
    new[operand] = value
    return new


class Arena:
    def __init__(self):
        self.buf = torch.zeros(WS_BYTES, dtype=U8)

    def get(self, nbytes):
        assert nbytes <= self.buf.numel()
        return self.buf


@contextlib.contextmanager
def stubbed():
    """the library replaced by recorders -> the list the calls land in"""
    from tensorflow_ocr_amd import _lib
    log = []

    def recorder(answer):
        def call(name, *a):
            log.append((name, a))
            return answer
        return call
    saved = _lib.call, _lib.call_size, _lib.call_int, _lib._STREAM
    _lib.call, _lib.call_size, _lib.call_int = recorder(0), recorder(WS_BYTES), recorder(1)
    _lib.set_stream(ctypes.c_void_p(0))
    try:
        yield log
    finally:
        _lib.call, _lib.call_size, _lib.call_int, _lib._STREAM = saved


def invoke(name, args, log):
    """one wrapper call on `args` -> the calls it made"""
    from tensorflow_ocr_amd import ops
    del log[:]
    arena = Arena()
    if "ws" in args and name not in WS_TENSOR:
        args = dict(args, ws=arena)
    getattr(ops, name)(**args)
    names = {t.data_ptr(): k for k, t in operands(args).items()}
    names[arena.buf.data_ptr()] = "ws"
    return [[entry, [_argument(a, names) for a in a_list]] for entry, a_list in log]


def _argument(a, names):
    kind = type(a).__name__
    if isinstance(a, ctypes.c_void_p):
        return [kind, "null" if not a.value else names[a.value]]
    if isinstance(a, ctypes.Array):
        return [kind, list(a)]
    return [kind, a.value]


def record_all():
    with stubbed() as log:
        return {name: invoke(name, args, log) for name, args in operand_sets().items()}


def dumps(table):
    rows = ['  %s: [\n%s]' % (json.dumps(name), ",\n".join("    " + json.dumps(c) for c in calls)) for name, calls in table.items()]
    return "{\n" + ",\n".join(rows) + "\n}\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    table = record_all()
    with open(GOLDEN, "w") as f:
        f.write(dumps(table))
    print("%d wrappers, %d calls -> %s (%d bytes)" % (len(table), sum(len(c) for c in table.values()), GOLDEN, os.path.getsize(GOLDEN)))
