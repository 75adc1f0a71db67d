"""GPU: the post-processing entries against their bit-exact oracles, one row per path, edge and refusal, through the C ABI.

  ocr_lanms / ocr_lanms_workspace        oracle/lanms.py (oracle/lanms_oracle.c)
  ocr_quad_fuse / ocr_quad_fuse_workspace tests/ms_ref.py (fuse_ref), only what shares quad_nms.h with ocr_lanms
  ocr_quad_iou                           two oracle.cvgeom.fill_poly masks, |a & b| and |a | b|
  ocr_resize_linear_u8 / _cubic_f32      oracle.cvgeom.resize_linear_u8 / resize_cubic_f32

Every reference is bit-exact, so no row has a tolerance.  Every output and every workspace is a Guard; the workspace Guard
has exactly the queried size.  ROWS is the inventory (name -> Row): tests/test_nms_matrix_inventory.py lists it and checks,
with the oracle alone, that each row's inputs have the pattern the row is named after.

What the ocr_lanms rows are built to reach (csrc/lanms.hip):
  path/<max_k>       2019 | 2020: the staged merge (quads in LDS) gives way to the unstaged one; 4096 | 4097: the sweep
                     that prefetches 64 rows (one mask word per lane) gives way to the generic one.  Image 0 has max_k
                     far-apart quads (all kept: at 4096 the sweep's kept list is full), image 1 is clustered, and at 4097
                     image 2 has its lowest-ranked quad (sorted position 4096, mask word 64) suppressed by the top one.
  verdict/<set>      iou(g[i+1], g[i]) > thr exactly for i in the set: where the run-skipping walk of the staged chain finds
                     its hits (lane 0 / 63 of a 64-verdict look, k-2, none at all, every one, every other one)
  runs               runs of exactly 63, 64, 65 and 128 non-merging neighbours behind a merge
  rejoin             groups a, b, c, d: b merges into a; c overlaps the INPUT b but not the merged quad, so it starts a fresh
                     run right behind a merged quad, and d merges into it
  rank/<m>           two score values only; both positions 2047 and 2048 hold 0.5 (image 0) or 0.75 (image 1): a tie across
                     the 2048-score block of the counting sort
  interleaved/<k>    quad t in cluster t % c: no neighbours merge (m = k) and all but c quads are suppressed; k = 64j, 64j+1
  pos63/<m>          a cluster's best quad at sorted position 63 (bit 63), its victims at 64 (bit 0 of the next word) and m-1
  clamp              counts above max_k are clamped: the first max_k rows are processed
"""
import ctypes

import numpy as np
import pytest
import torch

import ms_ref
from matrix_support import (FL, INVALID_ARG, OK, SZ, UNSUPPORTED, WORKSPACE, Guard, _lib, _rc, _rng)
from oracle import cvgeom as C
from oracle import lanms as OL

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
SHAPE_REFUSAL = UNSUPPORTED             # what OCR_CHECK_SHAPE of csrc/common.h returns (OCR_ERR_UNSUPPORTED)


class Row:
    def __init__(self, name, entries, build, **meta):
        self.name, self.entries, self.build = name, tuple(entries), build
        self.__dict__.update(meta)


class Img:
    """one image's quads f32 [k,9] and what the inventory test checks about them"""

    def __init__(self, q, kind="plain", **meta):
        self.q, self.kind = np.ascontiguousarray(q, f32).reshape(-1, 9), kind
        self.__dict__.update(meta)


ROWS = {}


def _row(name, entries, build, **meta):
    assert name not in ROWS
    ROWS[name] = Row(name, entries, build, **meta)


# ------------------------------------------------------------------------------------------------ quads
def sq(x, y, score, s=10.0):
    return [x, y, x + s, y, x + s, y + s, x, y + s, score]


def _scores(rng, k):
    """k distinct f32 scores in (0, 1]"""
    s = (0.05 + 0.9 * rng.permutation(k) / max(k, 1) + 0.04 * rng.uniform(size=k) / max(k, 1)).astype(f32)
    assert len(np.unique(s)) == k and (s > 0).all() and (s <= 1).all()
    return s


def site(t):
    """far-apart sites: 10-px squares on a 100-px grid, 64 per row"""
    return 100.0 * (t % 64), 100.0 * (t // 64)


def far(k, scores):
    return Img([sq(*site(t), scores[t]) for t in range(k)], "far")


def empty():
    return Img(np.zeros((0, 9), f32))


def single(rng):
    return Img([sq(30.0, 40.0, f32(rng.uniform(0.1, 1.0)))], "far")


def clustered(rng, k):
    """rotated text-like quads around a few centres, roughly row-major: merges and suppressions of every kind"""
    centres = rng.uniform(40, 900, size=(max(k // 12, 1), 2))
    out = []
    for _ in range(k):
        cx, cy = centres[rng.integers(len(centres))] + rng.normal(0, 1.5, 2)
        q = ms_ref.rot_rect(cx, cy, rng.uniform(40, 90), rng.uniform(12, 24), rng.uniform(-0.3, 0.3))
        if rng.uniform() < 0.3:
            q = q.reshape(4, 2)[::-1].reshape(8)
        out.append(np.concatenate([q, [rng.uniform(0.5, 1.0)]]))
    a = np.array(out, f32)
    return Img(a[np.lexsort((a[:, 0], a[:, 1].round(-1)))])


def verdicts(k, hits, rng):
    """k squares in a line: g[i+1] is g[i] moved by 1 px (iou 90/110) for i in hits, by 100 px (iou 0) otherwise"""
    hits = {i for i in hits if 0 <= i <= k - 2}
    s, x, rows = _scores(rng, k), 0.0, []
    for i in range(k):
        rows.append(sq(x, 0.0, s[i]))
        x += 1.0 if i in hits else 100.0
    return Img(rows, "verdict", hits=hits)


def rejoin(k, rng):
    """groups of four, 100 px apart: a (score 0.9) at 0, b (0.1) at 6, c at 12, d at 13.  iou(b, a) = iou(c, b) = 0.25 and
    iou(d, c) = 90/110, so all three input verdicts are 1; a + b merge to x ~ 0.6, which c (from 12) does not touch"""
    s, rows = _scores(rng, k), []
    for i in range(k):
        x0, j = 100.0 * (i // 4), i % 4
        rows.append(sq(x0 + (0.0, 6.0, 12.0, 13.0)[j], 0.0, (f32(0.9), f32(0.1), s[i], s[i])[j]))
    return Img(rows, "rejoin", n_merged=2 * (k // 4) + (0, 1, 1, 2)[k % 4])


def interleaved(k, c, rng):
    """quad t in cluster t % c, clusters 100 px apart, every quad jittered by at most 1 px each way"""
    s = _scores(rng, k)
    j = rng.uniform(-1.0, 1.0, size=(k, 2))
    return Img([sq(100.0 * (t % c) + j[t, 0], j[t, 1], s[t]) for t in range(k)], "interleaved", c=c)


def ranked(m, specials, rng):
    """m quads given by SORTED position: score 1 - p / (m + 1); `specials` {sorted position: (x, y)} are placed by hand and
    kept away from each other in the input order, every other position is a far-apart single"""
    score = (1.0 - np.arange(m) / (m + 1.0)).astype(f32)
    assert len(np.unique(score)) == m
    order = [p for p in rng.permutation(m) if p not in specials]
    for at, p in zip((5, 20, len(order) - 1), sorted(specials)):
        order.insert(at, p)
    assert sorted(order) == list(range(m))
    rows = [sq(*(specials[p] if p in specials else site(p)), score[p]) for p in order]
    return rows, order


def pos63(m, rng):
    lx, ly = site(m + 3)
    sp = {63: (lx, ly), m - 1: (lx, ly + 1.0), 64: (lx + 1.0, ly)}
    rows, order = ranked(m, sp, rng)
    return Img(rows, "pos63", leader=order.index(63), victims=sorted({order.index(64), order.index(m - 1)}))


def last_suppressed(m, rng):
    """the quad at sorted position m-1 lies on the one at position 0"""
    lx, ly = site(m + 3)
    rows, order = ranked(m, {0: (lx, ly), m - 1: (lx + 1.0, ly)}, rng)
    return Img(rows, "last", leader=order.index(0), victims=[order.index(m - 1)])


def two_scores(m, forced, rng):
    s = rng.choice(np.array([0.5, 0.75], f32), size=m)
    for p in (2047, 2048):
        if p < m:
            s[p] = forced
    return Img([sq(*site(t), s[t]) for t in range(m)], "far", forced=forced)


# ------------------------------------------------------------------------------------------------ ocr_lanms rows
LANMS = ("ocr_lanms", "ocr_lanms_workspace")
PATH_MAX_K = (2019, 2020, 4096, 4097)
VERDICT_SETS = {"edges": lambda k: {0, 62, 63, 64, 127, 128, k - 2}, "63": lambda k: {63}, "64": lambda k: {64},
                "k-2": lambda k: {k - 2}, "none": lambda k: set(), "all": lambda k: set(range(k - 1)),
                "alternating": lambda k: set(range(0, k - 1, 2))}
VERDICT_K = (66, 130, 200)
THRS = (0.2, 1e-4)
RUN_HITS = (63, 129, 196, 326)          # runs of 63, 64, 65, 128 flags without a hit: each hit restarts the walk 2 further on
RANK_M = (2047, 2048, 2049, 2100)
INTERLEAVED = {64: 3, 65: 2, 128: 5, 129: 64, 4096: 7}
POS63_M = (65, 200)


def _lanms(images, thr, max_k=None, counts=None):
    max_k = max_k or max(len(im.q) for im in images)
    return dict(images=images, thr=thr, max_k=max_k, counts=counts or [len(im.q) for im in images])


def _path(max_k):
    rng = _rng("nms", "path", max_k)
    images = [far(max_k, _scores(rng, max_k)), clustered(rng, max_k // 3)]
    images.append(last_suppressed(max_k, rng) if max_k == 4097 else (empty() if max_k % 2 else single(rng)))
    return _lanms(images, 0.2, max_k)


def _pattern(name, thr, part, make):
    """two calls per pattern: k = 66, none, 200 and one, 130 — ragged counts, the last image as long as max_k"""
    rng = _rng("nms", name, thr, part)
    images = [make(66, rng), empty(), make(200, rng)] if part == 0 else [single(rng), make(130, rng)]
    return _lanms(images, thr)


for _k in PATH_MAX_K:
    _row("lanms/path/%d" % _k, LANMS, lambda k=_k: _path(k))
for _thr in THRS:
    for _part in (0, 1):
        for _name, _fn in VERDICT_SETS.items():
            _row("lanms/verdict/%s/thr%g/%d" % (_name, _thr, _part), LANMS,
                 lambda n=_name, f=_fn, t=_thr, p=_part: _pattern("verdict-" + n, t, p, lambda k, rng: verdicts(k, f(k), rng)))
        _row("lanms/rejoin/thr%g/%d" % (_thr, _part), LANMS, lambda t=_thr, p=_part: _pattern("rejoin", t, p, rejoin))
    _row("lanms/runs/thr%g" % _thr, LANMS,
         lambda t=_thr: _lanms([single(_rng("nms", "runs", 1)), verdicts(330, RUN_HITS, _rng("nms", "runs", t))], t))
for _m in RANK_M:
    _row("lanms/rank/%d" % _m, LANMS,
         lambda m=_m: _lanms([two_scores(m, f32(0.5), _rng("nms", "rank", m, 0)), two_scores(m, f32(0.75), _rng("nms", "rank", m, 1)),
                              empty() if m % 2 else single(_rng("nms", "rank", m, 2))], 0.2, m))
for _k, _c in INTERLEAVED.items():
    for _thr in (THRS if _k <= 129 else THRS[:1]):
        _row("lanms/interleaved/%d/thr%g" % (_k, _thr), LANMS,
             lambda k=_k, c=_c, t=_thr: _lanms([interleaved(k, c, _rng("nms", "inter", k, 0)), single(_rng("nms", "inter", k, 1)),
                                                interleaved(k - 1, c, _rng("nms", "inter", k, 2))], t, k))
for _m in POS63_M:
    _row("lanms/pos63/%d" % _m, LANMS,
         lambda m=_m: _lanms([pos63(m, _rng("nms", "pos63", m)), empty(), pos63(m, _rng("nms", "pos63", m, 1))], 0.2, m))
# counts above max_k: the buffers still hold max_k rows, the first max_k are processed (staged at 130, unstaged at 2100)
_row("lanms/clamp/130", LANMS, lambda: _lanms([verdicts(130, VERDICT_SETS["edges"](130), _rng("nms", "clamp", 0)),
                                                interleaved(130, 5, _rng("nms", "clamp", 1)), single(_rng("nms", "clamp", 2))],
                                               0.2, 130, [137, 260, 1]))
_row("lanms/clamp/2100", LANMS, lambda: _lanms([interleaved(2100, 9, _rng("nms", "clamp", 3)), clustered(_rng("nms", "clamp", 4), 2100)],
                                                0.2, 2100, [2107, 4200]))

_ORACLE = {}


def lanms_oracle(name):
    """the row and [(merged, keep)] of its images, computed once"""
    if name not in _ORACLE:
        row = ROWS[name].build()
        _ORACLE[name] = (row, [OL.lanms(im.q[:row["max_k"]], row["thr"]) for im in row["images"]])
    return _ORACLE[name]


PAD = sq(5.0, 5.0, 1.0, 5000.0)         # rows beyond a count: a quad that would merge with anything, never read


def _ws_bytes(L, name, n, m):
    return int(L._fn(name, SZ)(ctypes.c_int(n), ctypes.c_int(m)))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class LanmsCall:
    def __init__(self, L, device, n, max_k, ws=None):
        self.L, self.n, self.max_k = L, n, max_k
        self.bytes = _ws_bytes(L, "ocr_lanms_workspace", n, max_k)
        self.merged, self.n_merged = Guard((n, max_k, 9), torch.float32, device), Guard((n,), torch.int32, device)
        self.keep, self.n_keep = Guard((n, max_k), torch.int32, device), Guard((n,), torch.int32, device)
        self.ws = Guard((self.bytes if ws is None else ws,), torch.uint8, device)
        self.guards = (self.merged, self.n_merged, self.keep, self.n_keep, self.ws)

    def run(self, boxes_t, counts_t, thr, **over):
        a = dict(boxes=boxes_t, counts=counts_t, n=self.n, max_k=self.max_k, merged=self.merged, n_merged=self.n_merged, keep=self.keep,
                 n_keep=self.n_keep, ws=self.ws, ws_bytes=self.ws.nbytes)
        a.update(over)
        return _rc(self.L, "ocr_lanms", a["boxes"], a["counts"], a["n"], a["max_k"], FL(thr), a["merged"], a["n_merged"], a["keep"],
                   a["n_keep"], a["ws"], SZ(a["ws_bytes"]))


def _pack(images, max_k, width=9):
    boxes = np.tile(np.array(PAD, f32), (len(images), max_k, 1))
    for b, im in enumerate(images):
        boxes[b, :len(im.q)] = im.q
    return boxes


LANMS_ROWS = [n for n in ROWS if n.startswith("lanms/")]


@pytest.mark.parametrize("name", LANMS_ROWS)
def test_lanms(device, name):
    L, _ = _lib()
    row, want = lanms_oracle(name)
    n, max_k = len(row["images"]), row["max_k"]
    boxes = _pack(row["images"], max_k)
    assert np.isfinite(boxes).all() and (boxes[:, :, 8] > 0).all() and (boxes[:, :, 8] <= 1).all()
    call = LanmsCall(L, device, n, max_k)
    assert call.run(_dev(boxes, device), _dev(np.array(row["counts"], i32), device), row["thr"]) == OK
    torch.cuda.synchronize()
    assert all(g.ok() for g in call.guards), "written outside a buffer"
    merged, keep = call.merged.raw().view(i32), call.keep.raw()
    n_merged, n_keep = call.n_merged.raw(), call.n_keep.raw()
    for b, (om, ok) in enumerate(want):
        assert n_merged[b] == len(om) and n_keep[b] == len(ok), (b, int(n_merged[b]), len(om), int(n_keep[b]), len(ok))
        assert np.array_equal(merged[b, :len(om)], om.view(i32)), b
        assert np.array_equal(keep[b, :len(ok)], ok), b
        assert (merged[b, len(om):] == -1).all() and (keep[b, len(ok):] == -1).all(), "rows beyond the counts were written"


def test_lanms_status(device):
    """every refusal leaves the outputs and the workspace as they were"""
    L, _ = _lib()
    n, max_k = 2, 130
    rng = _rng("nms", "status")
    boxes = _dev(_pack([verdicts(130, {3, 64}, rng), single(rng)], max_k), device)
    counts = _dev(np.array([130, 1], i32), device)
    call = LanmsCall(L, device, n, max_k)
    cases = [("ws_bytes - 1", dict(ws_bytes=call.bytes - 1), WORKSPACE), ("ws_bytes 0", dict(ws_bytes=0), WORKSPACE),
             ("max_k 32769", dict(max_k=32769, ws_bytes=1 << 62), SHAPE_REFUSAL), ("n_images 0", dict(n=0), INVALID_ARG),
             ("n_images -1", dict(n=-1), INVALID_ARG), ("max_k 0", dict(max_k=0), INVALID_ARG)]
    cases += [("%s null" % k, {k: None}, INVALID_ARG) for k in ("boxes", "counts", "merged", "n_merged", "keep", "n_keep", "ws")]
    for what, over, status in cases:
        assert call.run(boxes, counts, 0.2, **over) == status, what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in call.guards), what
    assert _ws_bytes(L, "ocr_lanms_workspace", n, max_k) == n * max_k * 4 + n * max_k * 3 * 8 + n * max_k + 512
    assert call.run(boxes, counts, 0.2) == OK               # the same buffers do take the call
    torch.cuda.synchronize()
    assert all(g.ok() for g in call.guards) and call.n_merged.raw().tolist() == [128, 1]


# ------------------------------------------------------------------------------------------------ ocr_quad_fuse rows
FUSE = ("ocr_quad_fuse", "ocr_quad_fuse_workspace")


def _fuse_images(max_pool):
    rng = _rng("nms", "fuse", max_pool)
    if max_pool == 64:
        return [interleaved(64, 3, rng), single(rng), empty()]
    if max_pool == 65:
        return [interleaved(65, 2, rng), pos63(65, rng), empty()]
    return [interleaved(4096, 7, rng), pos63(200, rng), single(rng)]


for _p in (64, 65, 4096):
    for _mode in (0, 1):
        _row("fuse/%d/mode%d" % (_p, _mode), FUSE, lambda p=_p, m=_mode: dict(images=_fuse_images(p), max_pool=p, mode=m, thr=0.2))


def fuse_oracle(name):
    if name not in _ORACLE:
        row = ROWS[name].build()
        _ORACLE[name] = (row, [ms_ref.fuse_ref(im.q, row["thr"], row["mode"]) for im in row["images"]])
    return _ORACLE[name]


class FuseCall:
    def __init__(self, L, device, n, max_pool, ws=None):
        self.L, self.n, self.max_pool = L, n, max_pool
        self.bytes = _ws_bytes(L, "ocr_quad_fuse_workspace", n, max_pool)
        self.fused, self.keep = Guard((n, max_pool, 9), torch.float32, device), Guard((n, max_pool), torch.int32, device)
        self.n_keep, self.owner = Guard((n,), torch.int32, device), Guard((n, max_pool), torch.int32, device)
        self.ws = Guard((self.bytes if ws is None else ws,), torch.uint8, device)
        self.guards = (self.fused, self.keep, self.n_keep, self.owner, self.ws)

    def run(self, pool, count, thr, mode):
        return _rc(self.L, "ocr_quad_fuse", pool, count, self.n, self.max_pool, FL(thr), mode, self.fused, self.keep, self.n_keep,
                   self.owner, self.ws, SZ(self.ws.nbytes))


@pytest.mark.parametrize("name", [n for n in ROWS if n.startswith("fuse/")])
def test_quad_fuse(device, name):
    L, _ = _lib()
    row, want = fuse_oracle(name)
    n, max_pool = len(row["images"]), row["max_pool"]
    pool = _pack(row["images"], max_pool)
    assert np.isfinite(pool).all()
    call = FuseCall(L, device, n, max_pool)
    assert call.bytes > 0
    count = _dev(np.array([len(im.q) for im in row["images"]], i32), device)
    assert call.run(_dev(pool, device), count, row["thr"], row["mode"]) == OK
    torch.cuda.synchronize()
    assert all(g.ok() for g in call.guards), "written outside a buffer"
    fused, keep, n_keep, owner = call.fused.raw().view(i32), call.keep.raw(), call.n_keep.raw(), call.owner.raw()
    for b, (w_fused, w_keep, w_owner) in enumerate(want):
        P = len(w_owner)
        assert n_keep[b] == len(w_keep) and np.array_equal(keep[b, :len(w_keep)], w_keep), b
        assert np.array_equal(owner[b, :P], w_owner) and (owner[b, P:] == -1).all(), b
        assert np.array_equal(fused[b, :P], w_fused.view(i32)), b
        assert (fused[b, P:] == -1).all() and (keep[b, len(w_keep):] == -1).all(), "rows beyond the counts were written"


def test_quad_fuse_refuses_4097(device):
    L, _ = _lib()
    assert _ws_bytes(L, "ocr_quad_fuse_workspace", 1, 4097) == 0
    call = FuseCall(L, device, 1, 4097, ws=_ws_bytes(L, "ocr_quad_fuse_workspace", 1, 4096))
    pool = _dev(_pack([interleaved(65, 2, _rng("nms", "fuse", "refused"))], 4097), device)
    for mode in (0, 1):
        assert call.run(pool, _dev(np.array([65], i32), device), 0.2, mode) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(g.untouched() for g in call.guards)


# ------------------------------------------------------------------------------------------------ ocr_quad_iou rows
IOU_VERTS, IOU_MASKS, IOU_GRIDS = (3, 4, 5, 8), ((40, 56), (300, 520)), ((1, 1), (1, 7), (5, 1), (6, 4))


def draw_polys(rng, count, V, h, w):
    """test_poly_cover_random_polygons_vs_fillpoly's polygons: integer vertices in [-12, max(h, w) + 12), so concave and
    self-intersecting ones; every fourth one inside the mask, with two identical vertices, or all on one row"""
    p = rng.integers(-12, max(h, w) + 12, size=(count, V, 2)).astype(i32)
    p[1::4] = np.clip(p[1::4], 0, min(h, w) - 1)
    p[2::4, 1] = p[2::4, 0]
    p[3::4, :, 1] = 9
    return p


def fixed_pairs(V, h, w):
    """(det, gt) pairs, vertex lists repeated up to V vertices"""
    def poly(pts):
        pts = list(pts)
        return np.array([pts[min(i, len(pts) - 1)] for i in range(V)], i32)
    tri = lambda x, y, s: poly([(x, y), (x + s, y), (x, y + s)])
    pairs = {"left of the mask": (tri(-40, 5, 20), tri(-35, 8, 25)), "above the mask": (tri(5, -40, 20), tri(8, -35, 25)),
             "whole mask": (poly([(0, 0), (w - 1, 0), (0, h - 1)]), poly([(w - 1, h - 1), (0, h - 1), (w - 1, 0)])),
             "3x3 box": (tri(17, 11, 2), poly([(19, 13), (17, 13), (19, 11)])),
             "identical": (poly([(3, 4), (30, 9), (12, 33), (25, 2)]), poly([(3, 4), (30, 9), (12, 33), (25, 2)]))}
    return pairs


def _iou_row(V, h, w):
    rng = _rng("nms", "iou", V, h, w)
    grids = [(draw_polys(rng, nd, V, h, w), draw_polys(rng, ng, V, h, w)[::-1].copy()) for nd, ng in IOU_GRIDS]
    fixed = fixed_pairs(V, h, w)
    grids.append((np.stack([d for d, _ in fixed.values()]), np.stack([g for _, g in fixed.values()])))
    return dict(V=V, h=h, w=w, grids=grids, fixed=list(fixed))


for _V in IOU_VERTS:
    for _h, _w in IOU_MASKS:
        _row("iou/v%d/%dx%d" % (_V, _h, _w), ("ocr_quad_iou",), lambda V=_V, h=_h, w=_w: _iou_row(V, h, w))


def iou_ref(dets, gts, h, w):
    a = [C.fill_poly(np.zeros((h, w), np.uint8), p, 1).astype(bool) for p in dets]
    b = [C.fill_poly(np.zeros((h, w), np.uint8), p, 1).astype(bool) for p in gts]
    inter = np.array([[(x & y).sum() for y in b] for x in a], i32)
    uni = np.array([[(x | y).sum() for y in b] for x in a], i32)
    return inter, uni


@pytest.mark.parametrize("name", [n for n in ROWS if n.startswith("iou/")])
def test_quad_iou(device, name):
    L, _ = _lib()
    row = ROWS[name].build()
    V, h, w = row["V"], row["h"], row["w"]
    for j, (dets, gts) in enumerate(row["grids"]):
        nd, ng = len(dets), len(gts)
        inter, uni = Guard((nd, ng), torch.int32, device), Guard((nd, ng), torch.int32, device)
        assert _rc(L, "ocr_quad_iou", _dev(dets, device), nd, _dev(gts, device), ng, V, h, w, inter, uni) == OK
        torch.cuda.synchronize()
        w_inter, w_uni = iou_ref(dets, gts, h, w)
        assert np.array_equal(inter.raw(), w_inter), (j, nd, ng)
        assert np.array_equal(uni.raw(), w_uni), (j, nd, ng)
    fixed = dict(zip(row["fixed"], zip(np.diag(w_inter), np.diag(w_uni))))      # the last grid: pair i is (det i, gt i)
    assert fixed["left of the mask"] == (0, 0) and fixed["above the mask"] == (0, 0)
    assert fixed["identical"][0] == fixed["identical"][1] > 0
    assert 0 < fixed["3x3 box"][0] <= fixed["3x3 box"][1] <= 9
    assert fixed["whole mask"][1] == h * w


def test_quad_iou_status(device):
    L, _ = _lib()
    pts = _dev(np.zeros((4, 9, 2), i32), device)
    inter, uni = Guard((4, 4), torch.int32, device), Guard((4, 4), torch.int32, device)
    for what, (nd, ng, V, h, w) in {"verts 2": (4, 4, 2, 40, 56), "verts 9": (4, 4, 9, 40, 56), "nd 65536": (65536, 4, 4, 40, 56),
                                    "mask_w 32769": (4, 4, 4, 40, 32769), "mask_h 32769": (4, 4, 4, 32769, 56)}.items():
        assert _rc(L, "ocr_quad_iou", pts, nd, pts, ng, V, h, w, inter, uni) == SHAPE_REFUSAL, what
    for what, a in {"dets null": (None, 4, pts, 4, 4, 40, 56, inter, uni), "inter null": (pts, 4, pts, 4, 4, 40, 56, None, uni),
                    "ng 0": (pts, 4, pts, 0, 4, 40, 56, inter, uni), "mask_h 0": (pts, 4, pts, 4, 4, 0, 56, inter, uni)}.items():
        assert _rc(L, "ocr_quad_iou", *a) == INVALID_ARG, what
    torch.cuda.synchronize()
    assert inter.untouched() and uni.untouched()


# ------------------------------------------------------------------------------------------------ resize rows
LINEAR_CN = (1, 3, 4)
LINEAR_SHAPES = {"identity": (37, 53, 37, 53), "halving": (36, 52, 18, 26), "up": (37, 53, 64, 64), "one-row": (50, 70, 1, 70),
                 "one-column": (50, 70, 50, 1), "from-one-row": (1, 9, 5, 20), "from-one-column": (9, 1, 20, 5), "3x3": (3, 3, 97, 131)}
CUBIC_PLANES = (1, 3)
CUBIC_SHAPES = ((4, 5, 13, 17), (32, 32, 128, 128), (45, 80, 5, 9), (1, 1, 3, 3), (7, 9, 7, 9))
CUBIC_SCALES = ((1.0, 1.0), (255.0, 1.0), (1.0, 255.0))

for _name, _s in LINEAR_SHAPES.items():
    _row("resize/linear/%s" % _name, ("ocr_resize_linear_u8",), lambda s=_s: dict(shape=s))
for _s in CUBIC_SHAPES:
    _row("resize/cubic/%dx%d-%dx%d" % _s, ("ocr_resize_cubic_f32",), lambda s=_s: dict(shape=s))


@pytest.mark.parametrize("name", list(LINEAR_SHAPES))
def test_resize_linear(device, name):
    L, _ = _lib()
    H, W, dh, dw = ROWS["resize/linear/%s" % name].build()["shape"]
    for cn in LINEAR_CN:
        src = _rng("nms", "linear", name, cn).integers(0, 256, size=(H, W, cn)).astype(np.uint8)
        dst = Guard((dh, dw, cn), torch.float32, device)
        assert _rc(L, "ocr_resize_linear_u8", _dev(src, device), H, W, cn, dst, dh, dw) == OK, cn
        torch.cuda.synchronize()
        want = C.resize_linear_u8(src, dh, dw)
        assert np.array_equal(dst.np().view(i32), want.astype(f32).view(i32)), cn
        if name == "identity":
            assert np.array_equal(want, src)
        if name == "halving":
            a = src.astype(i32)
            assert np.array_equal(want, (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2)


@pytest.mark.parametrize("shape", CUBIC_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_cubic(device, shape):
    L, _ = _lib()
    h, w, dh, dw = shape
    for planes in CUBIC_PLANES:
        src = _rng("nms", "cubic", shape, planes).uniform(0, 1, size=(planes, h, w)).astype(f32)
        src[planes - 1] = (src[planes - 1] > 0.5).astype(f32)       # a saturated map: the cubic over- and undershoots
        for pre, post in CUBIC_SCALES:
            dst = Guard((planes, dh, dw), torch.float32, device)
            assert _rc(L, "ocr_resize_cubic_f32", _dev(src, device), planes, h, w, dst, dh, dw, FL(pre), FL(post)) == OK
            torch.cuda.synchronize()
            got = dst.np().view(i32)
            for k in range(planes):
                want = C.resize_cubic_f32(src[k] * f32(pre), dh, dw) * f32(post)
                assert np.array_equal(got[k], want.view(i32)), (planes, k, pre, post)


def test_resize_status(device):
    L, _ = _lib()
    src8, src32 = _dev(np.zeros((4, 4, 3), np.uint8), device), _dev(np.zeros((3, 4, 4), f32), device)
    dst = Guard((3, 4, 4), torch.float32, device)
    for a in ((None, 4, 4, 3, dst, 4, 4), (src8, 4, 4, 3, None, 4, 4), (src8, 0, 4, 3, dst, 4, 4), (src8, 4, 4, 0, dst, 4, 4),
              (src8, 4, 4, 3, dst, 4, 0)):
        assert _rc(L, "ocr_resize_linear_u8", *a) == INVALID_ARG
    for a in ((None, 3, 4, 4, dst, 4, 4), (src32, 3, 4, 4, None, 4, 4), (src32, 0, 4, 4, dst, 4, 4), (src32, 3, 4, 4, dst, 0, 4)):
        assert _rc(L, "ocr_resize_cubic_f32", *a, FL(1.0), FL(1.0)) == INVALID_ARG
    torch.cuda.synchronize()
    assert dst.untouched()
