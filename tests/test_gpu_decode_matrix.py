"""GPU: every entry of csrc/decode.hip and csrc/boxes.hip — the pair softmaxes, the threshold masks, link-gated and
mask connected components, the directed grouping, contour parents and the hull / calipers of components and hole
borders — called through ctypes on the library tensorflow_ocr_amd.ops binds (no Python wrapper sizes a workspace,
picks max_comps or hides a status).  Every output sits in a 0xFF-filled buffer between guard bands, the workspace is
exactly the `_workspace()` answer in bytes between bands, and every status is asserted.  Integer outputs (labels,
ncomp, comps, hull_n, hull_head, parents, masks, first / second) are compared exactly, calipers bit for bit against
oracle/cvgeom.py, the softmaxes against float64 under the bound below.  Table rows at or beyond the documented count
must still hold the fill.
The reference for connected components is `flood` below: a breadth-first fill over an explicit undirected edge list, no
union-find.  tests/test_decode_matrix_inventory.py holds it equal to O.link_cc_union on every link row, on the host,
and asserts what each generator promises (tile-border crossings, the root tile's share, sizes around min_size).
The kernels here read f32 and integers only and the bf16 library compiles the same code, so this file is not run a
second time on the bf16 library (tests/test_gpu_bf16.py).  LANMS, iou.hip, resize.hip, eval_*.hip and link_boxes.hip
are not covered here: they are held bit for bit to oracle/lanms_oracle.c and oracle/cvgeom_oracle.c in
test_gpu_lanms.py, test_gpu_labels.py (IoU and resize), test_gpu_eval*.py and test_gpu_link_boxes.py.

Kernels and the rows that reach them
  cc_init_kernel, cc_root_kernel, cc_relabel_kernel   every test_link_cc row
  cc_union_tile_kernel<0,false>, <0,true>   test_link_cc: LINK_ROWS, each under both link layouts ([8][n][h][w] and
                            channel 1 of [8][n][h][w][2] with channel 0 holding the inverted links): random maps at
                            (3,3) (3,70) (70,3) (32,32) (33,31) (33,65) (64,96) (67,70); serpentine (one snake over
                            every second row of 67x70, one random direction per edge, > 60 tile-border crossings);
                            late_root (comb, smallest index in a tile with < 5 % of the pixels); corner_* (two blobs
                            joined only by one directed diagonal link across the corner of four tiles, each diagonal,
                            each direction, and the unjoined control); border_* (a border / corner pixel with all its
                            own links high is a singleton, joined once an interior neighbour links to it; 3x3: one
                            active pixel); thresholds (score and link at t, nextafter(t, +-1), NaN); min_size
                            (components of min_size and min_size + 1 pixels, min_size 0 and -1)
  cc_count_kernel, cc_assign_kernel   test_link_cc numbering rows: 70x70 all positive without links (4900 singletons,
                            five 1024-pixel blocks, the last ragged) at max_comps 4900 | 1025 | 16; fully_linked 70x70
                            (one component, every union contends); test_link_cc_batch (n = 3: dense, all-negative,
                            serpentine; each image bit-identical to its n = 1 run)
  cc_init_mask_kernel, cc_union_tile_kernel<1,*>, <2,*>   test_mask_cc: MASK_ROWS x connectivity 4 | 8 x value 0 | 1:
                            checkerboard 33x65, diagonal and anti-diagonal staircases through a tile corner (the
                            down-left step x = 32 -> 31 included), three nested rings, all-zero, all-one, bytes 2 and
                            255, n = 2 with different masks
  contour_parents_kernel    test_contours: rings three deep, a notch open to the image edge (background, hull_n 0), a
                            one-pixel hole (border = its four 4-neighbours only), a 2x2 hole, a component in column 0
                            (parent 0); the list rebuilt from the device's outputs equals oracle.contours
                            suzuki_contours and contour_order (kind, parent position, hull) and contour_boxes
  mar_init_kernel, mar_yext_kernel, mar_scan_kernel, mar_rows_kernel, mar_hull_calipers_kernel
                            test_min_area_rects: one pixel (hull_n 1), two pixels, horizontal / vertical / diagonal /
                            anti-diagonal lines (hull_n 2, zero calipers), axis-aligned and rotated rectangles, an L, an
                            id without pixels (hull_n 0, nothing else written) x scales (1,1) (4,4) (2.5,1.75);
                            test_rects_truncated (max_comps < ncomp on 100x5 and 5x100); test_contours
  mar_edge_kernel, mar_border_kernel<0>, <1>   test_contours, test_rects_truncated (max_regions < nregions)
  pixel_detect_kernel       test_pixel_detect: n = 2, image 1 a trap; equality and NaN on both thresholds
  east_mask_first_kernel, east_second_kernel   test_east_pixel_detect: hw 1 | 255 | 257 | 67*70; per channel: none below,
                            exactly one, two adjacent, first at 0, only one at hw - 1, values at the threshold and NaN
                            around one real pair, many; test_east_complete (the script's host step through
                            ocr_zero_pixels_u8, against oracle.contours.east_pixel_detect)
  zero_pixels_kernel        test_zero_pixels: count 0 | 1 | 16 (the host caller's) | 256 (the block), duplicates
  softmax_pairs_kernel      test_softmax_pairs: m 1 | 255 | 257 | 1 048 833 (4096 blocks of 256 and a second trip)
  link_softmax_stack_kernel test_link_softmax_stack: m 1 | 255 | 257 | 131 105 (8 m just past one pass), every direction
                            with its own logits
  cc_directed_kernel        test_directed: raw-ABI workspace guard, n = 2 against O.link_cc_reference_dfs and against the
                            n = 1 runs (labels are pinned bit for bit on more maps in test_gpu_decode_directed.py)
  ocr_py27_dict_order       a host routine; pinned in tests/test_oracle.py, not called here
  every OCR_CHECK_ARG / OCR_CHECK_SHAPE and every workspace check of the two files: test_status_codes (nothing written)

Softmax bound (u = 2^-24, g(m) = m u / (1 - m u)).  The expression is the one test_gpu_loss_matrix.py bounds
(p = expf(l - max) / (expf(l0 - max) + expf(l1 - max)); there: rel(p) <= 7 u — two expf at 2 u, the subtractions, the sum,
the division).  Written out per element, with d = min - max <= 0: the larger logit's exponent is expf(0) = 1; the smaller
one's argument carries u |d|, so rel(e_lo) <= (|d| + 2) u; rel(s) <= u + p_lo (|d| + 2) u + p_hi 2 u <= 3.37 u since
p_lo |d| <= |d| e^d <= 0.37; the division adds u.  Hence rel(p_hi) <= 6.37 u and rel(p_lo) <= (|d| + 6.37) u, and
    |dev - ref| <= g(7 + |d| [smaller logit]) p + 2^-149.
Logits 200 apart give exactly (1, 0) and are asserted so; a NaN logit makes both outputs of its pair NaN.

Findings
  * No entry bounded its extents.  ocr_link_cc and ocr_mask_cc put n into gridDim.y (n > 65535: a launch error after
    the init kernel had already run); every kernel of decode.hip forms h * w in int; ocr_min_area_rects and
    ocr_hole_border_rects form h * w and 3 * h * w in int for the row table.  All now answer OCR_ERR_UNSUPPORTED before
    any launch (test_status_codes); include/ocr_hip.h says so.
  * ocr_zero_pixels_u8 already refuses count > 256 (its one block); the header now documents it.

MEASURED (largest |err| / bound over the rows on the MI355X)
  softmax_pairs             0.774   (m 1: 0.000, 255: 0.551, 257: 0.574, 1 048 833: 0.774)
  link_softmax_stack        0.762   (m 1: 0.105, 255: 0.735, 257: 0.711, 131 105: 0.762)
  No row was over its bound and no integer row differed.
  Comparison mutations of a scratch copy of decode.hip, one at a time (never committed):
    sz[i] > min_size -> >=      fails test_link_cc[min_size-5-*] (and the random rows from 3x70 up, test_link_cc_batch);
                                min_size-0 and min_size--1 pass, as they must
    interior rule x <= w - 2 -> w - 1   not run: MODE 0 has no bounds check on the neighbour, the mutant would read
                                and unite outside the map
    border pass skips directions with dx != 0 and dy != 0   fails test_link_cc[corner_diag_down | diag_up | anti_down |
                                anti_up-*], the random rows with more than one tile, test_mask_cc[staircase-8-1],
                                [anti_staircase-8-1], [checkerboard-8-*]; the corner_*_none controls pass
    link > tl -> >= (tile kernel)   fails test_link_cc[thresholds-1] and [thresholds-2], nothing else
  Time on the MI355X: the file's 123 tests 3.2 s; slowest test_softmax_pairs[1048833] 0.18 s (the float64 reference).
"""
import ctypes
from collections import deque
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (DB, FL, I64, INVALID_ARG, OK, SZ, UNSUPPORTED, WORKSPACE, Guard, _bits_equal, _g, _lib, _ratio,
                            _rc, _rng, f32, f64)
from oracle import contours as OC
from oracle import cvgeom as C
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "decode")
I32, U8, F32 = torch.int32, torch.uint8, torch.float32
INT_MAX = 2 ** 31 - 1
KDX, KDY = (-1, -1, -1, 1, 1, 1, 0, 0), (0, 1, -1, 0, 1, -1, -1, 1)      # decode.hip kDx / kDy
TP, TL = f32(0.6), f32(0.7)
HI, LO = f32(0.95), f32(0.05)


# ------------------------------------------------------------------------------------------------ the reference
def flood(seg, src, dst, min_size):
    """Breadth-first fill.  seg bool [h, w]; src / dst: pixel indices of the undirected edges (ends outside seg drop the
    edge).  -> (labels int32 [h, w], [(smallest index, size)]): ids in ascending order of the smallest index, given to
    components with more than min_size pixels."""
    h, w = seg.shape
    segf = seg.ravel()
    nb = [[] for _ in range(h * w)]
    for a, b in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if segf[a] and segf[b]:
            nb[a].append(b)
            nb[b].append(a)
    seen = np.zeros(h * w, bool)
    labels = np.zeros(h * w, np.int32)
    comps = []
    for s in range(h * w):                      # ascending: s is the smallest index of the component it opens
        if not segf[s] or seen[s]:
            continue
        seen[s] = True
        members, queue = [s], deque([s])
        while queue:
            for q in nb[queue.popleft()]:
                if not seen[q]:
                    seen[q] = True
                    members.append(q)
                    queue.append(q)
        if len(members) > min_size:
            comps.append((s, len(members)))
            labels[members] = len(comps)
    return labels.reshape(h, w), comps


def link_edges(score, link, tp, tl):
    """(seg, src, dst) of one map: nodes score > tp in f32; p -- p + d iff p is interior and link[d][p] > tl"""
    h, w = score.shape
    with np.errstate(invalid="ignore"):
        seg = np.asarray(score, f32) > f32(tp)
        on = np.asarray(link, f32) > f32(tl)
    idx = np.arange(h * w).reshape(h, w)
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    src, dst = [], []
    for d in range(8):
        e = inner & seg & on[d]
        src.append(idx[e])
        dst.append(idx[e] + KDY[d] * w + KDX[d])
    return seg, np.concatenate(src), np.concatenate(dst)


def link_ref(score, link, tp, tl, min_size):
    return flood(*link_edges(score, link, tp, tl), min_size)


def mask_ref(mask, value, conn):
    seg = (np.asarray(mask) != 0) == (value != 0)
    h, w = seg.shape
    idx = np.arange(h * w).reshape(h, w)
    src, dst = [idx[:, :-1].ravel(), idx[:-1].ravel()], [idx[:, 1:].ravel(), idx[1:].ravel()]
    if conn == 8:
        src += [idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel()]
        dst += [idx[1:, 1:].ravel(), idx[1:, :-1].ravel()]
    return flood(seg, np.concatenate(src), np.concatenate(dst), 0)


# ------------------------------------------------------------------------------------------------ link rows
def _blank(h, w):
    return np.full((h, w), LO, f32), np.full((8, h, w), LO, f32)


def _row(name, score, link, min_size=0, max_comps=None, tp=TP, tl=TL, **meta):
    h, w = score.shape
    return NS(name=name, score=score, link=link, min_size=min_size, max_comps=max_comps or h * w, tp=tp, tl=tl, h=h, w=w, **meta)


def _dir(dy, dx):
    return [d for d in range(8) if (KDY[d], KDX[d]) == (dy, dx)][0]


def _link_all(score, link):
    """every link of every positive pixel towards a positive neighbour high"""
    h, w = score.shape
    for y, x in np.argwhere(score > TP):
        for d in range(8):
            ny, nx = y + KDY[d], x + KDX[d]
            if 0 <= ny < h and 0 <= nx < w and score[ny, nx] > TP:
                link[d, y, x] = HI


def _random(h, w):
    rng = _rng("decode", "random", h, w)
    score = rng.uniform(size=(h, w)).astype(f32)
    link = rng.uniform(size=(8, h, w)).astype(f32)
    return _row("random-%dx%d" % (h, w), score, link, min_size=2, tp=f32(0.4), tl=f32(0.85))


def _serpentine(h=67, w=70):
    """a one-pixel snake over the odd rows, joined at alternating ends; each edge linked in ONE random direction"""
    rng = _rng("decode", "serpentine", h, w)
    path = []
    for k, y in enumerate(range(1, h - 1, 2)):
        xs = range(1, w - 1) if k % 2 == 0 else range(w - 2, 0, -1)
        path += [(y, x) for x in xs]
        if y + 2 < h - 1:
            path.append((y + 1, path[-1][1]))
    score, link = _blank(h, w)
    for y, x in path:
        score[y, x] = HI
    crossings = 0
    for (y0, x0), (y1, x1) in zip(path[:-1], path[1:]):
        crossings += (y0 >> 5, x0 >> 5) != (y1 >> 5, x1 >> 5)
        if rng.integers(2):
            link[_dir(y1 - y0, x1 - x0), y0, x0] = HI
        else:
            link[_dir(y0 - y1, x0 - x1), y1, x1] = HI
    return _row("serpentine", score, link, size=len(path), root=path[0][0] * w + path[0][1], crossings=crossings)


def _late_root(h=67, w=70):
    """a comb: spine in tile (1,1), teeth into tiles (1,0) and (1,1), one short tooth up into tile (0,1)"""
    score, link = _blank(h, w)
    score[33:63, 33] = HI                   # spine
    for y in range(34, 63, 4):
        score[y, 2:33] = HI                 # teeth to the left, across x = 32 | 31 into tile (1,0)
    for y in range(36, 63, 4):
        score[y, 34:63] = HI                # teeth to the right, inside tile (1,1)
    score[29:33, 33] = HI                   # the short tooth: tile (0,1) holds the smallest index
    _link_all(score, link)
    pos = np.argwhere(score > TP)
    first = pos[0]
    share = float(((pos[:, 0] >> 5 == first[0] >> 5) & (pos[:, 1] >> 5 == first[1] >> 5)).mean())
    return _row("late_root", score, link, size=len(pos), root=int(first[0] * w + first[1]), share=share)


def _corner(kind, h=67, w=70):
    """two 3x3 blobs in diagonally opposite tiles that touch only at the tile corner; kind picks the one link between"""
    score, link = _blank(h, w)
    anti = kind.startswith("anti")
    a = (slice(29, 32), slice(32, 35)) if anti else (slice(29, 32), slice(29, 32))
    b = (slice(32, 35), slice(29, 32)) if anti else (slice(32, 35), slice(32, 35))
    score[a] = HI
    score[b] = HI
    for blob in (a, b):                     # links inside each blob only
        ys, xs = range(blob[0].start, blob[0].stop), range(blob[1].start, blob[1].stop)
        for y in ys:
            for x in xs:
                for d in range(8):
                    if y + KDY[d] in ys and x + KDX[d] in xs:
                        link[d, y, x] = HI
    up, down = ((31, 32), (32, 31)) if anti else ((31, 31), (32, 32))
    if kind.endswith("down"):
        link[_dir(down[0] - up[0], down[1] - up[1]), up[0], up[1]] = HI
    elif kind.endswith("up"):
        link[_dir(up[0] - down[0], up[1] - down[1]), down[0], down[1]] = HI
    return _row("corner_" + kind, score, link, ncomp=2 if kind.endswith("none") else 1)


def _border(kind, h=9, w=11):
    score, link = _blank(h, w)
    if kind.startswith("edge"):
        targets = [((0, 5), (1, 5)), ((h - 1, 4), (h - 2, 4)), ((4, 0), (4, 1)), ((5, w - 1), (5, w - 2))]
    else:
        targets = [((0, 0), (1, 1)), ((0, w - 1), (1, w - 2)), ((h - 1, 0), (h - 2, 1)), ((h - 1, w - 1), (h - 2, w - 2))]
    for (by, bx), (iy, ix) in targets:
        score[by, bx] = HI
        score[iy, ix] = HI
        link[:, by, bx] = HI                # the border pixel's own links: never looked at
        if kind.endswith("joined"):
            link[_dir(by - iy, bx - ix), iy, ix] = HI
    return _row("border_" + kind, score, link, ncomp=4 if kind.endswith("joined") else 8)


def _three(centre_links):
    score = np.full((3, 3), HI, f32)
    link = np.full((8, 3, 3), HI, f32)
    if not centre_links:
        link[:, 1, 1] = LO
    return _row("3x3_%s" % ("one" if centre_links else "singletons"), score, link, ncomp=1 if centre_links else 9)


def _thresholds(h=12, w=16):
    rng = _rng("decode", "thresholds", h, w)
    sv = np.array([TP, np.nextafter(TP, f32(1)), np.nextafter(TP, f32(-1)), np.nan, HI, HI, LO], f32)
    lv = np.array([TL, np.nextafter(TL, f32(1)), np.nextafter(TL, f32(-1)), np.nan, HI, LO, LO], f32)
    score = sv[rng.integers(len(sv), size=(h, w))]
    link = lv[rng.integers(len(lv), size=(8, h, w))]
    return _row("thresholds", score, link, values=(sv[:4], lv[:4]))


def _min_size(m, k=5, h=12, w=40):
    """horizontal bars of k and k + 1 pixels (twice, in both orders), fully linked"""
    score, link = _blank(h, w)
    score[2, 3:3 + k] = HI
    score[4, 3:4 + k] = HI
    score[6, 30:31 + k] = HI
    score[8, 30:30 + k] = HI
    score[10, 20] = HI
    _link_all(score, link)
    return _row("min_size-%d" % m, score, link, min_size=m, sizes=[k, k + 1, k + 1, k, 1])


def _singletons(max_comps, h=70, w=70):
    score, link = _blank(h, w)
    score[:] = HI
    return _row("singletons-%d" % max_comps, score, link, max_comps=max_comps, ncomp=h * w)


def _fully_linked(h=70, w=70):
    score = np.full((h, w), HI, f32)
    link = np.full((8, h, w), HI, f32)
    return _row("fully_linked", score, link, ncomp=1, size=h * w, root=0)


def link_rows():
    rows = [_random(h, w) for h, w in ((3, 3), (3, 70), (70, 3), (32, 32), (33, 31), (33, 65), (64, 96), (67, 70))]
    rows += [_serpentine(), _late_root()]
    rows += [_corner(k) for k in ("diag_down", "diag_up", "diag_none", "anti_down", "anti_up", "anti_none")]
    rows += [_border(k) for k in ("edge_alone", "edge_joined", "corner_alone", "corner_joined")]
    rows += [_three(True), _three(False), _thresholds()]
    rows += [_min_size(m) for m in (5, 0, -1)]
    rows += [_singletons(m) for m in (4900, 1025, 16)]
    rows += [_fully_linked()]
    return rows


LINK_ROWS = link_rows()
_REF = {}


def ref_of(row):
    """the flood-fill answer of a row, computed once and shared"""
    if row.name not in _REF:
        _REF[row.name] = link_ref(row.score, row.link, row.tp, row.tl, row.min_size)
    return _REF[row.name]


# ------------------------------------------------------------------------------------------------ device plumbing
def _i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)


def _f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(device)


def _u8(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(device)


def _size(L, name, *ints):
    return int(L._fn(name, SZ)(*[ctypes.c_int(int(v)) for v in ints]))


def _ws(nbytes, device):
    return Guard((nbytes,), U8, device)


def _table(got, k, what):
    """rows [0, k) of a table are written, rows [k, ...) still hold the fill (every byte 0xFF: -1, or a NaN)"""
    got = np.asarray(got)
    flat = got.reshape(got.shape[0], -1).view(np.int32)
    assert (flat[k:] == -1).all(), "%s: rows at or beyond %d were written" % (what, k)
    return got[:k]


def _cc_outputs(n, h, w, max_comps, device):
    return Guard((n, h, w), I32, device), Guard((n,), I32, device), Guard((n, max_comps, 2), I32, device)


def _cc_read(lab, nc, cp, ws, max_comps):
    torch.cuda.synchronize()
    assert ws.ok(), "written outside the workspace"
    labels, ncomp, comps = lab.raw(), nc.raw(), cp.raw()
    assert (labels >= 0).all() and (ncomp >= 0).all(), "labels / ncomp not written"
    return labels, ncomp, [_table(comps[i], min(int(ncomp[i]), max_comps), "comps") for i in range(len(ncomp))]


def run_link_cc(L, device, score, link, tp, tl, min_size, max_comps, layout):
    """score [n, h, w], link [8, n, h, w] -> (labels, ncomp, [comps rows per image]) of one raw call"""
    n, h, w = score.shape
    if layout == 1:
        lk, stride, off = _f32(link, device), 1, 0
    else:                                   # channel 1 of [8][n][h][w][2]; channel 0 would change the answer
        with np.errstate(invalid="ignore"):
            two = np.stack([np.where(link > tl, LO, HI).astype(f32), link], -1)
        lk, stride, off = _f32(two, device), 2, 1
    lab, nc, cp = _cc_outputs(n, h, w, max_comps, device)
    nbytes = _size(L, "ocr_link_cc_workspace", n, h, w)
    assert nbytes == 4 * (4 * n * h * w + n * (-(-h * w // 1024)))
    ws = _ws(nbytes, device)
    rc = _rc(L, "ocr_link_cc", _f32(score, device), lk, stride, off, n, h, w, FL(tp), FL(tl), min_size, lab, nc, cp, max_comps,
             ws, SZ(nbytes))
    assert rc == OK
    return _cc_read(lab, nc, cp, ws, max_comps)


def run_mask_cc(L, device, mask, value, conn, max_comps):
    n, h, w = mask.shape
    lab, nc, cp = _cc_outputs(n, h, w, max_comps, device)
    nbytes = _size(L, "ocr_link_cc_workspace", n, h, w)
    ws = _ws(nbytes, device)
    assert _rc(L, "ocr_mask_cc", _u8(mask, device), value, conn, n, h, w, lab, nc, cp, max_comps, ws, SZ(nbytes)) == OK
    return _cc_read(lab, nc, cp, ws, max_comps) + (lab, nc, cp)


def _same_cc(got, labels, comps, max_comps, what):
    glab, gn, gcomps = got
    assert int(gn) == len(comps), "%s: ncomp %d, reference %d" % (what, int(gn), len(comps))
    assert np.array_equal(glab, labels), "%s: %d labels differ" % (what, int((glab != labels).sum()))
    want = np.asarray(comps[:max_comps], np.int32).reshape(-1, 2)
    assert np.array_equal(gcomps, want), "%s: the component table differs" % what


# ------------------------------------------------------------------------------------------------ ocr_link_cc
@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("row", LINK_ROWS, ids=lambda r: r.name)
def test_link_cc(device, row, layout):
    L, _ = _lib()
    labels, comps = ref_of(row)
    for key, have in (("ncomp", len(comps)), ("size", comps[0][1] if comps else 0), ("root", comps[0][0] if comps else -1)):
        if hasattr(row, key):               # what the generator promises about its own map
            assert getattr(row, key) == have, (row.name, key, have)
    glab, gn, gcomps = run_link_cc(L, device, row.score[None], row.link[:, None], row.tp, row.tl, row.min_size, row.max_comps, layout)
    _same_cc((glab[0], gn[0], gcomps[0]), labels, comps, row.max_comps, row.name)


def test_link_cc_batch(device):
    """n = 3: a dense image, an all-negative one and the serpentine.  Each image equals its own n = 1 result bit for bit."""
    L, _ = _lib()
    dense, snake = LINK_ROWS[7], LINK_ROWS[8]
    assert dense.name == "random-67x70" and snake.name == "serpentine"
    tp, tl, min_size = dense.tp, dense.tl, 2
    score = np.stack([dense.score, np.full_like(dense.score, LO), snake.score])
    link = np.stack([dense.link, np.full_like(dense.link, HI), snake.link], 1)
    for layout in (1, 2):
        glab, gn, gcomps = run_link_cc(L, device, score, link, tp, tl, min_size, 256, layout)
        assert gn[1] == 0 and not glab[1].any() and gn[2] == 1 and gcomps[2].tolist() == [[snake.root, snake.size]]
        for i in range(3):
            one = run_link_cc(L, device, score[i:i + 1], link[:, i:i + 1], tp, tl, min_size, 256, layout)
            assert np.array_equal(one[0][0], glab[i]) and one[1][0] == gn[i] and np.array_equal(one[2][0], gcomps[i]), i
            labels, comps = link_ref(score[i], link[:, i], tp, tl, min_size)
            _same_cc((glab[i], gn[i], gcomps[i]), labels, comps, 256, "image %d" % i)


# ------------------------------------------------------------------------------------------------ ocr_mask_cc
def _staircase(anti, h=40, w=66):
    m = np.zeros((h, w), np.uint8)
    for k in range(8):
        m[28 + k, 35 - k if anti else 28 + k] = 1       # (31,31) -> (32,32), or (31,32) -> (32,31): down-left over x = 32 | 31
    return m


def _rings(h=33, w=65, depth=3):
    m = np.zeros((h, w), np.uint8)
    for k in range(0, 4 * depth, 4):
        m[k:h - k, k:w - k] = 1
        m[k + 1:h - k - 1, k + 1:w - k - 1] = 0
    return m


def mask_rows():
    ys, xs = np.mgrid[0:33, 0:65]
    rng = _rng("decode", "mask", "bytes")
    noise = (rng.uniform(size=(40, 66)) < 0.55)
    return [NS(name="checkerboard", mask=((ys + xs) & 1).astype(np.uint8)[None]),
            NS(name="staircase", mask=_staircase(False)[None]), NS(name="anti_staircase", mask=_staircase(True)[None]),
            NS(name="rings", mask=_rings()[None]), NS(name="zeros", mask=np.zeros((1, 33, 65), np.uint8)),
            NS(name="ones", mask=np.ones((1, 33, 65), np.uint8)),
            NS(name="bytes", mask=(noise * rng.choice(np.array([1, 2, 255], np.uint8), size=noise.shape))[None]),
            NS(name="batch2", mask=np.stack([noise.astype(np.uint8), _staircase(True)]))]


MASK_ROWS = mask_rows()


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("row", MASK_ROWS, ids=lambda r: r.name)
def test_mask_cc(device, row, conn, value):
    L, _ = _lib()
    n, h, w = row.mask.shape
    glab, gn, gcomps = run_mask_cc(L, device, row.mask, value, conn, h * w)[:3]
    for i in range(n):
        labels, comps = mask_ref(row.mask[i], value, conn)
        _same_cc((glab[i], gn[i], gcomps[i]), labels, comps, h * w, "%s image %d" % (row.name, i))
    count = int(gn[0])
    if row.name == "checkerboard":
        assert count == (1 if conn == 8 else int(((row.mask[0] != 0) == (value != 0)).sum()))
    if row.name in ("staircase", "anti_staircase") and value == 1:
        assert count == (1 if conn == 8 else 8)
    if row.name == "rings" and value == 1:
        assert count == 3
    if row.name in ("zeros", "ones"):
        assert count == (1 if (row.name == "ones") == (value == 1) else 0)


# ------------------------------------------------------------------------------------------------ rectangles
def _scaled(ys, xs, sx, sy):
    return np.stack([(xs * sx).astype(np.int64), (ys * sy).astype(np.int64)], 1)      # the (int)(x * scale) truncation


def _rect_ref(points):
    """(hull_n, hull_head [4], calipers [6]) of a point set [k, 2] (x, y); None for an empty one"""
    if len(points) == 0:
        return None
    _, cal, hull = C.min_area_rect(points)
    assert np.array_equal(hull, C.convex_hull(points))
    head = np.zeros(4, np.int32)
    head[:2] = hull[0]
    if len(hull) > 1:
        head[2:] = hull[1]
    return len(hull), head, cal


def _check_rects(got, refs, k, what):
    """refs[i]: _rect_ref of id i + 1 for i < k; rows >= k hold the fill; a row with hull_n 0 has nothing else written"""
    hn, hd, cal = (np.asarray(a) for a in got)
    _table(hn, k, what + " hull_n"), _table(hd, k, what + " hull_head"), _table(cal, k, what + " calipers")
    for i in range(k):
        if refs[i] is None:
            assert hn[i] == 0 and (hd[i] == -1).all() and (cal[i].view(np.int32) == -1).all(), (what, i)
            continue
        n_ref, head, c6 = refs[i]
        assert hn[i] == n_ref and np.array_equal(hd[i], head), (what, i, hn[i], n_ref, hd[i], head)
        assert cal[i].tobytes() == c6.tobytes(), (what, i, cal[i], c6)
        if n_ref <= 2:
            assert not cal[i].any()


def run_min_area_rects(L, device, labels, ncomp, max_comps, sx, sy):
    n, h, w = labels.shape
    hn, hd, cal = Guard((n, max_comps), I32, device), Guard((n, max_comps, 4), I32, device), Guard((n, max_comps, 6), F32, device)
    nbytes = _size(L, "ocr_min_area_rects_workspace", n, h, w, max_comps)
    assert nbytes == 4 * (3 * n * (max_comps + 1) + 2 * n * h * w)
    ws = _ws(nbytes, device)
    rc = _rc(L, "ocr_min_area_rects", labels if isinstance(labels, torch.Tensor) else _i32(labels, device),
             ncomp if isinstance(ncomp, torch.Tensor) else _i32(ncomp, device), n, h, w, max_comps, DB(sx), DB(sy), hn, hd, cal, ws,
             SZ(nbytes))
    assert rc == OK
    torch.cuda.synchronize()
    assert ws.ok()
    return hn.raw(), hd.raw(), cal.raw()


def run_hole_border_rects(L, device, mask, zlabels, nregions, max_regions, sx, sy):
    n, h, w = mask.shape
    hn, hd, cal = Guard((n, max_regions), I32, device), Guard((n, max_regions, 4), I32, device), Guard((n, max_regions, 6), F32, device)
    nbytes = _size(L, "ocr_hole_border_rects_workspace", n, h, w, max_regions)
    ws = _ws(nbytes, device)
    rc = _rc(L, "ocr_hole_border_rects", _u8(mask, device), zlabels if isinstance(zlabels, torch.Tensor) else _i32(zlabels, device),
             nregions if isinstance(nregions, torch.Tensor) else _i32(nregions, device), n, h, w, max_regions, DB(sx), DB(sy), hn, hd,
             cal, ws, SZ(nbytes))
    assert rc == OK
    torch.cuda.synchronize()
    assert ws.ok()
    return hn.raw(), hd.raw(), cal.raw()


def _shapes_map(h=64, w=80):
    """hand-made labels: id -> shape; id 9 has no pixel"""
    lab = np.zeros((h, w), np.int32)
    lab[3, 5] = 1                                           # one pixel
    lab[3, 20:22] = 2                                       # two pixels
    lab[8, 4:40] = 3                                        # horizontal line
    lab[10:50, 2] = 4                                       # vertical line
    for k in range(12):
        lab[12 + k, 10 + k] = 5                             # diagonal
        lab[12 + k, 40 - k] = 6                             # anti-diagonal
    lab[30:41, 45:70] = 7                                   # axis-aligned rectangle
    ys, xs = np.mgrid[0:h, 0:w]
    th = 0.5
    u = (xs - 30) * np.cos(th) + (ys - 45) * np.sin(th)
    v = -(xs - 30) * np.sin(th) + (ys - 45) * np.cos(th)
    lab[(np.abs(u) <= 14) & (np.abs(v) <= 4) & (lab == 0)] = 8       # rotated rectangle
    lab[52:62, 60:63] = 10                                  # an L
    lab[59:62, 63:78] = 10
    return lab, 10


def _label_refs(lab, k, sx, sy):
    refs = []
    for i in range(1, k + 1):
        ys, xs = np.nonzero(lab == i)
        refs.append(_rect_ref(_scaled(ys, xs, sx, sy)))
    return refs


SCALES = [(1.0, 1.0), (4.0, 4.0), (2.5, 1.75)]


@pytest.mark.parametrize("sx,sy", SCALES)
def test_min_area_rects(device, sx, sy):
    L, _ = _lib()
    lab, k = _shapes_map()
    labels = np.stack([lab, np.zeros_like(lab), lab[::-1].copy()])          # n = 3: the map, an empty image, the map flipped
    ncomp = np.array([k, 0, k], np.int32)
    max_comps = 13
    hn, hd, cal = run_min_area_rects(L, device, labels, ncomp, max_comps, sx, sy)
    for i in range(3):
        refs = _label_refs(labels[i], ncomp[i], sx, sy)
        sizes = [r[0] if r else 0 for r in refs]
        if i == 1:
            assert sizes == []
        elif sx == sy:
            assert sizes == [1, 2, 2, 2, 2, 2, 4, sizes[7], 0, 5] and sizes[7] > 4
        else:                               # the truncation turns the two diagonals into staircases
            assert sizes == [1, 2, 2, 2, sizes[4], sizes[5], 4, sizes[7], 0, 5] and min(sizes[4], sizes[5], sizes[7]) > 4
        _check_rects((hn[i], hd[i], cal[i]), refs, int(ncomp[i]), "image %d" % i)


def _tall(h, w):
    """ten ring-shaped components with a hole each, stacked along the long side of a 100x5 or 5x100 map"""
    m = np.zeros((100, 5), np.uint8)
    for k in range(10):
        m[10 * k + 1:10 * k + 3 + k % 5, :] = 1
        m[10 * k + 2:10 * k + 2 + k % 5, 1:4] = 0           # k % 5 = 0: a solid bar without a hole
    return m if (h, w) == (100, 5) else np.ascontiguousarray(m.T)


@pytest.mark.parametrize("h,w", [(100, 5), (5, 100)])
@pytest.mark.parametrize("sx,sy", SCALES[1:])
def test_rects_truncated(device, h, w, sx, sy):
    """max_comps / max_regions below the true count: ids beyond the table are ignored, its rows are complete"""
    L, _ = _lib()
    m = _tall(h, w)
    lab, comps = mask_ref(m, 1, 8)
    zl, zcomps = mask_ref(m, 0, 4)
    assert len(comps) == 10 and len(zcomps) >= 9
    for cap in (4, 1):
        got = run_min_area_rects(L, device, lab[None], [len(comps)], cap, sx, sy)
        _check_rects([a[0] for a in got], _label_refs(lab, cap, sx, sy), cap, "components cap %d" % cap)
    for cap in (13, 4):                     # 19 regions; on the wide map the first eleven are background
        got = run_hole_border_rects(L, device, m[None], zl[None], [len(zcomps)], cap, sx, sy)
        refs = _hole_refs(m, zl, cap, sx, sy)
        assert cap == 4 or (any(r is None for r in refs) and any(r is not None for r in refs))
        _check_rects([a[0] for a in got], refs, cap, "holes cap %d" % cap)


# ------------------------------------------------------------------------------------------------ contours
def _hole_points(m, zl, i):
    """the border of 0-region i: 1-pixels with a 4-neighbour in it; None if the region reaches the image edge"""
    reg = zl == i
    if reg[0].any() or reg[-1].any() or reg[:, 0].any() or reg[:, -1].any():
        return None
    near = np.zeros_like(reg)
    near[1:] |= reg[:-1]
    near[:-1] |= reg[1:]
    near[:, 1:] |= reg[:, :-1]
    near[:, :-1] |= reg[:, 1:]
    return np.nonzero(near & (m != 0))


def _hole_refs(m, zl, k, sx, sy):
    refs = []
    for i in range(1, k + 1):
        p = _hole_points(m, zl, i)
        refs.append(None if p is None else _rect_ref(_scaled(p[0], p[1], sx, sy)))
    return refs


def _contour_mask(h=40, w=56):
    m = np.zeros((h, w), np.uint8)
    for k in range(0, 12, 2):               # rings three deep: ring, gap, ring, gap, ring, gap
        v = 1 - (k // 2) % 2
        m[2 + k:26 - k, 20 + k:54 - k] = v
    m[13, 33] = 1                           # an island in the innermost gap
    m[28:38, 0:10] = 1                      # a component in column 0 ...
    m[31:34, 0:4] = 0                       # ... with a notch open to the image edge: background, not a hole
    m[30, 6] = 0                            # a one-pixel hole: its border is its four 4-neighbours only
    m[35:37, 6:8] = 0                       # a 2x2 hole: the four diagonal corners are not on its border
    m[2:7, 2:7] = 1
    m[4, 4] = 0                             # a one-pixel hole in a 5x5 block
    m[38, 50] = 1                           # a single pixel
    return m


def _tree_order(nodes, parent_of):
    """OpenCV's list: children newest (largest discovery key) first, pre-order.  nodes: id -> key."""
    kids = {}
    for nid, key in nodes.items():
        kids.setdefault(parent_of[nid], []).append((key, nid))
    out = []

    def walk(par, ppos):
        for _, nid in sorted(kids.get(par, []), reverse=True):
            me = len(out)
            out.append((nid, ppos))
            walk(nid, me)
    walk(None, -1)
    return out


@pytest.mark.parametrize("sx,sy", SCALES)
def test_contours(device, sx, sy):
    L, _ = _lib()
    m = _contour_mask()
    h, w = m.shape
    cap = h * w
    lab, ncomp, comps, g_lab, g_nc, g_cp = run_mask_cc(L, device, m[None], 1, 8, cap)
    zl, nreg, zcomps, g_zl, g_nz, g_zc = run_mask_cc(L, device, m[None], 0, 4, cap)
    rlab, rcomps = mask_ref(m, 1, 8)
    rzl, rzcomps = mask_ref(m, 0, 4)
    _same_cc((lab[0], ncomp[0], comps[0]), rlab, rcomps, cap, "components")
    _same_cc((zl[0], nreg[0], zcomps[0]), rzl, rzcomps, cap, "0-regions")
    k1, k0 = len(rcomps), len(rzcomps)
    # parents: the region left of each first pixel, 0 in column 0
    pc, pz = Guard((k1 + 3,), I32, device), Guard((k0 + 3,), I32, device)
    assert _rc(L, "ocr_contour_parents", g_lab, g_zl, g_cp, k1, g_zc, k0, h, w, pc, pz) == OK
    torch.cuda.synchronize()
    par_c, par_z = _table(pc.raw(), k1, "parent_c"), _table(pz.raw(), k0, "parent_z")
    assert par_c.tolist() == [int(rzl.flat[f - 1]) if f % w else 0 for f, _ in rcomps]
    assert par_z.tolist() == [int(rlab.flat[f - 1]) if f % w else 0 for f, _ in rzcomps]
    assert 0 in par_c.tolist()
    # rectangles of components and hole borders, straight from the device's own labels
    got1 = run_min_area_rects(L, device, g_lab.t, g_nc.t, cap, sx, sy)
    got0 = run_hole_border_rects(L, device, m[None], g_zl.t, g_nz.t, cap, sx, sy)
    refs1, refs0 = _label_refs(rlab, k1, sx, sy), _hole_refs(m, rzl, k0, sx, sy)
    _check_rects([a[0] for a in got1], refs1, k1, "components")
    _check_rects([a[0] for a in got0], refs0, k0, "holes")
    assert sum(r is None for r in refs0) >= 2                 # the outside and the notch: background
    assert any(r is not None and r[0] == 4 for r in refs0)    # a one-pixel hole: a diamond
    # the contour list rebuilt from those outputs against the border-following restatement
    hn0 = got0[0][0]
    holes = {j for j in range(k0) if hn0[j] > 0}
    nodes, parent_of = {}, {}
    for i in range(k1):
        nodes[(1, i)] = int(comps[0][i][0])
        z = int(par_c[i]) - 1
        parent_of[(1, i)] = (0, z) if z in holes else None
    for j in holes:
        nodes[(0, j)] = int(zcomps[0][j][0])
        parent_of[(0, j)] = (1, int(par_z[j]) - 1)
    order = _tree_order(nodes, parent_of)
    traced, derived = OC.suzuki_contours(m), OC.contour_order(m)
    assert len(order) == len(traced) == len(derived) and max(t[2] for t in traced) >= 5
    rects = []
    for ((kind, i), ppos), (is_hole, pts, tpos), (dkind, dpts, dpos) in zip(order, traced, derived):
        assert (kind == 0) == bool(is_hole) == (dkind == "hole") and ppos == tpos == dpos
        ref = (refs1 if kind else refs0)[i]
        for p in (np.unique(pts, axis=0), dpts):
            want = _rect_ref(_scaled(p[:, 1], p[:, 0], sx, sy))
            assert want[0] == ref[0] and np.array_equal(want[1], ref[1]) and want[2].tobytes() == ref[2].tobytes()
        rects.append(C.min_area_rect(_scaled(dpts[:, 1], dpts[:, 0], sx, sy))[0])
    if (sx, sy) == (1.0, 1.0):
        assert [r.tobytes() for r in rects] == [np.asarray(r, f32).tobytes() for r in OC.contour_boxes(m)[0]]


# ------------------------------------------------------------------------------------------------ small kernels
def test_pixel_detect(device):
    """n = 2; the answer is batch element 0 only, image 1 is a trap"""
    L, _ = _lib()
    rng = _rng("decode", "pixel_detect")
    n, h, w = 2, 33, 31
    ts, tl = f32(0.5), f32(0.25)
    sv = np.array([ts, np.nextafter(ts, f32(1)), np.nan, 0.9, 0.9, 0.9, 0.1], f32)
    lv = np.array([tl, np.nextafter(tl, f32(-1)), np.nan] + [0.9] * 40, f32)
    score = sv[rng.integers(len(sv), size=(n, h, w, 1))]
    link = lv[rng.integers(len(lv), size=(8, n, h, w, 2))]
    score[1] = np.where(score[0] > ts, f32(0.1), f32(0.9))      # the trap: image 1 answers the opposite
    link[:, 1] = f32(0.0)
    link[..., 0] = f32(0.0)                                     # and so does channel 0
    want = O.pixel_detect(score, link, ts, tl)
    assert 0 < want.sum() < h * w and (want != (score[0, :, :, 0] > ts)).any()
    mask = Guard((h, w), U8, device)
    assert _rc(L, "ocr_pixel_detect", _f32(score, device), _f32(link, device), n, h, w, FL(ts), FL(tl), mask) == OK
    torch.cuda.synchronize()
    assert np.array_equal(mask.raw(), want)


def _east_case(h, w):
    hw = h * w
    rng = _rng("decode", "east", h, w)
    tl = f32(0.8)
    link = rng.uniform(0.85, 1.0, size=(hw, 16)).astype(f32)
    link[:, 0::2] = f32(0.0)                                    # the even channels are never read
    mid = hw // 2
    below = [[], [mid], [mid, mid + 1], [0, hw - 1], [hw - 1], [mid // 2, mid], list(rng.integers(hw, size=40)), list(range(hw))]
    for c, idx in enumerate(below):
        for i in idx:
            if 0 <= i < hw:
                link[i, 2 * c + 1] = f32(0.3)
    for i in range(0, min(mid // 2, hw)):                       # channel 5: threshold and NaN before the first real one
        link[i, 11] = tl if i % 2 else np.nan
    score = rng.uniform(size=hw).astype(f32)
    score[::7] = f32(0.8)
    return score, link, tl


@pytest.mark.parametrize("h,w", [(1, 1), (15, 17), (1, 257), (67, 70)])
def test_east_pixel_detect(device, h, w):
    L, _ = _lib()
    hw = h * w
    score, link, tl = _east_case(h, w)
    want = np.full((2, 8), INT_MAX, np.int32)
    for c in range(8):
        with np.errstate(invalid="ignore"):
            idx = np.flatnonzero(link[:, 2 * c + 1] < tl)[:2]
        want[:len(idx), c] = idx
    if hw > 1:
        assert want[0, 0] == INT_MAX and want[1, 1] == INT_MAX and want[0, 1] < INT_MAX and want[1, 2] == want[0, 2] + 1
        assert want[0, 3] == 0 and want[0, 4] == hw - 1 and want[1, 4] == INT_MAX and want[0, 7] == 0 and want[1, 7] == 1
    mask = Guard((h, w), U8, device)
    fs = Guard((2, 8), I32, device, init=np.full((2, 8), INT_MAX, np.int32))
    assert _rc(L, "ocr_east_pixel_detect", _f32(score, device), _f32(link, device), h, w, FL(0.8), FL(tl), mask, fs) == OK
    torch.cuda.synchronize()
    assert np.array_equal(mask.raw().ravel(), (score > f32(0.8)).astype(np.uint8))
    assert np.array_equal(fs.raw(), want), (fs.raw(), want)


def test_east_complete(device):
    """the whole of test.py's pixel_detect: device mask and first / second, the script's index step on the host, the
    sixteen pixels cleared by ocr_zero_pixels_u8 — against oracle.contours.east_pixel_detect"""
    L, _ = _lib()
    rng = _rng("decode", "east_complete")
    h, w = 48, 52
    score = rng.uniform(size=(1, h, w, 1)).astype(f32)
    geo = rng.uniform(0.7, 1.0, size=(1, h, w, 16)).astype(f32)
    want = OC.east_pixel_detect(score, geo, f32(0.8), f32(0.8))
    mask = Guard((h, w), U8, device)
    fs = Guard((2, 8), I32, device, init=np.full((2, 8), INT_MAX, np.int32))
    assert _rc(L, "ocr_east_pixel_detect", _f32(score[0, :, :, 0], device), _f32(geo[0], device), h, w, FL(0.8), FL(0.8), mask, fs) == OK
    torch.cuda.synchronize()
    first, second = fs.raw()
    idx = []
    for c in range(8):
        (y0, x0), (y1, x1) = divmod(int(first[c]), w), divmod(int(second[c]), w)
        idx += [y0 * w + y1, x0 * w + x1]                       # res[[y0, x0], [y1, x1]] = 0
    assert len(idx) == 16 and max(idx) < h * w
    assert _rc(L, "ocr_zero_pixels_u8", mask, _i32(idx, device), 16) == OK
    torch.cuda.synchronize()
    assert np.array_equal(mask.raw(), want) and (want != (score[0, :, :, 0] > 0.8)).any()


@pytest.mark.parametrize("count", [0, 1, 16, 256])
def test_zero_pixels(device, count):
    L, _ = _lib()
    rng = _rng("decode", "zero_pixels", count)
    size = 300
    idx = rng.integers(size - 1, size=count + 1).astype(np.int32)
    idx[1::3] = idx[0]                                          # duplicate indices
    idx[count] = size - 1                                       # one index past the count: not read
    mask = Guard((size,), U8, device, init=np.full(size, 7, np.uint8))
    assert _rc(L, "ocr_zero_pixels_u8", mask, _i32(idx, device), count) == OK
    torch.cuda.synchronize()
    want = np.full(size, 7, np.uint8)
    want[idx[:count]] = 0
    assert np.array_equal(mask.raw(), want)


def _softmax_operands(rng, shape):
    """logit pairs [..., 2]: random, equal, 200 apart (both orders), +-80, NaN in either or both slots"""
    x = (rng.standard_normal(shape + (2,)) * 4).astype(f32)
    flat = x.reshape(-1, 2)
    special = np.array([[1.5, 1.5], [100, -100], [-100, 100], [80, -80], [-80, 80], [np.nan, 1], [1, np.nan], [np.nan, np.nan],
                        [0, 0], [-3, 197], [30, 29.5]], f32)
    k = min(len(flat), len(special))
    pos = rng.permutation(len(flat))[:k]
    flat[pos] = special[:k]
    return x


def _softmax_check(entry, row, got, x):
    """got, x [..., 2] in the same order"""
    x64 = x.astype(f64)
    mx = np.maximum(x64[..., :1], x64[..., 1:])
    e = np.exp(x64 - mx)
    ref = e / e.sum(-1, keepdims=True)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(nan[..., 0], np.isnan(x).any(-1))
    far = (np.abs(x64[..., 0] - x64[..., 1]) >= 200) & ~nan[..., 0]
    assert np.array_equal(got[far], (x[far] == x[far].max(-1, keepdims=True)).astype(f32)), "200 apart: exactly 1 and 0"
    d = np.abs(x64[..., :1] - x64[..., 1:])
    bound = _g(7 + d * (x64 < mx)) * ref + 2.0 ** -149
    _note(entry, row, _ratio(np.abs(got.astype(f64) - ref), bound, skip=nan))


@pytest.mark.parametrize("m", [1, 255, 257, 4096 * 256 + 257])
def test_softmax_pairs(device, m):
    L, _ = _lib()
    x = _softmax_operands(_rng("decode", "softmax_pairs", m), (m,))
    out = Guard((m, 2), F32, device)
    assert _rc(L, "ocr_softmax_pairs", _f32(x, device), I64(m), out) == OK
    torch.cuda.synchronize()
    _softmax_check("softmax_pairs", "m%d" % m, out.raw(), x)


@pytest.mark.parametrize("m", [1, 255, 257, 4096 * 256 // 8 + 33])
def test_link_softmax_stack(device, m):
    """[m][16] -> [8][m][2]; every direction has logits of its own, so a wrong slot of the stack cannot match"""
    L, _ = _lib()
    x = _softmax_operands(_rng("decode", "link_softmax_stack", m), (m, 8))
    x[..., 0] += np.arange(8, dtype=f32) * f32(0.25)
    out = Guard((8, m, 2), F32, device)
    assert _rc(L, "ocr_link_softmax_stack", _f32(x.reshape(m, 16), device), I64(m), out) == OK
    torch.cuda.synchronize()
    _softmax_check("link_softmax_stack", "m%d" % m, out.raw(), np.ascontiguousarray(x.transpose(1, 0, 2)))


# ------------------------------------------------------------------------------------------------ ocr_link_cc_directed
def run_directed(L, device, score, link, tp, tl, min_size, max_comps):
    n, h, w = score.shape
    sc, lk = _f32(score, device), _f32(link, device)
    ulab, unc, ucp = _cc_outputs(n, h, w, max_comps, device)
    nbytes = _size(L, "ocr_link_cc_workspace", n, h, w)
    ws = _ws(nbytes, device)
    assert _rc(L, "ocr_link_cc", sc, lk, 1, 0, n, h, w, FL(tp), FL(tl), min_size, ulab, unc, ucp, max_comps, ws, SZ(nbytes)) == OK
    lab, nc, cp = _cc_outputs(n, h, w, max_comps, device)
    nbytes = _size(L, "ocr_link_cc_directed_workspace", n, h, w)
    assert nbytes == n * h * w * 24
    ws = _ws(nbytes, device)
    rc = _rc(L, "ocr_link_cc_directed", sc, lk, 1, 0, n, h, w, FL(tp), FL(tl), min_size, ulab, unc, None, lab, nc, cp, max_comps, ws,
             SZ(nbytes))
    assert rc == OK
    return _cc_read(lab, nc, cp, ws, max_comps)


def test_directed(device):
    L, _ = _lib()
    rng = _rng("decode", "directed")
    n, h, w = 2, 33, 31
    score = rng.uniform(size=(n, h, w)).astype(f32)
    link = rng.uniform(size=(8, n, h, w)).astype(f32)
    tp, tl, min_size = f32(0.3), f32(0.75), 3
    glab, gn, gcomps = run_directed(L, device, score, link, tp, tl, min_size, h * w)
    for i in range(n):
        want = O.link_cc_reference_dfs(score[i], link[:, i], tp, tl, min_size, key_order="ascending")
        k = int(want.max())
        assert k >= 3 and gn[i] == k and np.array_equal(glab[i], want), i
        assert gcomps[i][:, 1].tolist() == np.bincount(want.ravel(), minlength=k + 1)[1:].tolist()
        assert [int(want.flat[s]) for s in gcomps[i][:, 0]] == list(range(1, k + 1))
        one = run_directed(L, device, score[i:i + 1], link[:, i:i + 1], tp, tl, min_size, h * w)
        assert np.array_equal(one[0][0], glab[i]) and one[1][0] == gn[i] and np.array_equal(one[2][0], gcomps[i]), i
    assert not np.array_equal(glab[0], glab[1])


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes(device):
    """every refusal of the two files, as read from the entries: each returns before the first launch.  The documented
    status comes back and no output, count or workspace word changes."""
    L, _ = _lib()
    n, h, w, mc = 2, 8, 9, 5
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device=device)
    sc, lk, lk16 = z(F32, n, h, w), z(F32, 8, n, h, w, 2), z(F32, n, h, w, 16)
    m8, li, one = z(U8, n, h, w), z(I32, n, h, w), torch.ones(n, dtype=I32, device=device)
    cpi = z(I32, n, mc, 2)
    G = {k: Guard(s, d, device) for k, (s, d) in {
        "lab": ((n, h, w), I32), "nc": ((n,), I32), "cp": ((n, mc, 2), I32), "ws": ((1 << 16,), U8), "mask": ((h, w), U8),
        "fs": ((2, 8), I32), "pc": ((mc,), I32), "pz": ((mc,), I32), "hn": ((n, mc), I32), "hd": ((n, mc, 4), I32),
        "cal": ((n, mc, 6), F32), "sm": ((n * h * w, 2), F32), "st": ((8, n * h * w, 2), F32)}.items()}
    ws_cc = _size(L, "ocr_link_cc_workspace", n, h, w)
    ws_dir = _size(L, "ocr_link_cc_directed_workspace", n, h, w)
    ws_mar = _size(L, "ocr_min_area_rects_workspace", n, h, w, mc)
    ws_hole = _size(L, "ocr_hole_border_rects_workspace", n, h, w, mc)
    assert max(ws_cc, ws_dir, ws_mar, ws_hole) <= G["ws"].nbytes
    P = n * h * w
    # entry: (arguments, indices of the required pointers, indices of the extents that must be positive)
    E = {
        "ocr_softmax_pairs": ([sc, I64(P // 2), G["sm"]], [0, 2], []),
        "ocr_link_softmax_stack": ([lk16, I64(P), G["st"]], [0, 2], []),
        "ocr_pixel_detect": ([sc, lk, n, h, w, FL(0.5), FL(0.5), G["mask"]], [0, 1, 7], [2, 3, 4]),
        "ocr_link_cc": ([sc, lk, 2, 1, n, h, w, FL(0.5), FL(0.5), 0, G["lab"], G["nc"], G["cp"], mc, G["ws"], SZ(ws_cc)],
                        [0, 1, 10, 11, 12, 14], [4, 5, 6, 13]),
        "ocr_link_cc_directed": ([sc, lk, 2, 1, n, h, w, FL(0.5), FL(0.5), 0, li, one, None, G["lab"], G["nc"], G["cp"], mc, G["ws"],
                                  SZ(ws_dir)], [0, 1, 10, 11, 13, 14, 15, 17], [4, 5, 6, 16]),
        "ocr_mask_cc": ([m8, 1, 8, n, h, w, G["lab"], G["nc"], G["cp"], mc, G["ws"], SZ(ws_cc)], [0, 6, 7, 8, 10], [3, 4, 5, 9]),
        "ocr_east_pixel_detect": ([sc, lk16, h, w, FL(0.5), FL(0.5), G["mask"], G["fs"]], [0, 1, 6, 7], [2, 3]),
        "ocr_contour_parents": ([li, li, cpi, mc, cpi, mc, h, w, G["pc"], G["pz"]], [0, 1, 2, 4, 8, 9], [6, 7]),
        "ocr_zero_pixels_u8": ([G["mask"], li, 4], [0, 1], []),
        "ocr_min_area_rects": ([li, one, n, h, w, mc, DB(1.0), DB(1.0), G["hn"], G["hd"], G["cal"], G["ws"], SZ(ws_mar)],
                               [0, 1, 8, 9, 10, 11], [2, 3, 4, 5]),
        "ocr_hole_border_rects": ([m8, li, one, n, h, w, mc, DB(1.0), DB(1.0), G["hn"], G["hd"], G["cal"], G["ws"], SZ(ws_hole)],
                                  [0, 1, 2, 9, 10, 11, 12], [3, 4, 5, 6]),
    }

    def bad(name, j, v, want=INVALID_ARG):
        a = list(E[name][0])
        for jj, vv in zip(np.atleast_1d(j), v if isinstance(v, tuple) else (v,)):
            a[jj] = vv
        assert _rc(L, name, *a) == want, (name, j, v)

    for name, (args, req, ext) in E.items():
        for j in req:
            bad(name, j, None)
        for j in ext:
            for v in (0, -1):
                bad(name, j, v)
    for v in (0, -5):
        bad("ocr_softmax_pairs", 1, I64(v))
        bad("ocr_link_softmax_stack", 1, I64(v))
    for v in (-1, 257):
        bad("ocr_zero_pixels_u8", 2, v)
    for v in (-1, -7):
        bad("ocr_contour_parents", 3, v)
        bad("ocr_contour_parents", 5, v)
    bad("ocr_contour_parents", (3, 5), (INT_MAX, 1), UNSUPPORTED)
    for name, jh, jst in (("ocr_link_cc", 5, 2), ("ocr_link_cc_directed", 5, 2)):
        for v in (1, 2):                                        # h, w >= 3: only interior pixels link
            bad(name, jh, v)
            bad(name, jh + 1, v)
        for st, off in ((0, 0), (-1, 0), (1, 1), (2, 2), (2, -1)):
            bad(name, (jst, jst + 1), (st, off))
        bad(name, (jh, jh + 1), (46341, 46341), UNSUPPORTED)    # h * w > INT32_MAX
    bad("ocr_link_cc_directed", 13, li)                         # labels == union_labels
    for v in (0, 6, -8):
        bad("ocr_mask_cc", 2, v)
    for name, jn in (("ocr_link_cc", 4), ("ocr_mask_cc", 3)):
        bad(name, jn, 65536, UNSUPPORTED)                       # images are gridDim.y
    bad("ocr_mask_cc", (4, 5), (46341, 46341), UNSUPPORTED)
    bad("ocr_pixel_detect", (3, 4), (46341, 46341), UNSUPPORTED)
    bad("ocr_east_pixel_detect", (2, 3), (46341, 46341), UNSUPPORTED)
    for name, jn in (("ocr_min_area_rects", 2), ("ocr_hole_border_rects", 3)):
        bad(name, jn, 65536, UNSUPPORTED)
        bad(name, jn + 1, 1025, UNSUPPORTED)                    # h <= 1024: a component's rows are staged in LDS
        bad(name, jn + 3, 65536, UNSUPPORTED)
        bad(name, jn + 4, DB(0.5), UNSUPPORTED)
        bad(name, jn + 5, DB(0.999), UNSUPPORTED)
        bad(name, jn + 4, DB(float("nan")), UNSUPPORTED)
        bad(name, jn + 4, DB(2.0 ** 24), UNSUPPORTED)           # w * scale_x must stay exact in f32
        bad(name, jn + 5, DB(2.0 ** 24), UNSUPPORTED)
    bad("ocr_min_area_rects", (3, 4), (1024, 2097153), UNSUPPORTED)         # h * w > INT32_MAX
    bad("ocr_hole_border_rects", (4, 5), (1024, 700000), UNSUPPORTED)       # 3 * h * w > INT32_MAX
    bad("ocr_link_cc", 15, SZ(ws_cc - 1), WORKSPACE)
    bad("ocr_link_cc_directed", 18, SZ(ws_dir - 1), WORKSPACE)
    bad("ocr_mask_cc", 11, SZ(ws_cc - 1), WORKSPACE)
    bad("ocr_min_area_rects", 12, SZ(ws_mar - 1), WORKSPACE)
    bad("ocr_hole_border_rects", 13, SZ(ws_hole - 1), WORKSPACE)
    torch.cuda.synchronize()
    for k, g in G.items():
        assert g.untouched(), k
    # nothing to do is not a refusal: no launch, nothing written
    assert _rc(L, "ocr_zero_pixels_u8", G["mask"], li, 0) == OK
    assert _rc(L, "ocr_contour_parents", li, li, cpi, 0, cpi, 0, h, w, G["pc"], G["pz"]) == OK
    torch.cuda.synchronize()
    assert G["mask"].untouched() and G["pc"].untouched() and G["pz"].untouched()
    # and the same buffers take a well-formed call
    assert _rc(L, "ocr_mask_cc", *E["ocr_mask_cc"][0]) == OK
    torch.cuda.synchronize()
    assert G["nc"].raw().tolist() == [0, 0] and not G["lab"].raw().any() and G["cp"].untouched()
