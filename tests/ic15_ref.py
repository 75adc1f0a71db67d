"""Not a test: the ICDAR-2015 Task-1 matching of include/ocr_eval_ic15.h in EXACT arithmetic (fractions.Fraction) — the
classification by integer turns, the triangle split, Sutherland-Hodgman clipping, don't-care detections, the
ground-truth-major greedy walk — and the fixtures of tests/test_ic15_host.py (which pins this file against answers worked
out by hand) and tests/test_gpu_eval_ic15.py (which holds the kernels to it).

A polygon here is 4 (x, y) integer pairs; rect(x0, y0, x1, y1) is the polygon with those corners, area (x1 - x0)(y1 - y0)
(no pixel counting anywhere in this protocol)."""
from fractions import Fraction as Fr

import numpy as np

CONVEX, REFLEX, BOWTIE, ZERO = 0, 1, 2, 3
LIMIT = 2 ** 22
MAX_D, MAX_G, N = 16, 8, 3          # the shapes of the GPU test
HALF = Fr(1, 2)
JITTER_SEEDS = (1, 2, 3)            # the first three seeds; test_ic15_host checks the distance condition on each


def rect(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def normalise(poly):
    """-> (4 integer points, counter-clockwise, a reflex vertex first; kind; area as a Fraction)"""
    p = [(max(-LIMIT, min(LIMIT, int(x))), max(-LIMIT, min(LIMIT, int(y)))) for x, y in np.asarray(poly).reshape(4, 2)]
    s2 = sum(p[i][0] * p[(i + 1) % 4][1] - p[(i + 1) % 4][0] * p[i][1] for i in range(4))
    if s2 < 0:
        p[1], p[3] = p[3], p[1]
    neg = [i for i in range(4)
           if (p[i][0] - p[i - 1][0]) * (p[(i + 1) % 4][1] - p[i][1]) - (p[i][1] - p[i - 1][1]) * (p[(i + 1) % 4][0] - p[i][0]) < 0]
    kind = BOWTIE if len(neg) >= 2 else ZERO if s2 == 0 else REFLEX if len(neg) == 1 else CONVEX
    if kind == REFLEX:
        p = p[neg[0]:] + p[:neg[0]]
    return p, kind, Fr(abs(s2), 2)


def _cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _area(pts):
    return abs(sum(pts[i - 1][0] * pts[i][1] - pts[i][0] * pts[i - 1][1] for i in range(len(pts)))) / 2 if len(pts) >= 3 else Fr(0)


def clip(subject, tri):
    """Sutherland-Hodgman: `subject` clipped by the counter-clockwise triangle `tri`, exact"""
    cur = [(Fr(x), Fr(y)) for x, y in subject]
    for k in range(3):
        c1, c2 = tri[k], tri[(k + 1) % 3]
        nxt = []
        for i in range(len(cur)):
            s, e = cur[i - 1], cur[i]
            ds, de = _cross(c1, c2, s), _cross(c1, c2, e)
            if (ds >= 0) != (de >= 0):
                t = Fr(ds) / (ds - de)
                nxt.append((s[0] + t * (e[0] - s[0]), s[1] + t * (e[1] - s[1])))
            if de >= 0:
                nxt.append(e)
        cur = nxt
    return cur


def intersection(det, gt):
    """exact area(det and gt) by the rule of the header: the convex one clipped by the other one's two triangles"""
    dp, dk, _ = normalise(det)
    gp, gk, _ = normalise(gt)
    if dk > REFLEX or gk > REFLEX or (dk == REFLEX and gk == REFLEX):
        return Fr(0)
    q, t = (gp, dp) if dk == REFLEX else (dp, gp)
    total = Fr(0)
    for tri in ((t[0], t[1], t[2]), (t[0], t[2], t[3])):
        if _cross(*tri) > 0:
            total += _area(clip(q, tri))
    return total


def match_image(dets, gts, dontcare, iou_thr=HALF, area_prec_thr=HALF):
    """one image -> dict(det_match [k], gt_match [g], record [4], inter [g][k], area_d, area_g, iou [g][k], prec [g][k]),
    every number a Fraction or an int"""
    iou_thr, area_prec_thr = Fr(iou_thr), Fr(area_prec_thr)
    k, n_g = len(dets), len(gts)
    area_d = [normalise(d)[2] for d in dets]
    area_g = [normalise(g)[2] for g in gts]
    kind_g = [normalise(g)[1] for g in gts]
    inter = [[intersection(dets[d], gts[g]) for d in range(k)] for g in range(n_g)]
    prec = [[inter[g][d] / area_d[d] if area_d[d] > 0 else Fr(0) for d in range(k)] for g in range(n_g)]
    iou = [[inter[g][d] / (area_g[g] + area_d[d] - inter[g][d]) if area_g[g] + area_d[d] - inter[g][d] != 0 else Fr(0)
            for d in range(k)] for g in range(n_g)]
    det_match = [-2 if any(dontcare[g] and prec[g][d] > area_prec_thr for g in range(n_g)) else -1 for d in range(k)]
    gt_match = [-2 if dontcare[g] or kind_g[g] == BOWTIE else -1 for g in range(n_g)]
    for g in range(n_g):
        for d in range(k):
            if gt_match[g] == -1 and det_match[d] == -1 and iou[g][d] > iou_thr:
                gt_match[g], det_match[d] = d, g
    matched = sum(m >= 0 for m in gt_match)
    record = [sum(m != -2 for m in gt_match), matched, sum(m != -2 for m in det_match) - matched, k]
    return dict(det_match=det_match, gt_match=gt_match, record=record, inter=inter, area_d=area_d, area_g=area_g, iou=iou,
                prec=prec)


def _image(dets, gts, dontcare):
    return (np.asarray(dets, np.int32).reshape(-1, 4, 2), np.asarray(gts, np.int32).reshape(-1, 4, 2),
            np.asarray(dontcare, bool).reshape(-1))


# the chevron (0,0) (10,4) (20,0) (10,12): the triangle (0,0) (20,0) (10,12) of area 120 without the notch (0,0) (20,0)
# (10,4) of area 40; the reflex vertex is (10,4).  Every rotation of the vertex list, both orientations.
CHEVRON = [[0, 0], [10, 4], [20, 0], [10, 12]]
CHEVRONS = [CHEVRON[r:] + CHEVRON[:r] for r in range(4)] + [(CHEVRON[r:] + CHEVRON[:r])[::-1] for r in range(4)]
BOW_TIE = [[0, 0], [10, 10], [10, 0], [0, 10]]
A, A_NEAR, B = rect(10, 10, 30, 30), rect(11, 10, 30, 31), rect(40, 40, 60, 60)

# (case, image) that hold pairs whose exact IoU or area precision IS the threshold: every polygon there is an axis-aligned
# rectangle on the integer lattice and no edge crosses another, so every clip vertex is a lattice point, float64 is exact
# and the strict comparison is decided as here
TIE_IMAGES = {("half_iou_is_no_match", 0), ("half_iou_is_no_match", 2), ("dontcare_half_precision", 0),
              ("dontcare_half_precision", 2)}


def directed_cases():
    """name -> ([3 images of (dets [k,4,2], gts [g,4,2], dontcare [g])], expected [(det_match, gt_match)] worked out by hand)"""
    c = {}
    c["identical_and_order"] = ([
        _image([A], [A], [0]),                              # IoU 1
        _image([A, A_NEAR], [A], [0]),                      # both above 0.5: the lower detection index wins, the other is fp
        _image([A], [A, A_NEAR], [0, 0]),                   # one detection over two ground truths: gt 0 takes it
    ], [([0], [0]), ([0, -1], [0]), ([0], [0, -1])])
    c["half_iou_is_no_match"] = ([
        _image([rect(0, 0, 10, 10)], [rect(0, 0, 20, 10)], [0]),          # 100 / (200 + 100 - 100) = 1/2: strict, no match
        _image([rect(0, 0, 11, 10)], [rect(0, 0, 20, 10)], [0]),          # 110 / 200: match
        _image([rect(0, 0, 10, 10), rect(0, 0, 11, 10)], [rect(0, 0, 20, 10)], [0]),
    ], [([-1], [-1]), ([0], [0]), ([-1, 0], [1])])
    c["dontcare_half_precision"] = ([
        _image([rect(0, 0, 20, 10)], [rect(0, 0, 10, 10)], [1]),          # 100 / 200 = 1/2 of the detection: it still counts
        _image([rect(0, 0, 20, 10)], [rect(0, 0, 11, 10)], [1]),          # 110 / 200: a don't-care detection
        _image([rect(0, 0, 20, 10), rect(0, 0, 20, 10)], [rect(0, 0, 10, 10), rect(0, 0, 20, 10), rect(9, 0, 20, 10)], [1, 0, 1]),
    ], [([-1], [-2]), ([-2], [-2]), ([-2, -2], [-2, -1, -2])])            # image 2: 110 / 200 inside gt 2, so gt 1 finds nobody
    # detections: the left half's box (inter 40), the strip y <= 4 (inter 200/3 - 40 = 80/3), the whole box (80), and the
    # enclosing triangle with a doubled vertex (inter 80, IoU 80 / 120: the only match, taken by gt 0)
    chev_dets = [rect(0, 0, 10, 12), rect(0, 0, 20, 4), rect(0, 0, 20, 12), [[0, 0], [20, 0], [10, 12], [10, 12]]]
    c["chevron"] = ([
        _image(chev_dets, CHEVRONS, [0] * 8),
        _image(chev_dets[::-1], CHEVRONS[4:] + CHEVRONS[:4], [1, 0, 0, 0, 0, 0, 0, 0]),
        _image([CHEVRON, chev_dets[3]], [rect(0, 0, 20, 13), CHEVRON], [0, 0]),
    ], [([-1, -1, -1, 0], [3] + [-1] * 7), ([-2, -1, -1, -1], [-2] + [-1] * 7), ([-1, 1], [-1, 1])])
    # image 0: IoUs 40 / 160, (80/3) / (400/3), 80 / 240, 80 / 120.  Image 1: gt 0 is don't-care and holds 80 / 120 of the
    # triangle (a don't-care detection), a third of each of the others; nothing else reaches 1/2.  Image 2: a reflex
    # DETECTION against a convex gt is clipped from the gt's side (80 / 260), reflex against reflex is outside the contract
    # (0), the triangle takes the chevron gt (80 / 120) after missing the box (120 / 260)
    c["bow_tie_and_zero_area"] = ([
        _image([rect(0, 0, 10, 10)], [BOW_TIE], [0]),                     # a bow-tie meets nothing and is not a care gt
        _image([rect(5, 5, 15, 5), A], [A, rect(5, 5, 15, 5)], [0, 0]),   # zero-area detection: fp; zero-area gt: care, unmatched
        _image([BOW_TIE, rect(0, 0, 10, 10)], [rect(0, 0, 10, 10), BOW_TIE], [1, 1]),      # bow-tie detection: prec 0, counts as fp
    ], [([-1], [-2]), ([-1, 0], [1, -1]), ([-1, -2], [-2, -2])])
    c["empty_and_negative"] = ([
        _image([A, B], np.zeros((0, 4, 2)), []),                          # ng = 0: every detection is a false positive
        _image(np.zeros((0, 4, 2)), [A, B], [0, 1]),                      # nd = 0
        _image([rect(-30, -30, -10, -10), rect(-5, -5, 5, 5)], [rect(-4, -6, 5, 5), rect(-30, -29, -10, -10)], [0, 0]),
    ], [([-1, -1], []), ([], [-1, -2]), ([1, 0], [1, 0])])
    return c


def _rot_rect(cx, cy, hw, hh, a):
    co, si = np.cos(a), np.sin(a)
    local = np.array([[-hw, -hh], [hw, -hh], [hw, hh], [-hw, hh]])
    return np.rint(np.stack([cx + local[:, 0] * co - local[:, 1] * si, cy + local[:, 0] * si + local[:, 1] * co], axis=1)).astype(np.int32)


def jittered_cases(seed):
    """3 images: ground truths = rotated rectangles on a 300 x 300 canvas (one per image bent into a chevron, a third of
    them don't-care), detections = rotated, scaled, shifted copies of them (IoUs spread over 0.2 .. 0.9) plus strays"""
    rng = np.random.default_rng(seed)
    images = []
    for n_g, n_d in ((MAX_G, MAX_D), (5, 9), (3, 12)):
        par = [(rng.uniform(40, 260), rng.uniform(40, 260), rng.uniform(12, 40), rng.uniform(6, 20), rng.uniform(-0.8, 0.8))
               for _ in range(n_g)]
        gts = np.stack([_rot_rect(*p) for p in par])
        j = int(rng.integers(0, 4))
        gts[0, j] = np.rint(gts[0, j] + 0.7 * (gts[0, (j + 2) % 4] - gts[0, j])).astype(np.int32)      # past the diagonal: reflex
        if rng.integers(0, 2):
            gts[0] = gts[0, ::-1]                                                                   # and clockwise, sometimes
        dets = []
        for d in range(n_d):
            if d % 4 == 3:
                dets.append(_rot_rect(rng.uniform(40, 260), rng.uniform(40, 260), rng.uniform(8, 30), rng.uniform(5, 15), rng.uniform(-0.8, 0.8)))
            else:
                cx, cy, hw, hh, a = par[int(rng.integers(0, n_g))]
                dets.append(_rot_rect(cx + rng.uniform(-0.3, 0.3) * hw, cy + rng.uniform(-0.3, 0.3) * hh, hw * rng.uniform(0.75, 1.25),
                                      hh * rng.uniform(0.75, 1.25), a + rng.uniform(-0.12, 0.12)))
        images.append(_image(np.stack(dets), gts, rng.integers(0, 3, n_g) == 0))
    return images
