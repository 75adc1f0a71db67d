"""Not a test: the NumPy reference of the multi-scale pool and fusion (include/ocr_multiscale.h), written as sequential
loops, and the case generators of tests/test_multiscale_host.py and tests/test_gpu_multiscale.py.

  append_ref   one scale of one image appended to the pooled list: float32 divisions, keep order, the three counters
  fuse_ref     stable rank, greedy sweep with the owner record, and (mode 1) the vote: float64 sums in visiting order;
               pair verdicts through the C clipper of oracle/lanms_oracle.c (`oracle.lanms.iou`'s function), the one
               the device is pinned to
  cluster_case rotated rectangles in clusters: sites along a chain, jittered copies of every site at "other scales"
"""
import ctypes

import numpy as np

from oracle import lanms as OL

f32, i32 = np.float32, np.int32
MODES = {"nms": 0, "vote": 1}


# ------------------------------------------------------------------------------------------------ append
def append_ref(pool, pool_scale, counters, merged, keep, n_keep, passed, mean, ratio, scale_id):
    """pool f32 [max_pool,9], pool_scale int32 [max_pool] and counters = [count, total, nonfinite] of ONE image are updated
    in place from one scale's merged f32 [max_k,9], keep int32 [max_k], n_keep, passed (bool / uint8 [max_k] or None), mean f32
    [max_k], ratio f32 [2] = (ratio_w, ratio_h)."""
    max_pool, max_k = pool.shape[0], merged.shape[0]
    rw, rh = f32(ratio[0]), f32(ratio[1])
    nk = min(max(int(n_keep), 0), max_k)
    with np.errstate(all="ignore"):
        for j in range(nk):
            if passed is not None and not passed[j]:
                continue
            r = int(keep[j])
            if not 0 <= r < max_k:
                counters[2] += 1
                continue
            row = np.empty(9, f32)
            for k in range(8):
                row[k] = f32(merged[r, k]) / (rh if k & 1 else rw)
            row[8] = mean[j]
            if not np.isfinite(row).all():
                counters[2] += 1
                continue
            if counters[1] < max_pool:
                pool[counters[1]] = row
                pool_scale[counters[1]] = scale_id
            counters[1] += 1
    counters[0] = min(counters[1], max_pool)


# ------------------------------------------------------------------------------------------------ fuse
def rank(scores):
    """pool indices in rank order: descending score, ties in pool order, NaN last"""
    s = np.asarray(scores, f32)
    nan = np.isnan(s)
    idx = np.arange(len(s))
    return np.concatenate([idx[~nan][np.argsort(-s[~nan], kind="stable")], idx[nan]]).astype(np.int64)


_iou_fn = None


def iou_rows(rows, a, b):
    """oracle.lanms.iou(rows[a], rows[b]) without the per-call copies: rows is a C-contiguous float32 [P,9] array"""
    global _iou_fn
    if _iou_fn is None:
        _iou_fn = OL._load().lanms_oracle_iou
        _iou_fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    base = rows.ctypes.data
    return float(_iou_fn(base + 36 * int(a), base + 36 * int(b)))


def best_shift(q, qk):
    """the cyclic vertex shift r of member q [8] nearest the kept quad qk [8]: squared distances in float64 from the float32
    values, x term then y term, vertex by vertex; ties to the smallest r"""
    best, best_r = None, 0
    for r in range(4):
        d = 0.0
        for p in range(4):
            dx = float(q[2 * ((p + r) & 3)]) - float(qk[2 * p])
            dy = float(q[2 * ((p + r) & 3) + 1]) - float(qk[2 * p + 1])
            d = d + dx * dx
            d = d + dy * dy
        if r == 0 or d < best:
            best, best_r = d, r
    return best_r


def fuse_ref(pool, thr, mode):
    """pool f32 [P,9] (the rows below the count) -> (fused f32 [P,9], keep int [K] in rank order, owner int [P])"""
    rows = np.ascontiguousarray(pool, f32)
    P = len(rows)
    thr = float(f32(thr))
    order = rank(rows[:, 8]) if P else np.zeros(0, np.int64)
    owner = np.full(P, -1, np.int64)
    keep = []
    for ia, a in enumerate(order):
        if owner[a] != -1:
            continue
        owner[a] = a
        keep.append(int(a))
        for b in order[ia + 1:]:
            if owner[b] == -1 and iou_rows(rows, a, b) > thr:
                owner[b] = a
    fused = rows.copy()
    if MODES.get(mode, mode) == 1:
        for k in keep:
            W, C = 0.0, [0.0] * 8
            for j in order:
                if owner[j] != k:
                    continue
                r = best_shift(rows[j], rows[k])
                s = float(rows[j, 8])
                W = W + s
                for c in range(8):
                    C[c] = C[c] + s * float(rows[j, (c + 2 * r) & 7])
            if W != 0.0:
                with np.errstate(all="ignore"):
                    fused[k, :8] = [f32(np.float64(C[c]) / np.float64(W)) for c in range(8)]
    return fused, np.asarray(keep, np.int64), owner


# ------------------------------------------------------------------------------------------------ cases
def rot_rect(cx, cy, w, h, angle):
    """the four corners (clockwise in image coordinates, from the top-left one) of a rotated rectangle -> f32 [8]"""
    c, s = np.cos(angle), np.sin(angle)
    pts = [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)]
    return np.array([v for x, y in pts for v in (cx + c * x - s * y, cy + s * x + c * y)], f32)


def cluster_case(P, seed, n_scales=3):
    """P pooled quads (f32 [P,9], scale int32 [P], cluster int32 [P]) in scale-major order.  Clusters sit on a 400-px grid;
    a cluster is one to three SITES in a chain (0.55 of the word's length apart along its axis: neighbours have IoU ~0.29 —
    between the two thresholds the tests use — and the outer two do not touch, so at 0.2 an outer site survives when the
    middle one is claimed), a site is one to three jittered copies "found at other scales" (IoU ~0.8); scores
    are multiples of 1/32 (ties), and one copy in five is stored one to three corners round."""
    rng = np.random.default_rng(seed)
    rows, scale, cluster = [], [], []
    grid = int(np.ceil(np.sqrt(max(P, 1)))) + 1
    c_id = 0
    while len(rows) < P:
        cx, cy = 200 + 400 * (c_id % grid), 200 + 400 * (c_id // grid)
        w, h = rng.uniform(60, 120), rng.uniform(16, 36)
        ang = rng.uniform(-np.pi / 4, np.pi / 4)
        full = c_id % 3 == 0                      # every third cluster: three sites of two copies, the top score at an outer one
        for site in range(3 if full else int(rng.integers(1, 4))):
            sx, sy = cx + (site - 1) * 0.55 * w * np.cos(ang), cy + (site - 1) * 0.55 * w * np.sin(ang)
            for copy in range(2 if full else int(rng.integers(1, 4))):
                if len(rows) == P:
                    break
                q = rot_rect(sx + rng.uniform(-1.5, 1.5), sy + rng.uniform(-1.5, 1.5), w + rng.uniform(-2, 2),
                             h + rng.uniform(-1, 1), ang + rng.uniform(-0.02, 0.02))
                if rng.uniform() < 0.2:
                    q = np.roll(q, -2 * int(rng.integers(1, 4)))
                score = 1.0 if full and site == 0 and copy == 0 else rng.integers(8, 32) / 32.0
                rows.append(np.concatenate([q, [f32(score)]]).astype(f32))
                scale.append(int(rng.integers(0, n_scales)))
                cluster.append(c_id)
        c_id += 1
    rows, scale, cluster = np.array(rows, f32).reshape(-1, 9), np.array(scale, i32), np.array(cluster, i32)
    by_scale = np.argsort(scale, kind="stable")
    return np.ascontiguousarray(rows[by_scale]), scale[by_scale], cluster[by_scale]


# the pooled counts of the GPU fuse test's batch (one image each), and the seeds of the two batches
FUSE_COUNTS = (0, 1, 2, 63, 64, 65, 129, 257, 1000)
FUSE_THRESHOLDS = (0.2, 0.5)


def fuse_batch(max_pool=1024):
    """the mixed-count batch: [(pool rows f32 [P,9], scale, cluster)] for P in FUSE_COUNTS"""
    return [cluster_case(P, 1000 + P) for P in FUSE_COUNTS]


# ------------------------------------------------------------------------------------------------ hand cases
def rect(x0, y0, x1, y1, score):
    return np.array([x0, y0, x1, y0, x1, y1, x0, y1, score], f32)


def hand_cases():
    """name -> (pool f32 [P,9], thr): the cases both test files name"""
    cases = {}
    # A-B-C chain: iou(A,B) = iou(B,C) = 1/3 > 0.2, iou(A,C) = 0.  B is claimed by A, so C is KEPT although B overlaps it
    cases["chain"] = (np.stack([rect(0, 0, 100, 20, 0.9), rect(50, 0, 150, 20, 0.8), rect(100, 0, 200, 20, 0.7)]), 0.2)
    # equal scores resolve by pool order: row 0 keeps and claims row 1; rows 2, 3 the same, one score lower
    cases["ties"] = (np.stack([rect(0, 0, 100, 20, 0.5), rect(2, 0, 102, 20, 0.5), rect(300, 0, 400, 20, 0.25),
                               rect(302, 0, 402, 20, 0.25)]), 0.2)
    # a member stored one corner round votes after its shift
    member = rect(4, 2, 104, 22, 0.5)
    member[:8] = np.roll(member[:8], -2)
    cases["rolled"] = (np.stack([rect(0, 0, 100, 20, 1.0), member]), 0.2)
    # W == 0 leaves the coordinates as they are
    cases["zero_weight"] = (np.stack([rect(0, 0, 100, 20, 0.0), rect(4, 2, 104, 22, 0.0)]), 0.2)
    return cases
