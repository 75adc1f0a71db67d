"""Not a test: the independent reference of the score-threshold sweep and AP (include/ocr_eval_curve.h).  For every
threshold the detection list is FILTERED and the matcher's reference is RE-RUN on what is left — tests/ic15_ref.py for the
ICDAR-2015 rule, oracle/evalboxes.py for the raster rule — so nothing here uses the prefix property the kernels rest
on; `counts_from_one_matching` is the counting the kernels do, restated, and tests/test_sweep_host.py holds the two
against each other.  AP is a Python sort with the tie rule of the header, in fractions.Fraction.

An image is (dets int32 [k,4,2], scores f32 [k] in ocr_eval_collect's order, gts int32 [g,4,2], flags bool [g])."""
from fractions import Fraction as Fr

import numpy as np

import ic15_ref as R
import test_eval_match_host as H

f32 = np.float32
ABSENT, CARE, MATCHED = 0, 1, 2


def kept_mask(scores, thr):
    """det_score >= threshold in f32: a NaN on either side keeps nothing"""
    with np.errstate(invalid="ignore"):
        return np.asarray(scores, f32) >= f32(thr)


def match_states(rule, dets, gts, flags, matching_threshold=0.5):
    """ONE matching of the whole list -> (state [k] in {ABSENT, CARE, MATCHED}, care ground truths)"""
    dets, gts, flags = np.asarray(dets, np.int32).reshape(-1, 4, 2), np.asarray(gts, np.int32).reshape(-1, 4, 2), np.asarray(flags, bool)
    if rule == "raster":
        n_g, tp, fp = H.oracle_image(dets, gts, flags, matching_threshold)
        return np.where(tp, MATCHED, np.where(fp, CARE, ABSENT)).astype(int), int(n_g)
    r = R.match_image(dets, gts, flags, Fr(matching_threshold))
    state = np.array([MATCHED if m >= 0 else CARE if m == -1 else ABSENT for m in r["det_match"]], int)
    return state, int(r["record"][0])


def row_of(state, care_gt):
    return [int(care_gt), int((state == MATCHED).sum()), int((state == CARE).sum()), int(len(state))]


def rerun_rows(rule, image, thresholds, matching_threshold=0.5):
    """rows [T][4] of one image: the list filtered by each threshold, the matcher's reference run again"""
    dets, scores, gts, flags = image
    rows = []
    for thr in thresholds:
        keep = kept_mask(scores, thr)
        state, care_gt = match_states(rule, np.asarray(dets)[keep], gts, flags, matching_threshold)
        rows.append(row_of(state, care_gt))
    return rows


def counts_from_one_matching(state, scores, care_gt, thresholds):
    """rows [T][4] counted from the states of the full matching — what ocr_eval_*curve_batch does"""
    rows = []
    for thr in thresholds:
        keep = kept_mask(scores, thr)
        rows.append(row_of(np.asarray(state)[keep], care_gt))
    return rows


def sum_rows(per_image):
    return np.asarray(per_image, np.int64).reshape(len(per_image), -1, 4).sum(axis=0)


def is_collect_order(scores):
    """non-increasing with the NaNs last"""
    s = np.asarray(scores, f32)
    for a, b in zip(s[:-1], s[1:]):
        if (np.isnan(a) and not np.isnan(b)) or (not np.isnan(a) and not np.isnan(b) and b > a):
            return False
    return True


def pool_cum(state, scores, max_d):
    """int [max_d][2]: inclusive prefix counts of the care and of the matched detections, NaN-scored ones absent"""
    care, matched = np.zeros(max_d, np.int64), np.zeros(max_d, np.int64)
    ok = ~np.isnan(np.asarray(scores, f32))
    care[:len(state)] = (np.asarray(state) != ABSENT) & ok
    matched[:len(state)] = (np.asarray(state) == MATCHED) & ok
    return np.stack([np.cumsum(care), np.cumsum(matched)], axis=1).astype(np.int32)


def average_precision(pool, care_gt_total):
    """pool: [(state [k], scores [k])] in image-sequence order -> (AP as a Fraction, the number of matched slots).
    A slot is before another when its score is higher, or equal and (image, detection) lexicographically smaller."""
    slots = []
    for i, (state, scores) in enumerate(pool):
        for d, (st, s) in enumerate(zip(state, np.asarray(scores, f32))):
            if st != ABSENT and not np.isnan(s):
                slots.append((-Fr(float(s)), i, d, int(st)))
    slots.sort()
    total, m, c, k = Fr(0), 0, 0, 0
    for _, _, _, st in slots:
        c += 1
        if st == MATCHED:
            m += 1
            k += 1
            total += Fr(m, c)
    return (total / care_gt_total if care_gt_total > 0 else Fr(0)), k


# ------------------------------------------------------------------------------------------------ random images (host test)
def random_image(rng, rule):
    """a 64 x 64 canvas: 0..4 ground truths (some don't-care), detections crowded on them — several compete for one
    ground truth — plus strays; now and then no ground truth or no detection at all; scores with ties, sometimes a NaN"""
    n_g = int(rng.integers(0, 5)) if rng.uniform() > 0.1 else 0
    n_d = int(rng.integers(1, 10)) if rng.uniform() > 0.1 else 0
    gts = np.zeros((n_g, 4, 2), np.int32)
    for g in range(n_g):
        x0, y0 = rng.integers(2, 40, 2)
        gts[g] = H.rect(x0, y0, x0 + rng.integers(6, 20), y0 + rng.integers(4, 16))
    flags = rng.integers(0, 3, n_g) == 0
    dets = np.zeros((n_d, 4, 2), np.int32)
    for d in range(n_d):
        if n_g and rng.uniform() < 0.75:
            dets[d] = gts[rng.integers(0, n_g)] + rng.integers(-2, 3, (4, 2))          # near a ground truth, often the same one
        else:
            x0, y0 = rng.integers(2, 50, 2)
            dets[d] = H.rect(x0, y0, x0 + rng.integers(3, 12), y0 + rng.integers(3, 10))
    dets = np.clip(dets, 0, 63).astype(np.int32)
    scores = np.sort(rng.choice(np.arange(1, 13, dtype=f32) / f32(8), n_d))[::-1].copy()
    if n_d and rng.uniform() < 0.15:
        scores[-1] = np.nan
    return dets, scores.astype(f32), gts, flags


# ------------------------------------------------------------------------------------------------ the GPU fixture
N, MAX_D, MAX_G, T = 3, 70, 5, 6
# below every score, NaN, equal to a score, above every score, two in between given out of order
THRESHOLDS = [0.0, float("nan"), 1.5, 100.0, 2.0625, 0.6875]


def gpu_images():
    """The 3 images of tests/test_gpu_eval_sweep.py, built from ic15_ref.jittered_cases(3) (whose every pair is further
    than 1e-6 from the matcher's thresholds; repeating or leaving out polygons changes no pair):
      'crowd'  66 detections (the 16 of the first jittered image, repeated: copies compete for one ground truth; index 64
               and 65 sit beyond a wave) on its first 5 ground truths, a don't-care one among them; scores with ties
               inside the image, the last one NaN
      'no_gt'  the third image's 12 detections and no ground truth; some of its scores equal scores of 'crowd'
      'no_det' no detection, 3 ground truths"""
    (d16, g8, c8), _, (d12, g3, c3) = R.jittered_cases(3)
    g5, c5 = g8[:5], c8[:5]
    crowd = np.concatenate([d16] * 4 + [d16[:2]])
    s = np.repeat(np.arange(22, 0, -1, dtype=f32) / f32(8), 3)          # 2.75 .. 0.125, each three times: ties inside the image
    s[-1] = np.nan
    s12 = (np.array([24, 22, 22, 17, 12, 12, 9, 9, 6, 5, 3, 1], f32) / f32(8)).astype(f32)     # 2.75 and 1.5 occur in both
    return {"crowd": (crowd, s, g5, c5), "no_gt": (d12, s12, np.zeros((0, 4, 2), np.int32), np.zeros(0, bool)),
            "no_det": (np.zeros((0, 4, 2), np.int32), np.zeros(0, f32), g3, c3)}


ORDERS = (("no_gt", "crowd", "no_det"), ("crowd", "no_det", "no_gt"))
