"""Synthetic training batches of the shape the reference's icdar generator feeds
(multigpu_train.py:164-174: images [N,S,S,3] 0..255, score map [N,S/4,S/4,1], 8 link maps,
training mask), per SURVEY.md §8d: pixel label = union of random axis-aligned rectangles at 1/4
resolution, link label = 1 where the neighbour in that direction shares the rectangle (border = 1;
direction order left, left_down, left_up, right, right_down, right_up, up, down), mask = 1."""
import numpy as np


def make_batch(rng, n, size, rects=8, return_ids=False):
    """return_ids=True adds a fifth value, the int32 [n, size/4, size/4] map of rectangle numbers (0: background, k + 1:
    rectangle k, later ones on top) the labels were made from: the instances of the instance-balanced loss."""
    q4 = size // 4
    images = rng.uniform(0, 255, size=(n, size, size, 3)).astype(np.float32)
    ids = np.zeros((n, q4, q4), np.int32)
    for b in range(n):
        for k in range(rects):
            hh = int(rng.integers(max(2, q4 // 16), max(3, q4 * 3 // 8)))
            ww = int(rng.integers(max(2, q4 // 16), max(3, q4 * 3 // 8)))
            y0 = int(rng.integers(0, q4 - hh + 1))
            x0 = int(rng.integers(0, q4 - ww + 1))
            ids[b, y0:y0 + hh, x0:x0 + ww] = k + 1
    pixel = (ids > 0).astype(np.float32)[..., None]
    offs = [(-1, 0), (-1, 1), (-1, -1), (1, 0), (1, 1), (1, -1), (0, -1), (0, 1)]   # (dx, dy)
    link = np.zeros((n, q4, q4, 8), np.float32)
    pad = np.pad(ids, ((0, 0), (1, 1), (1, 1)), constant_values=-1)
    for d, (dx, dy) in enumerate(offs):
        nb = pad[:, 1 + dy:1 + dy + q4, 1 + dx:1 + dx + q4]
        link[..., d] = ((ids > 0) & ((nb == ids) | (nb == -1))).astype(np.float32)
    mask = np.ones((n, q4, q4, 1), np.float32)
    if return_ids:
        return images, pixel, link, mask, ids
    return images, pixel, link, mask


def rbox_labels(n, size, rng, rects=3):
    """EAST RBOX label maps at 1/4 resolution for tests and smoke training (NOT labels from ICDAR polygons: those
    are datasets/icdar.generate_rbox_batch(geometry='RBOX'), in the same convention): per image `rects` random rotated rectangles, later ones on top.  Returns
    (score [n,q,q,1], geo [n,q,q,5], mask [n,q,q,1]) float32 with q = size // 4: inside a rectangle score = 1 and geo =
    (distance to its top, right, bottom, left edge in IMAGE pixels, its angle in (-pi/4, pi/4)), zeros outside; mask = 1.
    Map cell (x, y) stands for image point (4x, 4y); the rectangle's right-pointing axis is (cos a, -sin a) with y down,
    the convention tool/rbox.decode inverts."""
    q4 = size // 4
    score = np.zeros((n, q4, q4, 1), np.float32)
    geo = np.zeros((n, q4, q4, 5), np.float32)
    ys, xs = np.mgrid[0:q4, 0:q4]
    px, py = 4.0 * xs, 4.0 * ys
    for b in range(n):
        for _ in range(rects):
            a = float(rng.uniform(-0.7, 0.7))                                    # inside (-pi/4, pi/4)
            half_w, half_h = float(rng.uniform(size / 10.0, size / 3.2)), float(rng.uniform(size / 20.0, size / 8.0))
            cx, cy = float(rng.uniform(0.25 * size, 0.75 * size)), float(rng.uniform(0.25 * size, 0.75 * size))
            c, s = np.cos(a), np.sin(a)
            lx = (px - cx) * c - (py - cy) * s                                   # along the right-pointing axis
            ly = (px - cx) * s + (py - cy) * c                                   # along the down-pointing axis
            inside = (np.abs(lx) <= half_w) & (np.abs(ly) <= half_h)
            d = np.stack([ly + half_h, half_w - lx, half_h - ly, lx + half_w, np.full_like(lx, a)], axis=-1)
            score[b, inside, 0] = 1.0
            geo[b, inside] = d[inside].astype(np.float32)
    return score, geo, np.ones((n, q4, q4, 1), np.float32)
