"""GPU: RBOX training labels from ICDAR polygons (csrc/labels.hip ocr_icdar_rbox_labels, datasets/icdar.generate_rbox_batch(geometry=
'RBOX'), the generator, multigpu_train.build_forward_loss) and the post-NMS mean-score filter (csrc/rbox.hip
ocr_quad_mean_score, tool/rbox.detect(box_thresh=...)).

References are NumPy restatements written here on oracle.cvgeom.fill_poly (OpenCV's raster restated in C): polygons
drawn one after another, later ones on top; distances as the reference's point_dist_to_line in float64 from the
rectangle datasets/rbox_labels.fit_rectangle returns (its own properties: tests/test_rbox_labels_host.py).

Bounds (from the number formats, none from what the kernels give):
  score, mask     bit for bit
  distances       2e-3 px: about five f32 roundings (two products, two sums, the f32 line) at magnitude <= 2^12, half an
                  ulp (2.4e-4) each
  angle           the float32 angle, exactly; everything exactly 0 outside the score raster
  round trip      5e-2 px: labels and decode each add f32 sin / cos and distance error at coordinates <= 128
  mean score      1e-6 relative (f64 sums, one f32 rounding of the quotient); empty rasters exactly 0

Measured on the MI355X: distances at most 1.3e-5 px from float64 (bound 2e-3); round trip at most 1.5e-5 px (bound 5e-2);
mean score at most 5.4e-8 relative (bound 1e-6).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import cvgeom as C
from oracle import lanms as OL
from tensorflow_ocr_amd.datasets import rbox_labels as RL

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENT = -12345.5


def _rot_rect(cx, cy, W, H, a):
    u, v = np.array([math.cos(a), -math.sin(a)]), np.array([math.sin(a), math.cos(a)])
    c = np.array([cx, cy], f64)
    return np.array([c - W / 2 * u - H / 2 * v, c + W / 2 * u - H / 2 * v, c + W / 2 * u + H / 2 * v, c - W / 2 * u + H / 2 * v])


def _polys(rng, k, h, w):
    """k float32 quadrangles: perturbed rotated rectangles, then by position: [1] overlaps [0], [2] is below min_text_size,
    [3] is degenerate (a repeated vertex; its full raster is a triangle), tag [4] is set"""
    out = []
    for _ in range(k):
        W, H = rng.uniform(18, w / 2.5), rng.uniform(11, h / 5)
        q = _rot_rect(rng.uniform(12, w - 12), rng.uniform(12, h - 12), W, H, rng.uniform(-0.7, 0.7))
        out.append(q + rng.uniform(-1, 1, (4, 2)) * 0.1 * min(W, H))
    out = np.array(out)
    out[1] = out[0] + [7.3, 4.1]
    out[2] = _rot_rect(w * 0.5, h * 0.3, 14, 6, 0.2)
    out[3] = [[5.2, 6.1], [31.7, 5.5], [31.7, 5.5], [6.4, 29.9]]
    tags = np.zeros(k, bool)
    tags[4] = True
    return np.clip(out, -4, max(h, w) + 4).astype(f32), tags


def _dist(p1, p2, x, y):
    """the reference's point_dist_to_line (datasets/icdar.py:269-271) for grids x, y, float64"""
    d = p2 - p1
    return np.abs(d[0] * (p1[1] - y) - d[1] * (p1[0] - x)) / np.hypot(d[0], d[1])


def _ref_maps(h, w, polys, tags, step, shrink, min_text_size=10):
    owner, mask = np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)
    fits = []
    for i, (poly, tag) in enumerate(zip(polys, tags)):
        fit = RL.fit_rectangle(poly)
        fits.append(fit)
        full = poly.astype(np.int32)
        poly_h = min(np.linalg.norm(poly[0] - poly[3]), np.linalg.norm(poly[1] - poly[2]))
        poly_w = min(np.linalg.norm(poly[0] - poly[1]), np.linalg.norm(poly[2] - poly[3]))
        if tag or min(poly_h, poly_w) < min_text_size or fit is None:
            C.fill_poly(mask, full, 0)
        if fit is not None:
            C.fill_poly(owner, RL.shrink_poly(poly, RL.shrink_radii(poly), shrink).astype(np.int32) if shrink else full, i + 1)
    ys, xs = np.mgrid[0:h, 0:w].astype(f64)
    geo = np.zeros((h, w, 5), f64)
    for i, fit in enumerate(fits):
        if fit is None:
            assert not (owner == i + 1).any()
            continue
        r, sel = fit[0].astype(f64), owner == i + 1
        for k in range(4):
            geo[sel, k] = _dist(r[k], r[(k + 1) % 4], xs, ys)[sel]
        geo[sel, 4] = f32(fit[1])
    s = (slice(None, None, step), slice(None, None, step))
    return (owner > 0).astype(f32)[s][..., None], geo[s], mask.astype(f32)[s][..., None], owner[s], fits


@pytest.mark.parametrize("step", [1, 4])
@pytest.mark.parametrize("h,w,k,seed", [(64, 64, 5, 0), (128, 96, 12, 1)])
def test_maps_against_float64(device, h, w, k, seed, step):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device)
    rng = np.random.default_rng(seed)
    p0, t0 = _polys(rng, k, h, w)
    p1, t1 = _polys(rng, 5, h, w)                                   # fewer polygons than the table has rows
    polys_l, tags_l = [p0, p1, np.zeros((0, 4, 2), f32)], [t0, t1, np.zeros(0, bool)]
    score, geo, mask = icdar.generate_rbox_batch((h, w), polys_l, tags_l, step=step, graph=g, geometry='RBOX')
    oh, ow = -(-h // step), -(-w // step)
    assert score.shape == (3, oh, ow, 1) and geo.shape == (3, oh, ow, 5) and mask.shape == (3, oh, ow, 1)
    score, geo, mask = score.cpu().numpy(), geo.cpu().numpy(), mask.cpu().numpy()
    worst = 0.0
    for b in range(3):
        rs, rg, rm, owner, fits = _ref_maps(h, w, polys_l[b], tags_l[b], step, 0.3)
        assert np.array_equal(score[b], rs) and np.array_equal(mask[b], rm)
        on = rs[..., 0] > 0
        if b < 2:
            assert fits[3] is None and on.any() and (~on).any() and (rm == 0).any()
            assert len(set(owner[on].tolist())) >= 2                        # more than one polygon owns cells
        err = np.abs(geo[b][..., :4].astype(f64) - rg[..., :4])
        worst = max(worst, float(err.max()))
        assert (err <= 2e-3).all()
        assert np.array_equal(geo[b][..., 4].view(np.int32), rg[..., 4].astype(f32).view(np.int32))
        assert (geo[b][~on].view(np.int32) == 0).all()
    print("rbox labels %dx%d step %d: largest distance error %.3e px (bound 2e-3)" % (h, w, step, worst))
    assert (score[2] == 0).all() and (geo[2] == 0).all() and (mask[2] == 1).all()


def _round_trip_rects(rng, size, want):
    """Rotated rectangles (float64 corners) every sampled raster cell of which lies INSIDE the rectangle.  The labels hold
    unsigned distances, as EAST's do, so a raster cell outside the rectangle (fillPoly's outline reaches half a pixel
    beyond an edge, the int32 cast moves vertices) has no quad that decodes back: such rectangles are not candidates.
    The raster is the oracle's, the inside test float64: nothing here looks at the code under test."""
    out = []
    for _ in range(400):
        if len(out) == want:
            break
        W, H = rng.uniform(20, 60), rng.uniform(12, 40)
        q = _rot_rect(rng.uniform(30, size - 30), rng.uniform(30, size - 30), W, H, rng.uniform(-0.78, 0.78))
        if q.min() < 1 or q.max() > size - 2:
            continue
        m = np.zeros((size, size), np.uint8)
        C.fill_poly(m, q.astype(f32).astype(np.int32), 1)
        ys, xs = np.nonzero(m[::4, ::4])
        fit = RL.fit_rectangle(q.astype(f32))
        r = fit[0].astype(f64)
        c = r.mean(axis=0)
        inside = True
        for k in range(4):
            d = r[(k + 1) % 4] - r[k]
            side = lambda x, y: d[0] * (y - r[k][1]) - d[1] * (x - r[k][0])
            inside &= bool((side(4.0 * xs, 4.0 * ys) * np.sign(side(*c)) > 1e-3).all())
        if inside and len(xs) >= 4:
            out.append(q.astype(f32))
    assert len(out) == want
    return out


def test_round_trip_labels_decode_to_the_fitted_rectangles(device):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import rbox
    g = Graph(device)
    rng = np.random.default_rng(7)
    size = 128
    polys_l = [np.array(_round_trip_rects(rng, size, 4)) for _ in range(2)]
    tags_l = [np.zeros(4, bool)] * 2
    score, geo, mask = icdar.generate_rbox_batch((size, size), polys_l, tags_l, graph=g, geometry='RBOX', shrink=0)
    boxes, counts, total = rbox.decode(score, geo, score_map_thresh=0.5, graph=g)
    boxes, counts = boxes.cpu().numpy(), counts.cpu().numpy()
    worst, angles = 0.0, []
    for b in range(2):
        rs, _, _, owner, fits = _ref_maps(size, size, polys_l[b], tags_l[b], 4, 0)
        own = owner[rs[..., 0] > 0]                                   # raster order, as the decode
        assert counts[b] == len(own) > 20
        want = np.array([fits[o - 1][0].astype(f64).reshape(8) for o in own])
        err = np.abs(boxes[b, :counts[b], :8].astype(f64) - want)
        worst = max(worst, float(err.max()))
        angles += [f[1] for f in fits]
        assert (err <= 5e-2).all(), float(err.max())                  # measured: 1.5e-5 px
    print("rbox round trip: largest corner deviation %.3e px (bound 5e-2)" % worst)
    assert min(angles) < -0.1 and max(angles) > 0.1                   # both branches of the decode


def test_link_path_is_untouched(device):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device)
    rng = np.random.default_rng(3)
    polys_l, tags_l = zip(*[_polys(rng, 6, 64, 64) for _ in range(2)])
    a = icdar.generate_rbox_batch((64, 64), list(polys_l), list(tags_l), graph=g)
    b = icdar.generate_rbox_batch((64, 64), list(polys_l), list(tags_l), graph=g, geometry='link')
    assert a[1].shape == (2, 16, 16, 8) and all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="square"):
        icdar.generate_rbox_batch((64, 48), list(polys_l), list(tags_l), graph=g)
    with pytest.raises(ValueError, match="geometry"):
        icdar.generate_rbox_batch((64, 64), list(polys_l), list(tags_l), graph=g, geometry='QUAD')


def _dataset(tmp_path, rng, count):
    for i in range(count):
        H, W = int(rng.integers(60, 140)), int(rng.integers(60, 140))
        np.save(os.path.join(tmp_path, "im%02d.npy" % i), rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
        with open(os.path.join(tmp_path, "gt_im%02d.txt" % i), "w") as f:
            for j in range(3):
                q = _rot_rect(rng.uniform(25, W - 25), rng.uniform(20, H - 20), rng.uniform(20, 45), rng.uniform(12, 22),
                              rng.uniform(-0.6, 0.6))
                f.write(",".join("%d" % v for v in np.clip(q, 0, min(H, W) - 1).ravel()) + (",###\n" if j == 2 else ",w\n"))


def test_generator_and_feeder_yield_rbox_maps(device, tmp_path):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device)
    S, B = 64, 4
    _dataset(tmp_path, np.random.default_rng(11), 8)
    direct = icdar.generator(str(tmp_path), input_size=S, batch_size=B, graph=g, shuffle=True, seed=5, geometry='RBOX')
    feeder = icdar.get_batch(num_workers=0, training_data_path=str(tmp_path), input_size=S, batch_size=B, graph=g,
                             shuffle=True, seed=5, geometry='RBOX')
    try:
        for _ in range(3):                                            # crosses an epoch boundary
            a, b = next(direct), next(feeder)
            q = S // 4
            assert a[0].shape == (B, S, S, 3) and a[2].shape == (B, q, q, 1) and a[3].shape == (B, q, q, 5) and \
                a[4].shape == (B, q, q, 1)
            assert a[1] == b[1]
            for x, y in zip((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4])):
                assert x.dtype == torch.float32 and torch.equal(x, y)
            assert a[2].sum() > 0 and (a[4] == 0).any() and (a[3][..., :4].amax() > 4)
    finally:
        feeder.close()


def test_one_rbox_training_step_on_a_generator_batch(device, tmp_path):
    import multigpu_train as T
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=1)
    _dataset(tmp_path, np.random.default_rng(12), 2)
    images, _, score, geo, mask = next(icdar.generator(str(tmp_path), input_size=128, batch_size=2, graph=g, shuffle=False,
                                                       geometry='RBOX'))
    assert geo.shape == (2, 32, 32, 5) and score.sum() > 0
    step = TrainStep(g, T.build_forward_loss('east', geometry='RBOX'), lambda gr: AdamOptimizer(gr, learning_rate=1e-3))
    first = step(images, score, geo, mask).item()
    second = step(images, score, geo, mask).item()
    assert math.isfinite(first) and math.isfinite(second) and first != second      # the weights moved
    assert any("Conv_9" in k for k in g.store.order)                               # the RBOX heads, not the link heads


# ------------------------------------------------------------------------------------------------ mean score
def _ref_means(quads, score):
    h, w = score.shape
    out = []
    for q in quads:
        m = np.zeros((h, w), np.uint8)
        C.fill_poly(m, q.reshape(4, 2).astype(np.int32) // 4, 1)
        out.append(score[m > 0].astype(f64).mean() if m.any() else 0.0)
    return np.array(out)


def test_quad_mean_score_against_the_fillpoly_raster(device):
    from tensorflow_ocr_amd import ops
    rng = np.random.default_rng(5)
    score = rng.uniform(0, 1, (64, 64)).astype(f32)
    quads = np.array([
        [40.5, 30.2, 180.9, 52.7, 170.1, 120.3, 30.6, 99.9],            # fully inside (map cells 7..45)
        [-37.7, -21.3, 90.2, -9.9, 95.5, 60.1, -30.4, 55.5],            # partly outside: negative coordinates truncate, then floor
        [200.3, 180.8, 300.6, 190.2, 290.1, 280.7, 190.9, 270.4],       # crosses the right and bottom border (map is 256 px)
        [300.5, 20.5, 400.5, 20.5, 400.5, 90.5, 300.5, 90.5],           # fully outside
        [-90.0, -50.0, -10.0, -50.0, -10.0, -8.0, -90.0, -8.0],         # fully outside, negative
        [20.0, 200.0, 120.0, 230.0, 120.0, 230.0, 20.0, 200.0],         # collapsed to a line: the outline is its raster
        [100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0],       # a point
        [0.0, 0.0, 255.9, 0.0, 255.9, 255.9, 0.0, 255.9],               # the whole map: 4096 cells, every thread adds 16
    ], f32)
    ref = _ref_means(quads, score)
    assert ref[3] == 0 and ref[4] == 0 and (ref[[0, 1, 2, 5, 6, 7]] > 0).all()
    assert ref[6] == f64(score[25, 25]) and abs(ref[7] - score.astype(f64).mean()) < 1e-12
    pad = torch.full((len(quads) + 64,), SENT, device=device)
    ops.quad_mean_score(torch.from_numpy(quads).to(device), torch.from_numpy(score).to(device), 0.25, pad[:len(quads)])
    got = pad.cpu().numpy()
    assert (got[len(quads):] == f32(SENT)).all()
    got = got[:len(quads)].astype(f64)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("quad mean score: largest relative error %.3e (bound 1e-6)" % float(rel[ref > 0].max()))
    assert (got[ref == 0] == 0).all() and (rel[ref > 0] <= 1e-6).all(), (got, ref)
    # a non-finite coordinate: an empty raster
    bad = quads[:2].copy()
    bad[0, 3] = np.nan
    bad[1, 0] = np.inf
    out = torch.full((2,), SENT, device=device)
    ops.quad_mean_score(torch.from_numpy(bad).to(device), torch.from_numpy(score).to(device), 0.25, out)
    assert out.tolist() == [0.0, 0.0]


def test_detect_box_thresh_filters_on_the_reference_means(device):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import rbox
    g = Graph(device)
    rng = np.random.default_rng(31)
    label, geo, _ = synthetic.rbox_labels(2, 256, rng)                   # 64 x 64 maps
    score = (label[..., 0] * rng.uniform(0.85, 1.0, label.shape[:3])).astype(f32)
    ys, xs = np.mgrid[0:64, 0:64]
    score[1] = np.where((xs + ys) % 3 == 0, score[1], score[1] * f32(0.1))      # image 1: two cells of three are faint
    geo = geo.copy()
    geo[..., :4] += (label * rng.uniform(-1.5, 1.5, geo[..., :4].shape)).astype(f32)
    geo[..., 4] += (label[..., 0] * rng.uniform(-0.02, 0.02, label.shape[:3])).astype(f32)
    boxes, counts, _ = rbox.decode(score, geo, graph=g)
    boxes, counts = boxes.cpu().numpy(), counts.cpu().numpy()
    plain = rbox.detect(score, geo, graph=g)
    none = rbox.detect(score, geo, graph=g, box_thresh=None)
    kept = rbox.detect(score, geo, graph=g, box_thresh=0.5)
    n_in = n_out = 0
    for i in range(2):
        om, ok = OL.lanms(boxes[i, :counts[i]], 0.2)                      # today's output: the oracle on the decoded quads
        assert np.array_equal(plain[i].view(np.int32), om[ok].view(np.int32))
        assert np.array_equal(none[i].view(np.int32), plain[i].view(np.int32))
        ref = _ref_means(plain[i][:, :8], score[i])
        assert (np.abs(ref - 0.5) > 1e-3).all()
        want = plain[i][ref > 0.5]
        assert np.array_equal(kept[i].view(np.int32), want.view(np.int32))
        n_in, n_out = n_in + len(want), n_out + len(plain[i]) - len(want)
    assert n_in > 0 and n_out > 0


def test_bad_arguments_return_unsupported_without_a_launch(device):
    from tensorflow_ocr_amd import _lib as L
    p, ci = L.ptr, ctypes.c_int
    cover = torch.zeros((1, 8, 8), dtype=torch.int32, device=device)
    rects = torch.zeros((1, 255, 5, 3), device=device)
    o_score, o_geo, o_mask = (torch.full((1, 8, 8, c), SENT, device=device) for c in (1, 5, 1))
    fn = L._fn("ocr_icdar_rbox_labels", ctypes.c_int)

    def labels(n=1, P=1, h=8, w=8, step=1, cs=cover):
        return fn(p(cs), p(cover), p(rects), ci(n), ci(P), ci(h), ci(w), ci(step), p(o_score), p(o_geo), p(o_mask),
                  L.stream_ptr())
    assert labels(step=0) == -2 and labels(P=255) == -2 and labels(P=0) == -2
    assert labels(n=0) == -2 and labels(h=0) == -2 and labels(w=-1) == -2
    assert labels(cs=None) == -1
    fm = L._fn("ocr_quad_mean_score", ctypes.c_int)
    quads = torch.zeros((2, 8), device=device)
    score = torch.zeros((8, 8), device=device)
    mean = torch.full((2,), SENT, device=device)

    def means(k=2, h=8, w=8, inv=0.25):
        return fm(p(quads), ci(k), p(score), ci(h), ci(w), ctypes.c_float(inv), p(mean), L.stream_ptr())
    assert means(k=-1) == -2 and means(h=0) == -2 and means(w=0) == -2 and means(inv=0.0) == -2
    assert means(k=0) == 0
    torch.cuda.synchronize()
    assert all((t == SENT).all() for t in (o_score, o_geo, o_mask, mean))          # nothing was written
    assert means() == 0 and labels() == 0                                # the same calls with good arguments run
    torch.cuda.synchronize()
    assert mean.tolist() == [0.0, 0.0] and (o_score == 0).all() and (o_geo == 0).all() and (o_mask == 1).all()
