"""GPU: ocr_augment_u8_batch (one inverse-affine warp + colour matrix over a batch, one launch) against a NumPy
restatement of its specification written here — int64 geometry, float32 colour in the stated order — and the augmented
generator end to end.  The arithmetic is integer / exact, so every comparison is torch.equal: no tolerances."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 64), (130, 71)]                    # H, W: offsets 0, 5883, 18171 — unaligned and odd
IDENT = (65536, 0, 0, 0, 65536, 0)
EYE = np.eye(3, 4, dtype=np.float32)


def restate(im, A, col, S):
    """include/ocr_hip.h: ocr_augment_u8_batch for one image uint8 [H,W,3] -> float32 [S,S,3]."""
    H, W, _ = im.shape
    A = [int(a) for a in A]
    dy, dx = np.mgrid[0:S, 0:S].astype(np.int64)
    X16 = A[0] * dx + A[1] * dy + A[2]
    Y16 = A[3] * dx + A[4] * dy + A[5]
    X5, Y5 = (X16 + 1024) >> 11, (Y16 + 1024) >> 11          # numpy's >> on int64 is arithmetic
    sx, fx, sy, fy = X5 >> 5, X5 & 31, Y5 >> 5, Y5 & 31
    v = np.zeros((S, S, 3), np.int64)
    for ox, oy, wgt in ((0, 0, (32 - fx) * (32 - fy)), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy), (1, 1, fx * fy)):
        x, y = sx + ox, sy + oy
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        s = im[np.where(ok, y, 0), np.where(ok, x, 0)].astype(np.int64)
        v += np.where(ok, wgt, 0)[..., None] * s
    p = v.astype(np.float32) * np.float32(1.0 / 1024)
    col = np.asarray(col, np.float32)
    out = np.empty((S, S, 3), np.float32)
    for c in range(3):
        t = ((col[c, 0] * p[..., 0] + col[c, 1] * p[..., 1]) + col[c, 2] * p[..., 2]) + col[c, 3]
        out[..., c] = np.minimum(np.maximum(t, np.float32(0)), np.float32(255))
    assert out.dtype == np.float32
    return out


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(17)
    return [rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]


def run(device, ims, recs, S):
    """recs: one (image index, A, col) per output image; all source images sit back to back in one slab."""
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.datasets.augment import pack_desc
    offs = np.cumsum([0] + [im.size for im in ims])
    slab = np.concatenate([im.reshape(-1) for im in ims])
    desc = pack_desc([int(offs[i]) for i, _, _ in recs], [ims[i].shape for i, _, _ in recs],
                     [(np.array(A, np.int64), col) for _, A, col in recs], slab.size)
    d_slab = torch.from_numpy(slab).to(device)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(device)
    dst = torch.full((len(recs), S, S, 3), -7.0, dtype=torch.float32, device=device)
    ops.augment_u8_batch(d_slab, d_desc, len(recs), S, dst)
    return dst.cpu()


def check(device, ims, recs, S):
    got = run(device, ims, recs, S)
    for b, (i, A, col) in enumerate(recs):
        assert torch.equal(got[b], torch.from_numpy(restate(ims[i], A, col, S))), (b, A)
    return got


def test_identity_is_a_float_copy(device, images):
    got = run(device, images, [(1, IDENT, EYE)], 64)
    assert torch.equal(got[0], torch.from_numpy(images[1].astype(np.float32)))


@pytest.mark.parametrize("S", [64, 40, 37])
def test_integer_crop_and_offset_is_an_exact_copy(device, images, S):
    """Whole-pixel translations: every fraction is 0 and the output is the sub-rectangle itself, zero outside the image.
    S = 40 leaves the last block half empty; S = 37 takes the element-store kernel (rows are not 16-byte aligned)."""
    recs = [(0, (65536, 0, 5 << 16, 0, 65536, 3 << 16), EYE), (1, (65536, 0, 20 << 16, 0, 65536, 24 << 16), EYE),
            (2, (65536, 0, 7 << 16, 0, 65536, 66 << 16), EYE), (2, (65536, 0, -(3 << 16), 0, 65536, -(2 << 16)), EYE)]
    got = check(device, images, recs, S)
    for b, (i, A, _) in enumerate(recs):
        ox, oy = A[2] >> 16, A[5] >> 16
        H, W, _ = images[i].shape
        want = np.zeros((S, S, 3), np.float32)
        ys, xs = np.arange(S) + oy, np.arange(S) + ox
        yk, xk = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        want[np.ix_(yk, xk)] = images[i][np.ix_(ys[yk], xs[xk])]
        assert torch.equal(got[b], torch.from_numpy(want))


@pytest.mark.parametrize("S", [64, 40])
def test_quarter_turns_equal_rot90(device, images, S):
    from tensorflow_ocr_amd.datasets.augment import rot90_fixed
    base = (65536, 0, 4 << 16, 0, 65536, 9 << 16)
    recs = [(2, tuple(int(a) for a in rot90_fixed(base, S, k)), EYE) for k in range(4)]
    got = check(device, images, recs, S)
    for k in range(4):
        assert torch.equal(got[k], torch.from_numpy(np.rot90(got[0].numpy(), k).copy()))
    # by hand, so that the helper is not its own witness: k = 1 is out[dy][dx] = in[dx][S-1-dy]
    assert recs[1][1] == (0, -65536, (4 << 16) + 65536 * (S - 1), 65536, 0, 9 << 16)


@pytest.mark.parametrize("S", [64, 40, 37])
def test_general_matrices_against_the_restatement(device, images, S):
    th = np.deg2rad(17.0)
    c, s = int(round(np.cos(th) * 65536 * 1.3)), int(round(np.sin(th) * 65536 * 1.3))
    sat = np.array([[2.5, -0.9, 0.2, -60.0], [-1.25, 3.0, -0.5, 20.5], [0.1, 0.2, 1.7, -200.0]], np.float32)
    grey = np.array([[0.299, 0.587, 0.114, 0.0]] * 3, np.float32)
    recs = [
        # zoom-out by 3 from (-40, -30): samples beyond all four borders (negative sx / sy, sx = W-1, sy = H-1 and past them)
        (0, (3 << 16, 0, -(40 << 16), 0, 3 << 16, -(30 << 16)), EYE),
        (2, (5 << 16, 0, -(60 << 16) + 777, 0, 5 << 16, -(100 << 16) - 12345), grey),
        # X16 on the rounding tie for every dx (A0 a multiple of 2048, A2 & 2047 == 1024); Y16 one below a tie
        (1, (65536 + 2048, 0, 1024, 0, 65536 - 4096, 1023), EYE),
        (0, (32768, 0, -1024 - 2048 * 40, 0, 32768, -1024), EYE),            # ties at negative coordinates: floor
        # fx = fy = 0 everywhere with a half-pixel-free stride of 2
        (1, (2 << 16, 0, 0, 0, 2 << 16, 1 << 16), EYE),
        # rotation with zoom about an interior point, and a shear
        (2, (c, -s, 20 << 16, s, c, -(10 << 16)), EYE),
        (0, (65536, 21845, -(5 << 16), -9000, 70000, 1 << 16), grey),
        # a colour matrix that saturates at both ends
        (1, (60000, 3000, 12345, -2000, 61000, 54321), sat),
    ]
    assert recs[2][1][2] & 2047 == 1024 and recs[2][1][0] % 2048 == 0
    got = check(device, images, recs, S)
    zoom = got[0].numpy()
    assert (zoom[0] == 0).all() and (zoom[:, 0] == 0).all() and (zoom[-1] == 0).all() and (zoom[:, -1] == 0).all()
    assert zoom.any()
    satd = got[7].numpy()
    assert (satd == 0).any() and (satd == 255).any() and ((satd > 0) & (satd < 255)).any()


def test_single_image_and_a_one_pixel_source(device):
    rng = np.random.default_rng(5)
    one = [np.array([[[200, 17, 90]]], np.uint8)]
    # a 1x1 source: the magnified pixel fades to the zero border over one source pixel on each side
    got = check(device, one, [(0, (4096, 0, -(2 << 16), 0, 4096, -(2 << 16) + 100), EYE)], 64)
    assert got.shape == (1, 64, 64, 3) and got[0].max() == 200
    im = [rng.integers(0, 256, size=(9, 5, 3)).astype(np.uint8)]
    check(device, im, [(0, (20000, 0, -30000, 0, 30000, -70000), EYE)], 40)
    check(device, im, [(0, (20000, 500, -30000, -700, 30000, -70000), EYE)], 1)


def test_invalid_arguments_are_refused(device):
    from ctypes import c_int, c_void_p
    from tensorflow_ocr_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=device)
    p = c_void_p(buf.data_ptr())
    f = lib.ocr_augment_u8_batch
    f.restype = c_int
    for args in ((None, p, 1, 4, p), (p, None, 1, 4, p), (p, p, 1, 4, None), (p, p, 0, 4, p), (p, p, -1, 4, p), (p, p, 1, 0, p)):
        assert f(args[0], args[1], c_int(args[2]), c_int(args[3]), args[4], None) == -1      # OCR_ERR_INVALID_ARG
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- generator, end to end
def _dataset(tmp_path):
    rng = np.random.RandomState(21)
    for i in range(12):
        H, W = int(rng.randint(60, 140)), int(rng.randint(60, 140))
        np.save(os.path.join(tmp_path, "im%02d.npy" % i), rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
        with open(os.path.join(tmp_path, "gt_im%02d.txt" % i), "w") as f:
            for j in range(2):
                x0, y0 = rng.randint(0, W - 30), rng.randint(0, H - 30)
                x1, y1 = x0 + rng.randint(12, 30), y0 + rng.randint(12, 30)
                f.write("%d,%d,%d,%d,%d,%d,%d,%d,%s\n" % (x0, y0, x1, y0, x1, y1, x0, y1, "###" if (i + j) % 5 == 0 else "w"))


def _batches(device, path, count, **kw):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.datasets.augment import Augment
    from tensorflow_ocr_amd.graph import Graph
    aug = Augment.parse("pixellink")
    aug.log = []
    gen = icdar.generator(str(path), input_size=64, batch_size=4, graph=Graph(device), shuffle=True, seed=3, augment=aug, **kw)
    try:
        out = [next(gen) for _ in range(count)]
        torch.cuda.synchronize()
    finally:
        gen.close()
    return out, aug.log


def test_generator_end_to_end(device, tmp_path):
    from tensorflow_ocr_amd.datasets import icdar
    from tensorflow_ocr_amd.graph import Graph
    _dataset(tmp_path)
    S, B, N = 64, 4, 6                                       # six batches: several epochs of the 12 images
    first, log = _batches(device, tmp_path, N)
    again, log2 = _batches(device, tmp_path, N)
    threads, log3 = _batches(device, tmp_path, N, num_workers=2, worker_kind="thread")
    for other, lg in ((again, log2), (threads, log3)):
        for a, b in zip(first, other):
            assert a[1] == b[1]
            for x, y in zip((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4])):
                assert torch.equal(x, y)
        assert len(lg) >= N * B and all(p[0] == q[0] and all(np.array_equal(u, v) for u, v in zip(p[1:], q[1:]))
                                        for p, q in zip(log, lg))
    g = Graph(device)
    backgrounds = 0
    for k, (images, fns, score, geo, mask) in enumerate(first):
        plans = log[k * B:(k + 1) * B]
        assert [p[0] for p in plans] == fns and images.shape == (B, S, S, 3)
        for b, (fn, A, col, polys, tags) in enumerate(plans):
            assert torch.equal(images[b].cpu(), torch.from_numpy(restate(icdar.read_image_rgb(fn), A, col, S)))
            if len(polys) == 0:
                backgrounds += 1
                assert not score[b].any() and bool((mask[b] == 1).all()) and not geo[b].any()
        ws, wg, wm = icdar.generate_rbox_batch((S, S), [p[3] for p in plans], [p[4] for p in plans], graph=g)
        assert torch.equal(score, ws) and torch.equal(geo, wg) and torch.equal(mask, wm)
    assert backgrounds >= 1
    assert len({tuple(p[1].tolist()) for p in log}) > N * B // 2        # the plans do differ from sample to sample
