"""GPU: the link decode over a threshold grid (csrc/decode_grid.hip, include/ocr_decode_grid.h) against two references that
are not the code under test — a loop of the existing ocr_link_cc / ocr_component_scores, one call per grid point, and
oracle.ocr_oracle.link_cc_union on the CPU.  labels, ncomp and the written rows of comps are bit-equal for every slice
b = g * n + i; rows of comps at or beyond min(ncomp, max_comps) keep the fill.

Kernel inventory of decode_grid.hip (tests/test_decode_grid_host.py holds this list to the file):

  ocr_link_cc_grid, ocr_link_cc_grid_workspace
    ccg_init_kernel          one score read decides all G slices           every row (the point with no pixel: 2.0)
    ccg_union_tile_kernel    <false> LDS tiles, <true> tile-border edges   33x31 / 33x65 / 67x70 (2, 3 and 9 tiles), the
                                                                           serpentine and corner_* generators of the decode
                                                                           matrix at two link thresholds
    ccg_root_kernel          roots and sizes                               every row
    ccg_count_kernel, ccg_assign_kernel                                    67x70 (five 1024-pixel blocks), max_comps below
                                                                           the count at one point only
    ccg_relabel_kernel                                                     every row
  ocr_component_scores_grid, ocr_component_scores_grid_workspace
    csg_accum_kernel, csg_mean_kernel                                      an id beyond max_comps, a slice without components

Maps are drawn from {0, .25, .5, .75, 1, NaN, -1}, so the grid thresholds {.25, .5, 2} x {.25, .75} EQUAL map values and the
strict comparison shows: a pixel at 0.5 is out at 0.5 and in at 0.25, NaN is never in.  Points that differ only in the link
threshold nest their partitions (checked)."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_decode_matrix as M
from matrix_support import FL, INVALID_ARG, OK, SZ, UNSUPPORTED, WORKSPACE, Guard, _lib, _rc, _rng, f32
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu
I32, U8, F32 = torch.int32, torch.uint8, torch.float32
VALUES = np.array([0, 0.25, 0.5, 0.75, 1, np.nan, -1], f32)
PIXEL_T, LINK_T = (0.25, 0.5, 2.0), (0.25, 0.75)
POINTS = [(p, l) for p in PIXEL_T for l in LINK_T]          # G = 6, pixel-major
SHAPES = [(3, 3), (33, 31), (33, 65), (67, 70)]
N = 3


def maps_of(h, w):
    """score [N,h,w], link [8,N,h,w] from the value set; image 1 leans towards text so that some point links nearly all"""
    rng = _rng("decode_grid", "maps", h, w)
    score = VALUES[rng.integers(len(VALUES), size=(N, h, w))]
    link = VALUES[rng.integers(len(VALUES), size=(8, N, h, w))]
    score[1] = np.where(rng.uniform(size=(h, w)) < 0.7, f32(1), score[1])
    link[:, 1] = np.where(rng.uniform(size=(8, h, w)) < 0.7, f32(1), link[:, 1])
    return score, link


_ORACLE = {}


def oracle_of(h, w, min_size):
    """O.link_cc_union of every (point, image), computed once per shape and min_size: [G][N] of (labels, comps)"""
    key = (h, w, min_size)
    if key not in _ORACLE:
        score, link = maps_of(h, w)
        with np.errstate(invalid="ignore"):
            _ORACLE[key] = [[O.link_cc_union(score[i], link[:, i], f32(tp), f32(tl), min_size) for i in range(N)]
                            for tp, tl in POINTS]
    return _ORACLE[key]


def _link_operand(link, layout, device):
    if layout == 1:
        return M._f32(link, device), 1, 0
    with np.errstate(invalid="ignore"):                     # channel 1 of [8][n][h][w][2]; channel 0 would change the answer
        two = np.stack([np.where(np.isnan(link), f32(1), f32(0.6) - link).astype(f32), link], -1)
    return M._f32(two, device), 2, 1


def run_grid(L, device, score, link, points, min_size, max_comps, layout):
    """one raw call of ocr_link_cc_grid -> (labels [G*n,h,w], ncomp [G*n], [written comps rows per slice])"""
    n, h, w = score.shape
    G = len(points)
    lk, stride, off = _link_operand(link, layout, device)
    lab, nc, cp = M._cc_outputs(G * n, h, w, max_comps, device)
    nbytes = M._size(L, "ocr_link_cc_grid_workspace", G, n, h, w)
    assert nbytes == G * M._size(L, "ocr_link_cc_workspace", n, h, w)
    ws = M._ws(nbytes, device)
    tp, tl = (FL * G)(*[p for p, _ in points]), (FL * G)(*[l for _, l in points])
    rc = _rc(L, "ocr_link_cc_grid", M._f32(score, device), lk, stride, off, n, h, w, G, tp, tl, min_size, lab, nc, cp, max_comps,
             ws, SZ(nbytes))
    assert rc == OK
    return M._cc_read(lab, nc, cp, ws, max_comps)


def run_loop(L, device, score, link, points, min_size, max_comps, layout):
    """the same from the existing entry: one ocr_link_cc call per grid point"""
    labels, ncomp, comps = [], [], []
    lk, stride, off = _link_operand(link, layout, device)
    n, h, w = score.shape
    sc = M._f32(score, device)
    for tp, tl in points:
        lab, nc, cp = M._cc_outputs(n, h, w, max_comps, device)
        nbytes = M._size(L, "ocr_link_cc_workspace", n, h, w)
        ws = M._ws(nbytes, device)
        assert _rc(L, "ocr_link_cc", sc, lk, stride, off, n, h, w, FL(tp), FL(tl), min_size, lab, nc, cp, max_comps, ws,
                   SZ(nbytes)) == OK
        a, b, c = M._cc_read(lab, nc, cp, ws, max_comps)
        labels.append(a)
        ncomp.append(b)
        comps += c
    return np.concatenate(labels), np.concatenate(ncomp), comps


def _same_slices(got, want, what):
    glab, gn, gcomps = got
    wlab, wn, wcomps = want
    assert np.array_equal(gn, wn), "%s: ncomp %s, reference %s" % (what, gn.tolist(), wn.tolist())
    assert np.array_equal(glab, wlab), "%s: %d labels differ" % (what, int((glab != wlab).sum()))
    assert len(gcomps) == len(wcomps)
    for b, (a, c) in enumerate(zip(gcomps, wcomps)):
        assert np.array_equal(a, c), "%s: the component table of slice %d differs" % (what, b)


# ------------------------------------------------------------------------------------------------ ocr_link_cc_grid
@pytest.mark.parametrize("min_size", [0, 5])
@pytest.mark.parametrize("layout", [1, 2], ids=["stride1", "stride2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_grid_equals_the_loop_and_the_oracle(device, shape, layout, min_size):
    L, _ = _lib()
    h, w = shape
    score, link = maps_of(h, w)
    max_comps = h * w
    got = run_grid(L, device, score, link, POINTS, min_size, max_comps, layout)
    _same_slices(got, run_loop(L, device, score, link, POINTS, min_size, max_comps, layout), "grid vs loop %s" % (shape,))
    ref = oracle_of(h, w, min_size)
    for g in range(len(POINTS)):
        for i in range(N):
            labels, comps = ref[g][i]
            b = g * N + i
            M._same_cc((got[0][b], got[1][b], got[2][b]), labels, comps, max_comps, "point %d image %d" % (g, i))
    # what the grid was chosen for
    glab, gn, _ = got
    assert not gn[4 * N:].any() and not glab[4 * N:].any()                  # pixel > 2.0: no pixel at either link threshold
    for g in (0, 2):                                                        # (p, 0.25) and (p, 0.75): the partitions nest
        lo_t, hi_t = glab[g * N:(g + 1) * N], glab[(g + 1) * N:(g + 2) * N]
        if min_size == 0:
            assert np.array_equal(lo_t > 0, hi_t > 0)
            pairs = set(zip(hi_t[hi_t > 0].tolist(), lo_t[hi_t > 0].tolist(), np.nonzero(hi_t > 0)[0].tolist()))
            assert len({(i, a) for a, _, i in pairs}) == len({(i, a, b) for a, b, i in pairs})       # a fine id lies in one coarse id
            assert (gn[g * N:(g + 1) * N] <= gn[(g + 1) * N:(g + 2) * N]).all()
    if shape == (67, 70) and min_size == 0:
        with np.errstate(invalid="ignore"):
            inside = int((score[1] > 0.25).sum())
        assert max(c[1] for c in ref[0][1][1]) > 0.9 * inside               # image 1 at (0.25, 0.25): nearly all pixels in one component


def test_max_comps_below_the_count_at_one_point_only(device):
    L, _ = _lib()
    h, w = 33, 31
    score, link = maps_of(h, w)
    ref = oracle_of(h, w, 0)
    counts = np.array([[len(ref[g][i][1]) for i in range(N)] for g in range(len(POINTS))])
    worst = np.sort(counts.max(axis=1))
    max_comps = int(worst[-2])
    assert worst[-1] > max_comps >= 1 and int((counts.max(axis=1) > max_comps).sum()) == 1
    got = run_grid(L, device, score, link, POINTS, 0, max_comps, 1)         # (_cc_read: rows beyond min(ncomp, max_comps) keep the fill)
    assert np.array_equal(got[1].reshape(len(POINTS), N), counts)           # ncomp is the true count
    for g in range(len(POINTS)):
        for i in range(N):
            labels, comps = ref[g][i]
            b = g * N + i
            M._same_cc((got[0][b], got[1][b], got[2][b]), labels, comps, max_comps, "point %d image %d" % (g, i))
    _same_slices(got, run_loop(L, device, score, link, POINTS, 0, max_comps, 1), "grid vs loop, short table")


def test_generator_rows_at_two_link_thresholds(device):
    """the serpentine (one component held by one directed link per edge, crossing tile borders again and again) and the
    tile-corner rows of the decode matrix as one batch, at their own link threshold and at one above every link"""
    L, _ = _lib()
    rows = {r.name: r for r in M.LINK_ROWS}
    batch = [rows[k] for k in ("serpentine", "corner_diag_down", "corner_anti_up", "corner_diag_none")]
    score = np.stack([r.score for r in batch])
    link = np.stack([r.link for r in batch], 1)
    tp, tl = float(M.TP), float(M.TL)
    points = [(tp, tl), (tp, 0.96)]
    h, w = score.shape[1:]
    for layout in (1, 2):
        got = run_grid(L, device, score, link, points, 0, h * w, layout)
        for i, r in enumerate(batch):
            labels, comps = M.ref_of(r)                                     # the decode matrix's own flood fill, shared
            M._same_cc((got[0][i], got[1][i], got[2][i]), labels, comps, h * w, r.name)
            b = len(batch) + i                                              # no link above 0.96: singletons
            k = int((r.score > M.TP).sum())
            assert got[1][b] == k and np.array_equal(got[2][b][:, 1], np.ones(k, np.int32)), r.name
            assert np.array_equal(got[2][b][:, 0], np.nonzero((r.score > M.TP).ravel())[0])
        assert got[1][:4].tolist() == [1, 1, 1, 2]
        _same_slices(got, run_loop(L, device, score, link, points, 0, h * w, layout), "generators vs loop")


def test_status_codes_leave_the_outputs_untouched(device):
    L, _ = _lib()
    n, h, w, G, mc = 2, 5, 7, 3, 8
    sc, lk = torch.zeros((n, h, w), dtype=F32, device=device), torch.zeros((8, n, h, w), dtype=F32, device=device)
    lab, nc, cp = M._cc_outputs(G * n, h, w, mc, device)
    nbytes = M._size(L, "ocr_link_cc_grid_workspace", G, n, h, w)
    ws = M._ws(nbytes, device)
    t = (FL * 66)(*([0.5] * 66))
    good = [sc, lk, 1, 0, n, h, w, G, t, t, 0, lab, nc, cp, mc, ws, SZ(nbytes)]

    def bad(j, value, want):
        args = list(good)
        args[j] = value
        assert _rc(L, "ocr_link_cc_grid", *args) == want, (j, value)
        torch.cuda.synchronize()
        assert lab.untouched() and nc.untouched() and cp.untouched() and ws.untouched(), (j, value)
    bad(7, 66, UNSUPPORTED)                                                 # G > 65
    args = list(good)
    args[4], args[7] = 1024, 64                                             # G * n = 65536 (refused before anything is read)
    assert _rc(L, "ocr_link_cc_grid", *args) == UNSUPPORTED
    bad(5, 2, UNSUPPORTED)                                                  # h = 2
    bad(6, 2, UNSUPPORTED)
    bad(16, SZ(nbytes - 1), WORKSPACE)
    for j in (0, 1, 11, 12, 13, 15):
        bad(j, None, INVALID_ARG)
    bad(8, ctypes.POINTER(ctypes.c_float)(), INVALID_ARG)                   # a null threshold table
    bad(9, ctypes.POINTER(ctypes.c_float)(), INVALID_ARG)
    for j in (4, 5, 6, 7, 14):
        bad(j, 0, INVALID_ARG)
    bad(2, 0, INVALID_ARG)
    bad(3, 1, INVALID_ARG)                                                  # offset == stride
    torch.cuda.synchronize()
    assert lab.untouched() and nc.untouched() and cp.untouched() and ws.untouched()
    assert M._size(L, "ocr_link_cc_grid_workspace", 0, n, h, w) == 0
    assert _rc(L, "ocr_link_cc_grid", *good) == OK                          # ... and the good call runs
    torch.cuda.synchronize()
    assert not lab.raw().any() and not nc.raw().any()


def test_ops_binding_equals_link_cc_decode(device):
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    g = Graph(device)
    score, link = maps_of(33, 65)
    sc, lk = M._f32(score, device), M._f32(link, device)
    labels, ncomp, comps = P.link_cc_decode_grid(sc, lk, [p for p, _ in POINTS], [l for _, l in POINTS], min_size=2,
                                                 max_comps=64, graph=g)
    for k, (tp, tl) in enumerate(POINTS):
        a, b, c = P.link_cc_decode(sc, lk, tp, tl, min_size=2, max_comps=64, graph=g)
        s = slice(k * N, (k + 1) * N)
        assert torch.equal(labels[s], a) and torch.equal(ncomp[s], b)
        for i in range(N):
            m = min(int(b[i]), 64)
            assert torch.equal(comps[s][i, :m], c[i, :m]) and not comps[s][i, m:].any()


# ------------------------------------------------------------------------------------------------ ocr_component_scores_grid
def test_component_scores_grid_equals_the_entry_per_slice(device):
    """labels of the grid decode against the n maps: bit-equal to ocr_component_scores on every point's slices, with ids
    beyond max_comps in the labels (ignored) and slices without a component (the 2.0 points: all zeros)"""
    L, ops = _lib()
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device)
    h, w, max_comps = 33, 65, 16
    score, link = maps_of(h, w)
    G = len(POINTS)
    glab, gn, _ = run_grid(L, device, score, link, POINTS, 0, h * w, 1)
    assert glab.max() > max_comps and not gn[4 * N:].any()
    labels, ncomp, sc = M._i32(glab, device), M._i32(gn, device), M._f32(score, device)
    out = Guard((G * N, max_comps), F32, device)
    ops.component_scores_grid(labels, sc, ncomp, out.t, g.workspace())
    torch.cuda.synchronize()
    got = out.np()
    for k in range(G):
        s = slice(k * N, (k + 1) * N)
        one = torch.full((N, max_comps), float("nan"), dtype=F32, device=device)
        ops.component_scores(labels[s].contiguous(), sc, ncomp[s].contiguous(), one, g.workspace())
        assert np.array_equal(got[s].view(np.int32), one.cpu().numpy().view(np.int32)), k
    assert not got[4 * N:].any() and (got[:N] > 0).any()
    # the status codes: nothing is written
    nbytes = M._size(L, "ocr_component_scores_grid_workspace", G, N, max_comps)
    assert nbytes == G * M._size(L, "ocr_component_scores_workspace", N, max_comps)
    fresh, ws = Guard((G * N, max_comps), F32, device), M._ws(nbytes, device)
    good = [labels, sc, ncomp, G, N, h, w, max_comps, fresh, ws, SZ(nbytes)]
    for j, value, want in ((3, 66, UNSUPPORTED), (4, 65536, UNSUPPORTED), (7, 65536, UNSUPPORTED), (10, SZ(nbytes - 1), WORKSPACE),
                           (0, None, INVALID_ARG), (8, None, INVALID_ARG), (3, 0, INVALID_ARG), (5, 0, INVALID_ARG)):
        args = list(good)
        args[j] = value
        assert _rc(L, "ocr_component_scores_grid", *args) == want, (j, value)
    torch.cuda.synchronize()
    assert fresh.untouched() and ws.untouched()
