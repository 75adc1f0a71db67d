"""GPU: every extern "C" entry of csrc/pixellink_balance.hip (6), csrc/summary.hip (10) and csrc/augment.hip (1) through the
C ABI, at the shapes where its code changes path: the second trip of every grid-stride loop, every capped grid, the merge of
the per-workgroup histograms, the persistent workgroups' second and third chunk.  The references are the ones the feature
tests already use and are imported, not copied: tests/balanced_ref.py (weight map, mining, sums34, loss10, gradients and
their bounds), `_reference` / `_check` / `_image_rule` of tests/test_gpu_summary.py and `restate` of
tests/test_gpu_augment.py.  All of them are vectorised NumPy already and fast enough at the largest rows, so no second
restatement is introduced.  Every output and workspace is a Guard (0xFF-filled between bands; a byte image is preset to the
complement of its reference so that every byte has to be written), every input is read back and compared with what was
uploaded.  ROWS is the inventory (name -> Row); tests/test_train_side_matrix_inventory.py lists it against the sources and
checks, with the references alone, that each row's inputs reach the edge the row is named after.

Rows and the edges they are built to reach
  weights/cells<N>    label cells 1 | 1023 | 1024 | 1025 (two workgroups: the LDS histograms meet in the global atomic) |
                      513 x 512 = 262656 (ceil / 1024 = 257 > the cap of 256 workgroups: further grid-stride trips), n = 2,
                      from a 64 x 64 cover (new > old at the largest)
  weights/<directed>  ratio (cover 48 x 80 -> 13 x 21), p254 (254 live polygons, 16 different areas), counts (n = 3 with 0, 1
                      and 254 polygons), above (a cover painted with 20 polygons read with max_polys = 12), ignore-bytes
                      (ignore bytes 255 and 2), split (one instance over cells 205 .. 327 of a 1025-cell map: both workgroups)
  loss/n<n>_hw<hw>_f<focal>   n = 1 at hw 1 | 1023 | 1024 | 1025 | 4097 (the 1024-thread mining workgroup's second and fifth
                      trip); n = 3 at hw 1025 (4 blocks, both image boundaries inside a workgroup) and 11000 (33 blocks: the
                      finaliser's nine trips over its four row groups); each with CE and focal links.  n = 3, hw = 349526:
                      total 1048578, ceil / 1024 = 1025 > the cap of 1024 blocks, five trips in reduce and selected, three in
                      bwd; CE only.
  mine/<row>          hw = 4097, n = 1: lowbyte (every negative's score shares its upper three bytes: the fourth radix pass
                      decides), ties (the k-th place inside a group of equal scores, mined whole), kmax (k == n_neg), floor
                      (the smallest score there is; see below), nan-label (NaN labels are negatives), nan-weight (NaN weights
                      are outside P)
  stats/4100          4100 segments of 1 .. 9 elements at offsets off the 16-byte grid: 4100 chunks > 2 * 2048 persistent
                      workgroups, every one takes a second chunk and four a third; every segment's values lie in a decade
                      (and sign) that neither its neighbour nor the segments 2048 and 4096 later use, so a bin the flush left
                      behind lands in a record whose reference has it empty
  stats/301           one segment of 300 * chunk + 5 elements: 301 partials, the final kernel's second trip
  stats/<layout>      one (n_segments = 1), overlap (two overlapping segments), last (the last segment ends at the buffer's
                      last element; the words around x hold 1e30)
  stats/refused       a table with another magic, a table built for another n_segments: every record marked, workspace
                      untouched; the host-side refusals of ocr_tensor_stats_table and ocr_tensor_stats_f32
  stats/constants     the six getters against the header's macros and the record dtype
  image/n<N>          elements 1 | 16383 | 16384 | 16385 (one trip of the 64 x 256 min/max pass) | 262144 | 262656 (the cap of
                      1024 workgroups in the u8 pass); c in 1, 3, 4
  image/<content>     145 x 113 x 1 = 16385 elements: nonfinite, no-finite, zeros, tiny (9e-7), tiny-signed, neg-zero,
                      max-last / min-last (the extreme in element n - 1: thread 0's second trip), max-wg63 / min-wg63 (element
                      16383: only workgroup 63 reads it), mn-gt-mx, mn-lt-mx
  augment/S<S>        S 1 | 2 | 3 | 4 | 5 | 36 (324 quads: a second workgroup with 68 live threads) | 37 | 128; n = 3 with three
                      source sizes at odd slab offsets, rotation + zoom, a shear, a saturating colour matrix
  augment/<map>/S<S>  S 36 (vector stores) and 5 (element stores): identity, half (taps at sx = -1 and W - 1), outside, big (A
                      entries of +-2^40), negfrac, src1x1, src1xW, sat0, sat255
  augment/unaligned   S = 36 into a dst 4 bytes off the 16-byte grid: equal to the aligned run

Bounds.  None is new: area, weight, threshold, selected mask, `_dyn` against the seeded plain form, image bytes and warped
pixels are bit for bit; sums34, loss10 and the gradients are held to the bounds balanced_ref returns (derived in the docstring
of tests/test_gpu_balanced_loss.py; m_sum(total) follows the trips); the f64 sums of a stats record to n 2^-52 sum|term|
(tests/test_gpu_summary.py), everything else in a record equal.

mine/floor.  This row was meant to hold a negative of score exactly 0.  No logit pair has one: det_exp clamps its
argument to [-80, 80] (csrc/loss_math.h, oracle.det_exp_f32), so the score 1 / (1 + exp(l1 - l0)) is at least
1 / (1 + e^80) = 1.8e-35.  The row holds negatives at that floor instead (l1 - l0 = 80, 100 and 1000: one tie group through
the clamp) with k = 1, and the inventory asserts the floor is positive.

Findings: none.  No row was over its bound, no exact row differed, no refusal wrote anything.

MEASURED (largest |err| / bound over the rows on the MI355X, f16 library; these kernels read f32 and integers only;
0.000 = bit-exact index work)
  instance_weights area / weight 0.000      threshold, selected mask       0.000
  balanced_loss_fwd_sums         0.138      balanced_loss_fwd              0.134      (both at n1_hw1_f1)
  balanced_loss_bwd_pixel        0.194      balanced_loss_bwd_link         0.268      (n3_hw349526_f0, n3_hw1025_f1)
  balanced_loss_bwd_dyn_pixel    0.184      balanced_loss_bwd_dyn_link     0.261      (n3_hw349526_f0, n3_hw11000_f1)
  _dyn against the plain form seeded grad_scale * s: bit-identical.
  tensor_stats_f32 sum           0.000      tensor_stats_f32 sum_squares   0.158      (stats/4100; the sums of stats/301 agree to
                                                                                       13 digits, its bound is n = 4.9 M times wider)
  num, nonfinite, min, max, every bucket, image bytes, warped pixels: equal.  No row was over its bound.
  Time on the MI355X: the file's 85 tests 5.6 s; slowest test_balanced_loss_capped_grid 2.0 s (the float64 reference over
  1 M pixels and 8 M links on the host).
"""
import ctypes
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import balanced_ref as B
import matrix_support
import test_gpu_augment as TA
import test_gpu_balanced_loss as TB
import test_gpu_summary as TS
from matrix_support import FL, INVALID_ARG, OK, SZ, Guard, _cdiv, _d32, _lib, _ratio, _raw, _rc, _rng, f32, f64
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu
_note = partial(matrix_support._note, "trainside")
i32, i64, u8, u32 = np.int32, np.int64, np.uint8, np.uint32
VP = ctypes.c_void_p


class Row:
    def __init__(self, name, entries, build, **meta):
        self.name, self.entries, self.build = name, tuple(entries), build
        self.__dict__.update(meta)


ROWS = {}
_CASES = {}


def _row(name, entries, build, **meta):
    assert name not in ROWS
    ROWS[name] = Row(name, entries, build, **meta)


def case(name):
    """a row's inputs and references, built once, without a device, and left unchanged"""
    if name not in _CASES:
        _CASES[name] = ROWS[name].build()
    return _CASES[name]


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same(t, a):
    """the device tensor still holds the bytes that were uploaded"""
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def _cmp(entry, row, got, ref, bound):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    bound = np.broadcast_to(np.asarray(bound, f64), ref.shape)
    assert got.shape == ref.shape and np.isfinite(got).all(), (entry, row)
    _note(entry, row, _ratio(np.abs(got - ref), bound + 2.0 ** -149))


# ------------------------------------------------------------------------------------------------ instance weight map
WEIGHTS = ("ocr_pixellink_instance_weights",)
WM_CELLS = {1: (1, 1), 1023: (33, 31), 1024: (32, 32), 1025: (25, 41), 262656: (513, 512)}
WM_PER_BLOCK, WM_CAP = 256 * 4, 256
RECTS64 = [(2, 2, 30, 20), (20, 10, 50, 40), (40, 44, 60, 62), (0, 50, 10, 63), (55, 0, 63, 8), (12, 30, 14, 33)]
# 254 rectangles on a 16 x 16 grid of 4 x 4 blocks of a 64 x 64 cover, (1 + k % 4) x (1 + k // 4 % 4) pixels: 16 areas
VARIED254 = [(4 * (k % 16), 4 * (k // 16), 4 * (k % 16) + k % 4, 4 * (k // 16) + (k // 4) % 4) for k in range(254)]
GRID20 = [(12 * (k % 5), 12 * (k // 5), 12 * (k % 5) + 9, 12 * (k // 5) + 7 + k % 3) for k in range(20)]


def wm_blocks(cells):
    return min(_cdiv(cells, WM_PER_BLOCK), WM_CAP)


def weight_case(h, w, nh, nw, images, P=None, flag=1):
    """images: per image (rectangles, indices whose ignore byte is `flag`)"""
    n = len(images)
    P = P or max([len(r) for r, _ in images] + [1])
    cover = np.stack([B.paint_cover(h, w, r) for r, _ in images]).astype(u32)
    ignore = np.zeros((n, P), u8)
    for b, (_, ig) in enumerate(images):
        for k, j in enumerate(ig):
            ignore[b, j] = flag[k] if isinstance(flag, tuple) else flag
    area, weight, live = B.instance_weights(cover, ignore, nh, nw)
    return dict(n=n, P=P, h=h, w=w, nh=nh, nw=nw, cover=cover, ignore=ignore, area=area, weight=weight, live=live,
                owner=B.owner_map(cover, nh, nw, P), raw_owner=B.owner_map(cover, nh, nw, 255))


WM_ROWS = {"cells%d" % c: (lambda s=s: weight_case(64, 64, s[0], s[1], [(RECTS64, [3]), ([(0, 0, 63, 63), (10, 10, 20, 50)], [])]))
           for c, s in WM_CELLS.items()}
WM_ROWS.update({
    "ratio": lambda: weight_case(48, 80, 13, 21, [([(2, 2, 40, 20), (30, 10, 79, 47), (50, 30, 60, 40)], [2]), ([(0, 0, 79, 47)], [])]),
    "p254": lambda: weight_case(64, 64, 64, 64, [(VARIED254, [])]),
    "counts": lambda: weight_case(64, 64, 64, 64, [([], []), ([(5, 9, 40, 33)], []), (VARIED254, [])], P=254),
    "above": lambda: weight_case(64, 64, 32, 32, [(GRID20, [1]), (GRID20[:14], [])], P=12),
    "ignore-bytes": lambda: weight_case(64, 64, 16, 16, [(RECTS64, [0, 2])], flag=(255, 2)),
    "split": lambda: weight_case(25, 41, 25, 41, [([(0, 5, 40, 7), (3, 12, 30, 20)], []), ([(0, 0, 40, 24)], [])]),
})
for _k, _b in WM_ROWS.items():
    _row("weights/" + _k, WEIGHTS, _b)


@pytest.mark.parametrize("key", list(WM_ROWS))
def test_instance_weights(device, key):
    L, _ = _lib()
    c = case("weights/" + key)
    cover, ig = _t(c["cover"].view(i32), device), _t(c["ignore"], device)
    area, weight = Guard((c["n"], c["P"]), torch.int32, device), Guard((c["n"], c["nh"], c["nw"]), torch.float32, device)
    assert _rc(L, "ocr_pixellink_instance_weights", cover, ig, c["n"], c["P"], c["h"], c["w"], c["nh"], c["nw"], area, weight) == OK
    torch.cuda.synchronize()
    assert np.array_equal(area.raw(), c["area"]), "area: %d entries differ" % int((area.raw() != c["area"]).sum())
    got = weight.np()
    bad = got.view(i32) != c["weight"].view(i32)
    assert not bad.any(), "%d weights differ, first at %s" % (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert not (got[c["owner"] == 0] != 0).any()
    for b in range(c["n"]):
        S = int(c["area"][b][c["live"][b]].sum())
        assert abs(got[b].astype(f64).sum() - S) <= 2.0 ** -24 * S
    assert _same(cover, c["cover"]) and _same(ig, c["ignore"]), "an input was written"


# ------------------------------------------------------------------------------------------------ the balanced loss
LOSS = ("ocr_balanced_loss_workspace", "ocr_balanced_loss_fwd", "ocr_balanced_loss_selected", "ocr_balanced_loss_bwd",
        "ocr_balanced_loss_bwd_dyn")
BL_PER_BLOCK, BL_CAP, MINE_THREADS, FINAL_GROUPS, NS34 = 256 * 4, 1024, 1024, 4, 34
LOSS_TOTALS = ((1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 1025), (3, 11000), (3, 349526))       # (n, hw)
LOSS_SMALL = LOSS_TOTALS[:-1] + ((1, 4097),)
CAPPED = LOSS_TOTALS[-1]
MINE_HW = 4097
MINE_ROWS = ("lowbyte", "ties", "kmax", "floor", "nan-label", "nan-weight")


def loss_case(n, hw, focal):
    c = TB._case(n, hw, focal, key="trainside")
    c.row = "n%d_hw%d_f%d" % (n, hw, focal)
    if hw == 1:                                        # the one cell is weighted text: the sums are not all zero
        c.plab[:], c.w[:] = 1, f32(1.5)
    return c


def lowbyte_differences():
    """l1 - l0 values (f32, rising) whose scores share the most populated upper three bytes among 4000 consecutive floats
    below -1: there a step of the difference moves the score by a fifth of an ulp, so the scores run through a whole
    256-value block"""
    d = -1.0 - np.arange(4000, dtype=f64) * 2.0 ** -23
    d = d.astype(f32)
    assert np.array_equal(d.astype(f64), -1.0 - np.arange(4000) * 2.0 ** -23)
    u = O.neg_score_f32(np.zeros_like(d), d).view(u32)
    top, cnt = np.unique(u >> 8, return_counts=True)
    return d[(u >> 8) == top[cnt.argmax()]]


def _mining(c, n_pos, d_neg, rng):
    """image 0 of c: n_pos weighted text cells, the rest negatives with l0 = 0 and l1 = d_neg (exact), shuffled"""
    hw = c.hw
    d_neg = np.asarray(d_neg, f32)
    assert len(d_neg) == hw - n_pos
    y = np.zeros(hw, f32)
    y[:n_pos] = 1
    w = np.where(y > 0, f32(1.5), f32(0))
    l = np.zeros((hw, 2), f32)
    l[:, 1] = np.concatenate([rng.standard_normal(n_pos).astype(f32), d_neg])
    perm = rng.permutation(hw)
    c.plab[0], c.w[0], c.pl[0] = y[perm], w[perm], l[perm]


def mine_case(kind):
    rng = _rng("trainside", "mine", kind)
    hw = MINE_HW
    c = TB._case(1, hw, 0, key=("trainside", kind), neg_ratio=1.0 if kind == "floor" else 3.0)
    c.row = "mine_" + kind
    if kind == "lowbyte":
        _mining(c, 500, rng.choice(lowbyte_differences(), hw - 500), rng)                   # k = 1500 of 3597
    elif kind == "ties":                                                                     # k = 300: inside the second group
        _mining(c, 100, np.repeat([2.0, 0.5, -1.0], [200, 300, hw - 600]), rng)
    elif kind == "kmax":                                                                     # k = min(3300, 2997)
        _mining(c, 1100, rng.standard_normal(hw - 1100), rng)
    elif kind == "floor":                                                                    # k = 1
        _mining(c, 1, np.concatenate([[80.0, 100.0, 1000.0], rng.uniform(-4, 4, hw - 4)]), rng)
    elif kind == "nan-label":
        _mining(c, 400, rng.standard_normal(hw - 400) * 2, rng)
        at = np.flatnonzero(c.plab[0] == 0)[::3]
        c.plab[0, at] = np.nan
    elif kind == "nan-weight":
        _mining(c, 400, rng.standard_normal(hw - 400) * 2, rng)
        c.w[0, np.flatnonzero(c.plab[0] > 0)[::4]] = np.nan                                 # text outside P: in neither set
        c.w[0, np.flatnonzero(c.plab[0] == 0)[::5]] = np.nan                                # a negative all the same
    return c


for _n, _hw in LOSS_SMALL:
    for _f in (0, 1):
        _row("loss/n%d_hw%d_f%d" % (_n, _hw, _f), LOSS, lambda a=_n, b=_hw, f=_f: loss_case(a, b, f))
_row("loss/n%d_hw%d_f0" % CAPPED, LOSS, lambda: loss_case(CAPPED[0], CAPPED[1], 0))
for _k in MINE_ROWS:
    _row("mine/" + _k, LOSS, lambda k=_k: mine_case(k))


def loss_reference(name):
    """balanced_ref.loss_ref of a row, kept with the row"""
    if ("ref", name) not in _CASES:
        _CASES["ref", name] = B.loss_ref(case(name))
    return _CASES["ref", name]


def _run_loss(device, name):
    """fwd, selected, bwd and bwd_dyn on one row, everything checked against balanced_ref"""
    L, _ = _lib()
    c, r = case(name), loss_reference(name)
    d = TB._desc(L, c)
    dr = ctypes.byref(d)
    total = c.n * c.hw
    nb = int(L._fn("ocr_balanced_loss_workspace", SZ)(dr))
    assert nb == B.blocks(total) * NS34 * 4
    pl, ll, plab, llab, w = (_d32(a, device) for a in (c.pl, c.ll, c.plab, c.llab, c.w))
    thr, sums, loss, ws = (Guard(s, torch.float32, device) for s in ((c.n,), (NS34,), (10,), (nb // 4,)))
    assert _rc(L, "ocr_balanced_loss_fwd", dr, pl, ll, plab, llab, w, thr, sums, loss, ws, SZ(nb)) == OK
    mask = Guard((c.n, c.hw), torch.uint8, device, init=np.full((c.n, c.hw), 7, u8))
    assert _rc(L, "ocr_balanced_loss_selected", dr, pl, plab, w, thr, mask) == OK
    torch.cuda.synchronize()
    out = NS(r=r, thr=thr.np(), sums=sums.np(), loss=loss.np(), mask=mask.raw())
    assert ws.ok()
    assert np.array_equal(out.thr.view(i32), r.thr.view(i32)), (out.thr, r.thr)
    assert np.array_equal(out.mask, (r.W != 0).astype(u8)), "mask: %d cells differ" % int((out.mask != (r.W != 0)).sum())
    _cmp("balanced_loss_fwd_sums", c.row, out.sums, r.sums, r.sums_bound)
    _cmp("balanced_loss_fwd", c.row, out.loss, r.loss, r.loss_bound)
    scale = _d32(np.array([3.0], f32), device)
    runs = {}
    for tag, entry, gs, extra in (("bwd", "ocr_balanced_loss_bwd", f32(1.7), ()), ("bwd_dyn", "ocr_balanced_loss_bwd_dyn", f32(0.85), (scale,)),
                                  ("seeded", "ocr_balanced_loss_bwd", f32(0.85) * f32(3.0), ())):
        dpl, dll = Guard((c.n, c.hw, 2), torch.float32, device), Guard((c.n, c.hw, 16), torch.float32, device)
        assert _rc(L, entry, dr, pl, ll, plab, llab, w, thr, sums, FL(gs), *extra, dpl, dll) == OK
        torch.cuda.synchronize()
        gp, gl = dpl.np(), dll.np()                      # every element written
        del dpl, dll
        if tag != "seeded":                              # (the seeded run is held to the _dyn run bit for bit below)
            rp, bp, rl, bl = B.grad_ref(c, r, out.sums, f64(gs * f32(3.0)) if extra else f64(gs))
            _cmp("balanced_loss_%s_pixel" % tag, c.row, gp, rp, bp)
            _cmp("balanced_loss_%s_link" % tag, c.row, gl, rl, bl)
            del rp, bp, rl, bl
        assert (gp[r.W == 0] == 0).all(), "a pixel gradient on a cell of weight 0"
        assert (gl[~r.P] == 0).all(), "a link gradient outside P"
        runs[tag] = (gp, gl)
    for a, b in zip(runs["bwd_dyn"], runs["seeded"]):
        assert np.array_equal(a.view(i32), b.view(i32)), "_dyn differs from the plain form seeded grad_scale * s"
    out.dpl, out.dll = runs["bwd"]
    for t, a in ((pl, c.pl), (ll, c.ll), (plab, c.plab), (llab, c.llab), (w, c.w), (scale, np.array([3.0], f32))):
        assert _same(t, a), "an input was written"
    return out


@pytest.mark.parametrize("focal", [0, 1])
@pytest.mark.parametrize("n,hw", LOSS_SMALL)
def test_balanced_loss(device, n, hw, focal):
    out = _run_loss(device, "loss/n%d_hw%d_f%d" % (n, hw, focal))
    assert out.loss[0] > 0 and (hw == 1 or out.r.mined.any())


def test_balanced_loss_capped_grid(device):
    L, _ = _lib()
    n, hw = CAPPED
    c = case("loss/n%d_hw%d_f0" % CAPPED)
    assert int(L._fn("ocr_balanced_loss_workspace", SZ)(ctypes.byref(TB._desc(L, c)))) == 1024 * 34 * 4
    out = _run_loss(device, "loss/n%d_hw%d_f0" % CAPPED)
    assert out.r.mined.all(1).sum() == 0 and out.r.mined.any(1).all() and len(set(out.thr.tolist())) == 3


@pytest.mark.parametrize("kind", MINE_ROWS)
def test_directed_mining(device, kind):
    out = _run_loss(device, "mine/" + kind)
    c, r = case("mine/" + kind), out.r
    mined = out.mask.astype(bool) & ~r.P
    assert mined.sum() == r.mined.sum() >= r.ks[0] > 0
    if kind == "ties":
        assert r.ks == [300] and int(mined.sum()) == 500
    if kind == "kmax":
        assert int(mined.sum()) == r.ks[0] == MINE_HW - 1100
    if kind == "floor":
        assert int(mined.sum()) == 3 and out.thr[0] > 0


# ------------------------------------------------------------------------------------------------ tensor statistics
STATS = ("ocr_tensor_stats_table", "ocr_tensor_stats_f32", "ocr_tensor_stats_workspace", "ocr_tensor_stats_table_bytes")
STATS_GETTERS = ("ocr_tensor_stats_num_buckets", "ocr_tensor_stats_chunk", "ocr_tensor_stats_record_bytes", "ocr_tensor_stats_workspace",
                 "ocr_tensor_stats_table_bytes", "ocr_tensor_stats_limits")
STATS_GRID, CHUNK, BUCKETS, POS_LIMITS, RECORD_BYTES, PARTIAL_BYTES, FINAL_THREADS = 2048, 16384, 1551, 775, 6240, 32, 256
HEADER_BYTES, SEG_BYTES, MAGIC = 16, 24, 0x53544154
XBAND = 64                                # f32 words of 1e30 on either side of x
DECADES = 29                              # 1e-10 .. 1e18


def _specials(rng, v):
    at = rng.choice(v.size, 12, replace=False)
    v[at] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, 1e-13, 1.0, -1.0]


def stats_case(kind):
    rng = _rng("trainside", "stats", kind)
    mul = (1.0, None)
    if kind == "4100":
        sizes = [1 + k % 9 for k in range(4100)]
        offs, o = [], 1
        for k, s in enumerate(sizes):
            offs.append(o)
            o += s + 1 + k % 3
        x = np.full(o + 3, TS.PAD, f32)
        for k, (off, s) in enumerate(zip(offs, sizes)):
            dec = (k + 3 * (k // STATS_GRID)) % DECADES - 10
            x[off:off + s] = (rng.uniform(1, 8, s) * 10.0 ** dec * (-1 if k % 5 == 0 else 1)).astype(f32)
        mul = (0.5, 3.0)
    elif kind == "301":
        n = 300 * CHUNK + 5
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-14, 6, n)).astype(f32)
        _specials(rng, x)
        x[np.abs(x) == f32(3e38)] = 2.5            # (nothing that would drown the sums: their bound is to mean something here)
        x[0], x[-1] = -5e7, np.inf                 # the minimum in the first chunk, a non-finite element in the last
        offs, sizes = [0], [n]
    else:
        n = CHUNK + 11
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-14, 6, n)).astype(f32)
        _specials(rng, x)
        offs, sizes = {"one": ([1], [CHUNK + 3]), "overlap": ([2, 3000], [5000, CHUNK - 3000 + 7]), "last": ([0, 9], [7, n - 9])}[kind]
    with np.errstate(all="ignore"):
        v = x * (f32(mul[0]) * (f32(1) if mul[1] is None else f32(mul[1])))
    assert v.dtype == f32
    x.setflags(write=False)
    return dict(x=x, offs=offs, sizes=sizes, mul=mul, refs=[TS._reference(v[o:o + s]) for o, s in zip(offs, sizes)],
                n_chunks=sum(_cdiv(s, CHUNK) for s in sizes))


STATS_ROWS = ("4100", "301", "one", "overlap", "last")
for _k in STATS_ROWS:
    _row("stats/" + _k, STATS, lambda k=_k: stats_case(k))
_row("stats/refused", ("ocr_tensor_stats_table", "ocr_tensor_stats_f32"), lambda: stats_case("overlap"))
_row("stats/constants", STATS_GETTERS, lambda: None)


def host_table(L, offs, sizes, n_table=None):
    """(status, table as numpy uint8, n_chunks) of ocr_tensor_stats_table; no device involved"""
    offs, sizes = np.ascontiguousarray(offs, i64), np.ascontiguousarray(sizes, i64)
    n = len(offs) if n_table is None else n_table
    table = np.zeros((int(L._fn("ocr_tensor_stats_table_bytes", SZ)(ctypes.c_int(max(n, 1)))) + 7) // 8, i64)
    nc = ctypes.c_int64(-7)
    rc = _raw(L, "ocr_tensor_stats_table", ctypes.c_int(n), offs.ctypes.data_as(VP), sizes.ctypes.data_as(VP), table.ctypes.data_as(VP),
              ctypes.byref(nc))
    return rc, table.view(u8), int(nc.value)


class StatsRun:
    """x between two bands of 1e30, the table, records and a workspace of exactly the queried size as Guards"""

    def __init__(self, device, c, table=None, n_segments=None, n_chunks=None):
        from tensorflow_ocr_amd import summary
        L, _ = _lib()
        self.L, self.c, self.n = L, c, n_segments or len(c["offs"])
        if table is None:
            rc, table, nc = host_table(L, c["offs"], c["sizes"])
            assert rc == OK and nc == c["n_chunks"]
        self.host_table = table
        self.table = _t(table.view(i64), device)
        self.host_flat = np.concatenate([np.full(XBAND, TS.PAD, f32), c["x"], np.full(XBAND, TS.PAD, f32)])
        self.flat = _t(self.host_flat, device)
        self.x = self.flat[XBAND:XBAND + c["x"].size]
        assert summary.RECORD_DTYPE.itemsize == RECORD_BYTES
        n_chunks = n_chunks or c["n_chunks"]
        self.ws_bytes = int(L._fn("ocr_tensor_stats_workspace", SZ)(ctypes.c_int64(n_chunks)))
        assert self.ws_bytes == PARTIAL_BYTES * n_chunks
        self.rec = Guard((self.n * RECORD_BYTES // 8,), torch.int64, device)
        self.ws = Guard((self.ws_bytes // 8,), torch.int64, device)
        self.mul_dev = None if c["mul"][1] is None else _d32(np.array([c["mul"][1]], f32), device)

    def call(self, x=None, table=None, n=None, rec=None, ws=None, ws_bytes=None):
        pick = lambda v, d: d if v is None else v
        return _rc(self.L, "ocr_tensor_stats_f32", pick(x, self.x), pick(table, self.table), pick(n, self.n), FL(self.c["mul"][0]), self.mul_dev,
                   pick(rec, self.rec), pick(ws, self.ws), SZ(pick(ws_bytes, self.ws_bytes)))

    def records(self):
        from tensorflow_ocr_amd import summary
        torch.cuda.synchronize()
        assert self.ws.ok()
        return self.rec.raw().view(summary.RECORD_DTYPE)

    def inputs_unwritten(self):
        return _same(self.flat, self.host_flat) and _same(self.table, self.host_table.view(i64))


@pytest.mark.parametrize("kind", STATS_ROWS)
def test_tensor_stats(device, kind):
    from tensorflow_ocr_amd import summary
    c = case("stats/" + kind)
    r = StatsRun(device, c)
    assert r.call() == OK
    raw = r.records()
    worst = [0.0, 0.0]
    for k, ref in enumerate(c["refs"]):
        rec = summary.record_dict(raw[k])
        TS._check(rec, ref, "stats/%s segment %d" % (kind, k))
        n = ref["num"]
        worst[0] = max(worst[0], _ratio(abs(rec["sum"] - ref["sum"]), n * 2.0 ** -52 * ref["abs_sum"]))
        worst[1] = max(worst[1], _ratio(abs(rec["sum_squares"] - ref["sum_squares"]), n * 2.0 ** -52 * ref["sum_squares"]))
    _note("tensor_stats_f32", "%s sum" % kind, worst[0])
    _note("tensor_stats_f32", "%s sum_squares" % kind, worst[1])
    assert (raw["reserved"] == 0).all() and r.inputs_unwritten()
    first = raw.tobytes()
    assert r.call() == OK                                    # the workspace and the records are reused as they are
    assert r.records().tobytes() == first


def _marked(raw):
    return (raw["nonfinite"] == 0xFFFFFFFF).all() and (raw["num"] == 0).all() and not raw["bucket"].any()


def test_tensor_stats_refusals(device):
    L, _ = _lib()
    c = case("stats/refused")
    # on the device: a table that is none, a table for another number of segments
    rc, table, _ = host_table(L, c["offs"], c["sizes"])
    bad = table.copy()
    bad.view(u32)[3] ^= 1
    assert rc == OK and table.view(u32)[3] == MAGIC
    rc3, table3, nc3 = host_table(L, c["offs"] + [0], c["sizes"] + [5])
    assert rc3 == OK and table3.view(i32)[0] == 3 and nc3 == 3
    for what, tb, n in (("magic", bad, 2), ("n_segments 3 read as 2", table3, 2), ("n_segments 2 read as 3", table, 3)):
        r = StatsRun(device, c, table=tb, n_segments=n, n_chunks=3)          # room for either table's chunks: the header alone refuses
        assert r.call() == OK, what
        torch.cuda.synchronize()
        assert r.ws.untouched(), what
        assert _marked(r.records()) and r.inputs_unwritten(), what
    # ocr_tensor_stats_table on the host
    for what, offs, sizes in (("negative offset", [0, -1], [4, 4]), ("size 0", [0, 8], [4, 0]), ("size 2^32", [0, 8], [4, 2 ** 32]),
                              ("chunks above 2^31 - 1", [0] * 8193, [2 ** 32 - 1] * 8193)):
        assert host_table(L, offs, sizes)[0] == INVALID_ARG, what
    assert 8193 * _cdiv(2 ** 32 - 1, CHUNK) > 2 ** 31 - 1 >= 8191 * _cdiv(2 ** 32 - 1, CHUNK)
    assert host_table(L, [0] * 8191, [2 ** 32 - 1] * 8191)[::2] == (OK, 8191 * 2 ** 18)
    offs, sizes, tb, nc = np.zeros(2, i64), np.ones(2, i64), np.zeros(2048, i64), ctypes.c_int64(0)
    good = [ctypes.c_int(2), offs.ctypes.data_as(VP), sizes.ctypes.data_as(VP), tb.ctypes.data_as(VP), ctypes.byref(nc)]
    assert _raw(L, "ocr_tensor_stats_table", *good) == OK and nc.value == 2
    for k in (1, 2, 3, 4):
        a = list(good)
        a[k] = None
        assert _raw(L, "ocr_tensor_stats_table", *a) == INVALID_ARG, k
    assert _raw(L, "ocr_tensor_stats_table", ctypes.c_int(0), *good[1:]) == INVALID_ARG
    # ocr_tensor_stats_f32 on the host
    r = StatsRun(device, c)
    off = lambda g, by: VP(g.t.data_ptr() + by)
    for what, kw in (("x + 2 bytes", dict(x=VP(r.x.data_ptr() + 2))), ("records + 4", dict(rec=off(r.rec, 4))), ("workspace + 4", dict(ws=off(r.ws, 4))),
                     ("table + 4", dict(table=VP(r.table.data_ptr() + 4))), ("n_segments 0", dict(n=0)), ("n_segments -1", dict(n=-1))):
        assert r.call(**kw) == INVALID_ARG, what
    for k in ("x", "table", "rec", "ws"):
        assert r.call(**{k: VP(0)}) == INVALID_ARG, k
    torch.cuda.synchronize()
    assert r.rec.untouched() and r.ws.untouched() and r.inputs_unwritten(), "a refused call wrote"
    assert r.call() == OK and not _marked(r.records())


def test_tensor_stats_constants(device):
    from tensorflow_ocr_amd import summary
    L, _ = _lib()
    assert _raw(L, "ocr_tensor_stats_num_buckets") == BUCKETS == 2 * POS_LIMITS + 1 and _raw(L, "ocr_tensor_stats_chunk") == CHUNK
    assert int(L._fn("ocr_tensor_stats_record_bytes", SZ)()) == RECORD_BYTES == summary.RECORD_DTYPE.itemsize
    ws, tb = L._fn("ocr_tensor_stats_workspace", SZ), L._fn("ocr_tensor_stats_table_bytes", SZ)
    assert [int(ws(ctypes.c_int64(v))) for v in (-1, 0, 1, 4100, 2 ** 31 - 1)] == [0, 0, 32, 4100 * 32, (2 ** 31 - 1) * 32]
    assert [int(tb(ctypes.c_int(v))) for v in (-1, 0, 1, 4100)] == [HEADER_BYTES + 8 * POS_LIMITS + SEG_BYTES * max(v, 0) for v in (-1, 0, 1, 4100)]
    lim = np.full(BUCKETS + 2, -7.0)
    assert _raw(L, "ocr_tensor_stats_limits", lim[1:].ctypes.data_as(VP), ctypes.c_int(BUCKETS)) == OK
    assert lim[0] == -7 and lim[-1] == -7 and np.array_equal(lim[1:-1], summary.bucket_limits())
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(np.finfo(f64).max)
    assert len(pos) == POS_LIMITS and np.array_equal(lim[1:-1], np.array([-p for p in pos[::-1]] + [0.0] + pos))
    for n in (BUCKETS - 1, BUCKETS + 1, 0):
        assert _raw(L, "ocr_tensor_stats_limits", lim[1:].ctypes.data_as(VP), ctypes.c_int(n)) == INVALID_ARG
    assert _raw(L, "ocr_tensor_stats_limits", None, ctypes.c_int(BUCKETS)) == INVALID_ARG


# ------------------------------------------------------------------------------------------------ image summary
IMAGE = ("ocr_summary_image_workspace", "ocr_summary_image_u8")
IMG_GRID, IMG_U8_CAP = 64, 1024
IMG_TRIP = IMG_GRID * 256
IMAGE_SHAPES = {1: (1, 1, 1), 16383: (127, 43, 3), 16384: (64, 64, 4), 16385: (145, 113, 1), 262144: (256, 256, 4), 262656: (171, 512, 3)}
IMAGE_CONTENT = ("nonfinite", "no-finite", "zeros", "tiny", "tiny-signed", "neg-zero", "max-last", "min-last", "max-wg63", "min-wg63",
                 "mn-gt-mx", "mn-lt-mx")
CONTENT_SHAPE = IMAGE_SHAPES[16385]


def image_ref(x):
    """TS._image_rule, with the two things it leaves open said: an inf / NaN element gives 0, and so does every element of
    a map without a finite one"""
    fin = np.isfinite(x)
    if not fin.any():
        return np.zeros(x.shape, u8)
    with np.errstate(all="ignore"):
        out = TS._image_rule(np.where(fin, x, x[fin][0]))
    out[~fin] = 0
    return out


def image_case(kind, shape):
    rng = _rng("trainside", "image", kind, shape)
    n = int(np.prod(shape))
    x = rng.uniform(0, 7.3, n).astype(f32) if kind in ("size-even", "max-last", "max-wg63", "neg-zero") else (rng.standard_normal(n) * 40).astype(f32)
    at = None
    if kind == "nonfinite":
        at = rng.choice(n, 300, replace=False)
        x[at] = np.tile(np.array([np.inf, -np.inf, np.nan], f32), 100)
    elif kind == "no-finite":
        x[:] = np.tile(np.array([np.inf, -np.inf, np.nan, -np.nan], f32), n // 4 + 1)[:n]
    elif kind == "zeros":
        x[:] = 0
    elif kind == "tiny":
        x = rng.uniform(0, 9e-7, n).astype(f32)
        x[n // 2] = 9e-7
    elif kind == "tiny-signed":
        x = rng.uniform(-9e-7, 9e-7, n).astype(f32)
        x[n // 2], x[n // 3] = 9e-7, -9e-7
    elif kind == "neg-zero":
        x[::7] = -0.0
    elif kind in ("max-last", "max-wg63"):
        at = n - 1 if kind == "max-last" else IMG_TRIP - 1
        x[at] = 50.0
    elif kind in ("min-last", "min-wg63"):
        at = n - 1 if kind == "min-last" else IMG_TRIP - 1
        x[at] = -900.0
    elif kind == "mn-gt-mx":
        x = np.clip(x, -250, 90)
        x[5], x[n - 7] = -250, 90
    elif kind == "mn-lt-mx":
        x = np.clip(x, -90, 250)
        x[5], x[n - 7] = -90, 250
    x = x.reshape(shape)
    x.setflags(write=False)
    return dict(x=x, ref=image_ref(x), at=at)


for _n, _s in IMAGE_SHAPES.items():
    _row("image/n%d" % _n, IMAGE, lambda s=_s, k=("size-even" if _n % 2 == 0 else "size-odd"): image_case(k, s))
for _k in IMAGE_CONTENT:
    _row("image/" + _k, IMAGE, lambda k=_k: image_case(k, CONTENT_SHAPE))
IMAGE_ROWS = [k[6:] for k in ROWS if k.startswith("image/")]


@pytest.mark.parametrize("key", IMAGE_ROWS)
def test_image_summary(device, key):
    L, _ = _lib()
    c = case("image/" + key)
    h, w, ch = c["x"].shape
    nb = int(L._fn("ocr_summary_image_workspace", SZ)())
    assert nb == 2 * IMG_GRID * 4
    x = _d32(c["x"].copy(), device)
    ws = Guard((nb // 4,), torch.float32, device)
    out = Guard((h, w, ch), torch.uint8, device, init=~c["ref"])           # every byte has to be written to match
    assert _rc(L, "ocr_summary_image_u8", x, h, w, ch, out, ws) == OK
    torch.cuda.synchronize()
    got = out.raw()
    bad = got != c["ref"]
    assert not bad.any(), "%d bytes differ, first at %s: %s, reference %s" % (int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:3], c["ref"][bad][:3])
    assert ws.ok() and _same(x, c["x"])


def test_image_summary_refusals(device):
    L, _ = _lib()
    x = _d32(np.ones((4, 4, 4), f32), device)
    ws, out = Guard((128,), torch.float32, device), Guard((4, 4, 4), torch.uint8, device)
    good = [x, 4, 4, 1, out, ws]
    for what, k, v in (("c 2", 3, 2), ("c 0", 3, 0), ("c 5", 3, 5), ("h 0", 1, 0), ("w 0", 2, 0), ("h -1", 1, -1), ("x null", 0, None), ("out null", 4, None),
                       ("ws null", 5, None), ("ws + 2 bytes", 5, VP(ws.t.data_ptr() + 2)), ("x + 2 bytes", 0, VP(x.data_ptr() + 2))):
        a = list(good)
        a[k] = v
        assert _rc(L, "ocr_summary_image_u8", *a) == INVALID_ARG, what
    assert _rc(L, "ocr_summary_image_u8", x, 32768, 32768, 3, out, ws) == INVALID_ARG            # 3 * 2^30 elements
    assert _rc(L, "ocr_summary_image_u8", x, 32768, 32769, 1, out, ws) == INVALID_ARG            # 2^30 + 2^15
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()
    assert _rc(L, "ocr_summary_image_u8", *good) == OK
    torch.cuda.synchronize()
    assert (out.raw().reshape(-1)[:16] == 255).all() and ws.ok()            # a map of ones: 255 / 1


# ------------------------------------------------------------------------------------------------ augmentation
AUGMENT = ("ocr_augment_u8_batch",)
PX = 4
AUG_S = (1, 2, 3, 4, 5, 36, 37, 128)
AUG_MAPS = ("identity", "half", "outside", "big", "negfrac", "src1x1", "src1xW", "sat0", "sat255")
MAP_S = {36: (30, 20), 5: (4, 3)}                       # S -> (H, W) of the source the map rows read
SRC_SIZES = [(37, 53), (64, 64), (130, 71)]
GAPS = (7, 1, 4, 5)                                    # bytes of 0xFB in front of, between and behind the images
IDENT, EYE = TA.IDENT, TA.EYE
SAT = np.array([[2.5, -0.9, 0.2, -60.0], [-1.25, 3.0, -0.5, 20.5], [0.1, 0.2, 1.7, -200.0]], f32)


def aug_quads(S):
    return S * _cdiv(S, PX)


def _slab(ims):
    """the images in one slab with odd gaps of a value no image byte is likely to equal -> (slab, offsets)"""
    parts, offs, o = [], [], 0
    for k, im in enumerate(ims):
        parts.append(np.full(GAPS[k % 4], 0xFB, u8))
        o += GAPS[k % 4]
        offs.append(o)
        parts.append(im.reshape(-1))
        o += im.size
    parts.append(np.full(GAPS[len(ims) % 4] + 16, 0xFB, u8))
    return np.concatenate(parts), offs


def augment_case(ims, recs, S):
    """recs: (image index, A, col) per output image"""
    slab, offs = _slab(ims)
    ref = np.stack([TA.restate(ims[i], A, col, S) for i, A, col in recs])
    assert ref.dtype == f32 and np.isfinite(ref).all()
    return dict(ims=ims, recs=recs, S=S, slab=slab, offs=[offs[i] for i, _, _ in recs], ref=ref)


def size_case(S):
    rng = _rng("trainside", "augment", "sources")
    ims = [rng.integers(0, 256, size=(h, w, 3)).astype(u8) for h, w in SRC_SIZES]
    th = np.deg2rad(17.0)
    co, si = int(round(np.cos(th) * 65536 * 1.3)), int(round(np.sin(th) * 65536 * 1.3))
    recs = [(2, (co, -si, 20 << 16, si, co, -(10 << 16)), EYE), (0, (65536, 21845, -(5 << 16), -9000, 70000, 1 << 16), SAT),
            (1, (3 << 16, 0, -(40 << 16) + 777, 0, 3 << 16, -(30 << 16) - 12345), EYE)]
    return augment_case(ims, recs, S)


def map_case(kind, S):
    rng = _rng("trainside", "augment", kind, S)
    H, W = {"src1x1": (1, 1), "src1xW": (1, MAP_S[S][1])}.get(kind, MAP_S[S])
    im = rng.integers(0, 256, size=(H, W, 3)).astype(u8)
    col = EYE
    A = IDENT
    if kind == "half":
        A = (65536, 0, -32768, 0, 65536, 0)
    elif kind == "outside":
        A, col = (65536, 0, 1000 << 16, 0, 65536, -(500 << 16)), np.array([[1, 0, 0, -5.0], [0, 1, 0, 300.0], [0, 0, 1, 77.5]], f32)
    elif kind == "big":
        A = (2 ** 40, -2 ** 41, 1 << 16, -2 ** 40, 2 ** 40, 2 << 16)          # only pixel (0, 0) lands inside the source
    elif kind == "negfrac":
        A = (65536, 0, -90000, 0, 65536, -40000)
    elif kind in ("src1x1", "src1xW"):
        A = (20000, 0, -30000, 0, 30000, -70000)
    elif kind == "sat0":
        col = np.array([[-1, 0, 0, 10.0], [0, -2, 0, 3.0], [-1, -1, -1, 0.0]], f32)
    elif kind == "sat255":
        col = np.array([[4, 0, 0, 100.0], [0, 1, 0, 250.0], [1, 1, 1, 0.0]], f32)
    return augment_case([im], [(0, A, col)], S)


def map_coords(c):
    """(sx, sy) of the first record of a case, unclamped, as `restate` forms them"""
    A = [int(a) for a in c["recs"][0][1]]
    dy, dx = np.mgrid[0:c["S"], 0:c["S"]].astype(i64)
    return ((A[0] * dx + A[1] * dy + A[2] + 1024) >> 11) >> 5, ((A[3] * dx + A[4] * dy + A[5] + 1024) >> 11) >> 5


for _S in AUG_S:
    _row("augment/S%d" % _S, AUGMENT, lambda S=_S: size_case(S))
for _k in AUG_MAPS:
    for _S in MAP_S:
        _row("augment/%s/S%d" % (_k, _S), AUGMENT, lambda k=_k, S=_S: map_case(k, S))
_row("augment/unaligned", AUGMENT, lambda: size_case(36))
AUG_ROWS = [k[8:] for k in ROWS if k.startswith("augment/") and k != "augment/unaligned"]


def _augment(device, c, shift=0):
    """-> (output [n, S, S, 3], the Guard it lies in); shift: f32 words between the Guard's aligned start and dst"""
    from tensorflow_ocr_amd.datasets.augment import pack_desc
    L, _ = _lib()
    n, S = len(c["recs"]), c["S"]
    desc = pack_desc(c["offs"], [c["ims"][i].shape for i, _, _ in c["recs"]], [(np.array(A, i64), col) for _, A, col in c["recs"]], c["slab"].size)
    d_slab, d_desc = _t(c["slab"], device), _t(desc.view(u8).copy(), device)
    g = Guard((shift + n * S * S * 3,), torch.float32, device)
    dst = g.t[shift:]
    assert dst.data_ptr() % 16 == 4 * shift
    assert _rc(L, "ocr_augment_u8_batch", d_slab, d_desc, n, S, dst) == OK
    torch.cuda.synchronize()
    a = g.raw()
    assert np.isnan(a[:shift]).all() and not np.isnan(a[shift:]).any(), "dst: words in front written, or words left unwritten"
    assert _same(d_slab, c["slab"]) and _same(d_desc, desc.view(u8)), "an input was written"
    return a[shift:].reshape(n, S, S, 3), g


@pytest.mark.parametrize("key", AUG_ROWS)
def test_augment(device, key):
    c = case("augment/" + key)
    got, _ = _augment(device, c)
    bad = got.view(i32) != c["ref"].view(i32)
    assert not bad.any(), "%d values differ, first at %s" % (int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_augment_dst_off_the_16_byte_grid(device):
    c = case("augment/unaligned")
    a, _ = _augment(device, c)
    b, _ = _augment(device, c, shift=1)
    assert np.array_equal(a.view(i32), b.view(i32)) and np.array_equal(b.view(i32), c["ref"].view(i32))
