"""GPU: every entry of csrc/optim.hip and csrc/s2d.hip — the two files that write the parameters themselves — against a
float64 (update steps, sum of squares) or an integer (16-bit rounding, data movement) restatement in NumPy of the
formula in the kernel.  Every entry is called through ctypes on the library tensorflow_ocr_amd.ops binds and the status
of each call is asserted.  Every buffer a call may write sits between guard bands (matrix_support.carve / Guard), the
f32 ones at each of the four 4-byte offsets inside 16 bytes with the slack words checked as well, and every buffer a
call must only read is compared bit for bit afterwards.  tests/test_optim_matrix_host.py shows on the CPU that the
bounds below separate the kernel's formula from ten near misses of it, and that an uncontracted f32 restatement stays
inside them.

Kernels and the rows that reach them
  adam_kernel<AdamP|AdamDynP|AdamClipP>, momentum_kernel<MomP|MomDynP|MomClipP>
                            test_update: (plain | dyn | clip) x (ema | NULL) x n 1 | 5 | 257 | 256*4096 + 5 (one past the
                            4096-workgroup cap of ogrid: the grid-stride loop makes a second trip) x n_reg 0 | 1 | n - 1 | n |
                            3, 100, 300007 (no multiple of 256), three in-place steps each, the reference re-seeded from
                            the device state after every step; test_update_zero (g = m = v = 0), test_update_skip (skip = 1 in
                            the dyn / clip state), test_update_refusals
  pack_weights_kernel       test_pack: cin x cout 1x1 | 31x33 | 32x32 | 33x31 | 40x24 | 1x33 | 33x1, taps 1 | 4 | 9, both
                            layouts, w_kc alone, w_ck alone; unrounded operands with the DIRECTED set below
  pack_weights_batch_kernel test_pack_batch: 1 item; 61 items (single-block items first, last and side by side so the
                            bisection over block_first meets every boundary; one with ld_ck = 32 > cout; one per missing
                            layout); test_pack_refusals (ocr_pack_weights_batch_table, ocr_pack_weights_batch_f16)
  pack_small_kernel         test_pack_small: cout 1 | 31 | 32 x cin 1 | 13 (two workgroups), zero padding
  scale_kernel, fill_kernel test_scale_fill: the n of test_update, each 4-byte offset
  sumsq_partial_kernel, sumsq_final_kernel   test_sum_squares: n 1 | 2 | 3 | 4 | 5 | 1023 | 4*256*1024 + 4*256 + 3 (past the
                            1024-workgroup cap, n & 3 tail), twice for the same bits; inf and NaN in body and tail;
                            test_sum_squares_refusals (misaligned pointer, workspace one byte short)
  loss_scale_init_kernel, grad_check_kernel, grad_clip_init_kernel, grad_clip_kernel<false|true>, grad_accum_init_kernel,
  grad_accum_kernel, grad_accum_advance_kernel   test_state_entries: one call each, status and one result (their own files
                            tests/test_gpu_loss_scale.py, test_gpu_grad_clip.py and test_gpu_grad_accum.py are exhaustive)
  space_to_depth_kernel, depth_to_space_kernel   test_s2d: (1, 2, 2, 8) | (2, 6, 10, 16) | (3, 4, 6, 24); accumulate onto a
                            DIFFERENT tensor, exact ties included; test_s2d_refusals
  weights_s2d_kernel, weights_s2d_grad_kernel   test_weights_s2d: (cin, cout) (1, 1) | (16, 8) | (512, 512): 16 c k / 256 IS the
                            16384-workgroup cap of sgrid | (520, 512): one wrap

Update steps: reference and bounds (u = 2^-24, g(k) = k u / (1 - k u); no relative tolerance anywhere)
  The reference is the kernel's formula in float64 on the f32 operands and f32 scalars.  1 - beta1, 1 - beta2 and
  1 - ema_decay are exact in f32 for the values used (Sterbenz; asserted), and the `_dyn` factor grad_scale * inv_scale_used
  is one f32 product of two scalars, taken as the kernel forms it.  optim.hip is compiled with contraction: a product
  may fuse into the following sum, which removes a rounding, so the counts below are upper limits.  sqrtf and the f32
  division are correctly rounded in this build (v_sqrt_f32 with its fix-up, v_div_scale / v_div_fmas / v_div_fixup) and
  count as one rounding each.  With reg = (i < n_reg), gs = g s, t = wd w reg, S = |gs| + |t|, kg = 1 + reg:
    gi = gs + t               kg roundings on each term:  e_gi = g(kg) S
  Momentum
    acc' = mom acc + gi       d_acc = g(2) |mom acc| + g(kg + 1) S
    w'   = w - lr acc'        d_w   = g(1) |w| + g(4) |lr mom acc| + g(kg + 3) lr S
  Adam
    m'   = b1 m + c1 gi       d_m   = g(2) |b1 m| + g(kg + 2) c1 S
    v'   = b2 v + c2 gi gi    d_v   = g(2) b2 v + c2 ((|gi| + e_gi)^2 (1 + g(3)) - gi^2)      (c2 gi, the second gi, the sum)
    r    = sqrt(v')           the argument lies in [v' - d_v, v' + d_v] (cut at 0) and the root rounds once:
                              r_lo = sqrt(max(v' - d_v, 0)) (1 - u), r_hi = sqrt(v' + d_v) (1 + u)
    den  = r + eps            den_lo = (r_lo + eps) (1 - u) > 0 (asserted)
    q    = lr m' / den        product and quotient round once each, and |q^ - q| is largest with the numerator up and the
                              denominator down:  d_q = lr (|m'| + d_m) (1 + g(2)) / den_lo - lr |m'| / den
    w'   = w - q              d_w   = d_q + g(1) (|w| + |q| + d_q)
  EMA (both)
    s'   = s - c3 (s - w')    d_s   = g(1) |s| + g(3) c3 (|s| + |w'|) + (1 + g(3)) c3 d_w
  Nothing but the first-order-free forms above is used: no term is dropped.  Operands: |w| in [0.05, 1], g = 1024 times a
  normal times 10^U(-3, 0), |m| >= 1e-3, v = 10^U(-8, 0), ema = w + 0.01 normal; lr 0.01 (Adam) | 0.05, wd 0.1, eps 1e-2 (sqrt(v')
  runs from 1e-4 to 1), factors 1/1536 (plain), 0.3 * (1/768) (dyn), 6.1e-4 (clip g_mul): no operand or product is subnormal.

Pack, s2d: the conversion f32 -> storage type is round-to-nearest-even (v_cvt_f16_f32; v_cvt_pk_bf16_f32 in the bf16
  build, denormals on).  _rne below restates it on the integer bit patterns; tests/test_optim_matrix_host.py pins it to
  _h.  Results are compared bit for bit; where the operand is a NaN the result must be a NaN.  DIRECTED: exact ties on
  both parities of the kept bit, one f32 ulp either side of each, the largest operand that stays finite and the smallest
  that becomes infinite, the storage type's subnormal range with its ties, +-0, +-inf, NaN, both signs throughout.
ocr_sum_squares_f32: squares and sums are formed in double on the device (relative error under (n + 16) 2^-53), the
  result rounds to f32 once: |dev - ref| <= (u + (n + 16) 2^-53) |ref|.

Every row prints `optim <entry> <row> ratio=<|err| / bound>`; a ratio of 0.000 is a bit-exact row.

MEASURED on the MI355X (largest |err| / bound over the rows of an entry; the f16 and the bf16 library gave the same figures:
  their f32 rows are the same code and their 16-bit rows are bit-exact)
  entry                         rows                                                        ratio
  ocr_adam_step                 ema | noema x 17 (n, n_reg) pairs, three steps each; zero   0.994
  ocr_adam_step_dyn             the same                                                    0.993
  ocr_adam_step_clip            the same                                                    0.993
  ocr_momentum_step             as Adam                                                     0.993
  ocr_momentum_step_dyn         as Adam                                                     0.989
  ocr_momentum_step_clip        as Adam                                                     0.991
      per output over all twelve: w 0.994, m / acc 0.938, v 0.875, ema 0.983.  The bounds are worst cases of half an ulp
      per rounding, and a single rounding of a value just above a power of two reaches them: the uncontracted f32
      restatement on the CPU measures 0.934.  skip and refusals rows: 0.000 (bit-identical buffers)
  ocr_sum_squares_f32           n 1 .. 1049603                                              0.961
  ocr_grad_clip_f32, ocr_grad_check_clip_f32   norm, n = 1003                               0.412
  ocr_pack_weights_f16 (21 rows), ocr_pack_weights_batch_f16 (one | many), ocr_pack_weights_small_f16 (6),
  ocr_space_to_depth_f16, ocr_depth_to_space_f16 (3; 24 | 1374 | 1237 of the sums round in f16), ocr_weights_s2d_f32,
  ocr_weights_s2d_grad_f32 (4), ocr_scale_f32, ocr_fill_f32 (4), the init / check / accumulate rows     0.000 (bit-exact)
  No row was over its bound and no defect was found in optim.hip or s2d.hip.
  Time on the MI355X: the file's 116 tests 10.4 s; slowest test_update[adam-plain-ema-n1048581] 0.74 s.
"""
import ctypes
from functools import partial
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matrix_support
from matrix_support import (FL, I64, INVALID_ARG, OK, SZ, U32, UNSUPPORTED, WORKSPACE, Guard, _g, _lib, _ratio, _raw, _rc, _rng,
                            bands_untouched, carve, f32, f64, untouched)
from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

_note = partial(matrix_support._note, "optim")
KIND16 = "f16" if matrix_support.F16 else "bf16"

N_BIG = 256 * 4096 + 5
SIZES = [1, 5, 257, N_BIG]
ODD_REG = {1: 1, 5: 3, 257: 100, N_BIG: 300007}
KINDS, FORMS = ("adam", "mom"), ("plain", "dyn", "clip")
HP = {"adam": NS(lr=f32(0.01), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-2), wd=f32(0.1), decay=f32(0.997)),
      "mom": NS(lr=f32(0.05), mom=f32(0.9), wd=f32(0.1), decay=f32(0.997))}
STATE_NAMES = {"adam": ("w", "m", "v"), "mom": ("w", "m")}          # (Momentum's accumulator travels as m)
INV_SCALE, GRAD_SCALE, INV_USED, G_MUL = f32(1.0 / 1536), f32(0.3), f32(1.0 / 768), f32(6.1e-4)
MUTATIONS = ("reg_le", "reg_lt_minus_1", "no_decay", "decay_after_moments", "eps_in_root", "scale_after_decay", "ema_old_w",
             "ema_decay_swapped", "beta2_for_m", "lr_in_accumulator")


def _nregs(n):
    out = []
    for r in (0, 1, n - 1, n, ODD_REG[n]):
        if r not in out:
            out.append(r)
    return out


UPDATE_ROWS = [(k, f, e, n) for k in KINDS for f in FORMS for e in (True, False) for n in SIZES]


# ------------------------------------------------------------------------------------------------ update: reference
def _operands(kind, n):
    rng = _rng("optim", "update", kind, n)
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    w = sign() * rng.uniform(0.05, 1.0, n)
    o = NS(w=w.astype(f32),
           g=(sign() * (np.abs(rng.standard_normal(n)) + 0.05) * 1024.0 * 10.0 ** rng.uniform(-3, 0, n)).astype(f32),
           m=(sign() * (np.abs(rng.standard_normal(n)) * 0.3 + 1e-3)).astype(f32),
           v=(10.0 ** rng.uniform(-8, 0, n)).astype(f32))
    o.ema = (o.w.astype(f64) + 0.01 * rng.standard_normal(n)).astype(f32)
    return o


def _factor(form):
    """the f32 factor the kernel multiplies g with"""
    return {"plain": INV_SCALE, "dyn": f32(GRAD_SCALE * INV_USED), "clip": G_MUL}[form]


def _one_minus(x):
    c = f32(1) - x
    assert f64(1) - f64(x) == f64(c), "1 - x must be exact in f32 for the scalars of this file"
    return f64(c)


def _reg(idx, n_reg, mut):
    if mut == "reg_le":
        return idx <= n_reg
    if mut == "reg_lt_minus_1":
        return idx < n_reg - 1
    if mut == "no_decay":
        return np.zeros(idx.shape, bool)
    return idx < n_reg


def _ema64(s, w_new, w_old, d_w, c3, mut):
    src = w_old if mut == "ema_old_w" else w_new
    c = 1.0 - c3 if mut == "ema_decay_swapped" else c3
    return s - c * (s - src), _g(1) * np.abs(s) + _g(3) * c * (np.abs(s) + np.abs(src)) + (1 + _g(3)) * c * d_w


def update_ref(kind, o, idx, n_reg, s, ema, mut=None):
    """-> (reference, bound), dicts over w, m, v (Adam only) and ema: the step of `kind` in float64 on the elements `idx`
    of the flat buffer (o holds those elements), and the bounds of the docstring.  `mut` names one of MUTATIONS: the
    same step with that one thing wrong (the bound is then the unmutated formula's and is not used)."""
    H = HP[kind]
    w, g, m = o.w.astype(f64), o.g.astype(f64), o.m.astype(f64)
    reg = _reg(idx, n_reg, mut).astype(f64)
    s, lr, wd, c3 = f64(s), f64(H.lr), f64(H.wd), _one_minus(H.decay)
    kg = 1 + reg
    gs, t = g * s, wd * w * reg
    late = 0.0
    if mut == "scale_after_decay":
        gs, t = g * s, wd * w * reg * s
    if mut == "decay_after_moments":
        late, t = lr * t, 0.0 * t
    gi, S = gs + t, np.abs(gs) + np.abs(t)
    ref, bnd = {}, {}
    if kind == "mom":
        mom = f64(H.mom)
        if mut == "lr_in_accumulator":
            acc = mom * m + lr * gi
            w2 = w - acc - late
        else:
            acc = mom * m + gi
            w2 = w - lr * acc - late
        ref["m"], bnd["m"] = acc, _g(2) * np.abs(mom * m) + _g(kg + 1) * S
        bnd["w"] = _g(1) * np.abs(w) + _g(4) * np.abs(lr * mom * m) + _g(kg + 3) * lr * S
    else:
        v = o.v.astype(f64)
        b1, b2, c1, c2, eps = f64(H.b1), f64(H.b2), _one_minus(H.b1), _one_minus(H.b2), f64(H.eps)
        if mut == "beta2_for_m":
            b1, c1 = b2, c2
        m2 = b1 * m + c1 * gi
        v2 = b2 * v + c2 * gi * gi
        d_m = _g(2) * np.abs(b1 * m) + _g(kg + 2) * c1 * S
        d_v = _g(2) * b2 * v + c2 * ((np.abs(gi) + _g(kg) * S) ** 2 * (1 + _g(3)) - gi * gi)
        den = np.sqrt(v2 + eps) if mut == "eps_in_root" else np.sqrt(v2) + eps
        den_lo = (np.sqrt(np.maximum(v2 - d_v, 0.0)) * (1 - U32) + eps) * (1 - U32)
        assert (den_lo > 0).all()
        q = lr * m2 / den
        d_q = lr * (np.abs(m2) + d_m) * (1 + _g(2)) / den_lo - np.abs(q)
        w2 = w - q - late
        ref["m"], bnd["m"], ref["v"], bnd["v"] = m2, d_m, v2, d_v
        bnd["w"] = d_q + _g(1) * (np.abs(w) + np.abs(q) + d_q)
    ref["w"] = w2
    if ema:
        ref["ema"], bnd["ema"] = _ema64(o.ema.astype(f64), w2, w, bnd["w"], c3, mut)
    return ref, bnd


# ------------------------------------------------------------------------------------------------ update: device
class _Buf:
    """n f32 elements starting `off` elements behind a 16-byte boundary, NaN words in front and behind, inside bands"""

    def __init__(self, n, off, init, device):
        self.guard, t = carve((n + 4,), torch.float32, 64, device)
        self.t, self.slack = t[off:off + n], (t[:off], t[off + n:])
        assert self.t.data_ptr() % 16 == 4 * off
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=f32)))

    def get(self):
        assert bands_untouched(self.guard) and all(untouched(s) for s in self.slack), "written outside the buffer"
        return self.t.cpu().numpy()


def _state(form, device, skip=0):
    """the 8-word block the `_dyn` / `_clip` step reads, between guard bands"""
    if form == "plain":
        return None
    words = np.zeros(8, np.int32)
    fl = words.view(f32)
    if form == "dyn":
        fl[0], fl[1], words[2], words[3] = 768.0, INV_USED, skip, 5
    else:
        fl[0], fl[1], fl[2], words[3], words[4] = G_MUL, 3.25, 0.5, skip, 2
    return Guard((8,), torch.int32, device, words)


def _call(kind, form, B, ema, n, n_reg, st):
    """(entry, arguments) of one step"""
    H = HP[kind]
    e = B["ema"].t if ema else None
    if kind == "adam":
        head = [B["w"].t, B["g"].t, B["m"].t, B["v"].t, e, I64(n), I64(n_reg), FL(H.lr), FL(H.b1), FL(H.b2), FL(H.eps), FL(H.wd)]
        name = "ocr_adam_step"
    else:
        head = [B["w"].t, B["g"].t, B["m"].t, e, I64(n), I64(n_reg), FL(H.lr), FL(H.mom), FL(H.wd)]
        name = "ocr_momentum_step"
    if form == "plain":
        return name, head + [FL(INV_SCALE), FL(H.decay)]
    if form == "dyn":
        return name + "_dyn", head + [FL(GRAD_SCALE), FL(H.decay), st]
    return name + "_clip", head + [FL(H.decay), st]


ENTRY = {(k, f): (("ocr_adam_step", "ocr_momentum_step")[k == "mom"] + {"plain": "", "dyn": "_dyn", "clip": "_clip"}[f])
         for k in KINDS for f in FORMS}
assert sorted(ENTRY.values()) == sorted(["ocr_adam_step", "ocr_adam_step_dyn", "ocr_adam_step_clip", "ocr_momentum_step",
                                         "ocr_momentum_step_dyn", "ocr_momentum_step_clip"])


def _bufs(kind, o, n, j, device):
    names = STATE_NAMES[kind] + ("g", "ema")
    return {k: _Buf(n, (j + b) % 4, getattr(o, k), device) for b, k in enumerate(names)}


def _snapshot(B, st):
    d = {k: b.get().view(np.int32).copy() for k, b in B.items()}
    if st is not None:
        d["state"] = st.raw().copy()
    return d


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind,form,ema,n", UPDATE_ROWS, ids=["%s-%s-%s-n%d" % (k, f, "ema" if e else "noema", n) for k, f, e, n in UPDATE_ROWS])
def test_update(device, kind, form, ema, n):
    L, _ = _lib()
    o0, idx, s = _operands(kind, n), np.arange(n), _factor(form)
    for j, n_reg in enumerate(_nregs(n)):
        B, st = _bufs(kind, o0, n, j, device), _state(form, device)
        before = _snapshot(B, st)
        cur, worst = o0, {}
        for step in range(3):
            ref, bnd = update_ref(kind, cur, idx, n_reg, s, ema)
            name, args = _call(kind, form, B, ema, n, n_reg, st)
            assert _rc(L, name, *args) == OK
            after = _snapshot(B, st)
            for k in ("g", "state") + (() if ema else ("ema",)):          # read-only, or not passed at all
                assert k not in before or np.array_equal(after[k], before[k]), "%s was written" % k
            got = NS(g=cur.g, ema=cur.ema, v=getattr(cur, "v", None))
            for k in ref:
                a = after[k].view(f32)
                worst[k] = max(worst.get(k, 0.0), _ratio(np.abs(a.astype(f64) - ref[k]), bnd[k]))
                setattr(got, k, a)
            cur = got                                                     # the next step starts from the device's state
        print("   ".join("%s %.3f" % kv for kv in sorted(worst.items())))
        _note(name, "%s n=%d n_reg=%d" % ("ema" if ema else "noema", n, n_reg), max(worst.values()))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_update_zero(device, kind, form):
    """g = m = v = 0: behind n_reg the moments stay exactly 0 and w keeps its bits (the EMA still moves towards it); in
    front of n_reg the decay rule alone moves w, inside the bound"""
    L, _ = _lib()
    n, n_reg = 257, 100
    o = _operands(kind, n)
    o.g, o.m, o.v = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    B, st = _bufs(kind, o, n, 1, device), _state(form, device)
    ref, bnd = update_ref(kind, o, np.arange(n), n_reg, _factor(form), True)
    name, args = _call(kind, form, B, True, n, n_reg, st)
    assert _rc(L, name, *args) == OK
    got = {k: B[k].get() for k in ref}
    for k in STATE_NAMES[kind]:
        want = o.w if k == "w" else np.zeros(n, f32)
        assert np.array_equal(got[k][n_reg:].view(np.int32), want[n_reg:].view(np.int32)), k
    assert not np.array_equal(got["w"][:n_reg], o.w[:n_reg])
    _note(name, "zero", max(_ratio(np.abs(got[k].astype(f64) - ref[k]), bnd[k]) for k in ref))


@pytest.mark.parametrize("form", ("dyn", "clip"))
@pytest.mark.parametrize("kind", KINDS)
def test_update_skip(device, kind, form):
    L, _ = _lib()
    for n in (5, N_BIG):
        o = _operands(kind, n)
        B, st = _bufs(kind, o, n, 2, device), _state(form, device, skip=1)
        before = _snapshot(B, st)
        name, args = _call(kind, form, B, True, n, n // 2, st)
        assert _rc(L, name, *args) == OK
        assert _same(before, _snapshot(B, st))
    _note(name, "skip", 0.0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_update_refusals(device, kind, form):
    L, _ = _lib()
    n = 257
    B, st = _bufs(kind, _operands(kind, n), n, 3, device), _state(form, device)
    before = _snapshot(B, st)
    name, good = _call(kind, form, B, True, n, 100, st)
    i_n = next(i for i, a in enumerate(good) if isinstance(a, I64))
    required = [i for i, a in enumerate(good) if isinstance(a, (torch.Tensor, Guard)) and a is not B["ema"].t]
    assert len(required) == len(STATE_NAMES[kind]) + 1 + (form != "plain")
    rows = [(i, None) for i in required] + [(i_n, I64(0)), (i_n + 1, I64(-1)), (i_n + 1, I64(n + 1))]
    for i, bad in rows:
        args = list(good)
        args[i] = bad
        assert _rc(L, name, *args) == INVALID_ARG, (name, i)
    assert _same(before, _snapshot(B, st))
    _note(name, "refusals", 0.0)


# ------------------------------------------------------------------------------------------------ 16-bit rounding
def _rne(x, kind=KIND16):
    """uint16 bit patterns of f32 -> f16 / bf16, round to nearest even, in integer arithmetic; a NaN gives a quiet NaN
    of its sign (compare NaNs with _isnan16, not by bits)"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.int64)
    sign, e, man = (b >> 16) & 0x8000, (b >> 23) & 0xFF, b & 0x7FFFFF
    nan = (e == 255) & (man != 0)
    if kind == "bf16":
        h = ((b & 0x7FFFFFFF) + 0x7FFF + ((b >> 16) & 1)) >> 16           # a carry runs into the exponent, up to infinity
        return np.where(nan, sign | 0x7FC0, sign | h).astype(np.uint16)
    E = e - 127 + 15                                                      # the f16 exponent field before rounding
    full = np.where(e > 0, man | 0x800000, 0)                             # (an f32 subnormal is far below 2^-25)
    shift = np.clip(np.where(E >= 1, 13, 14 - E), 13, 26)                 # bits dropped; 2^-24 is the last f16 unit
    q, rem, half = full >> shift, full & ((1 << shift) - 1), 1 << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    h = ((np.maximum(E, 1) - 1) << 10) + q                                # q carries the implicit bit of a normal number
    h = np.where((E >= 31) | (h >= 0x7C00), 0x7C00, h)
    return np.where(nan, sign | 0x7E00, sign | h).astype(np.uint16)


def _isnan16(h, kind=KIND16):
    h = np.asarray(h).astype(np.int64)
    return ((h & 0x7C00) == 0x7C00) & ((h & 0x3FF) != 0) if kind == "f16" else ((h & 0x7F80) == 0x7F80) & ((h & 0x7F) != 0)


def directed(kind=KIND16):
    """f32 operands at which a wrong rounding mode, a flushed subnormal or a clamped overflow shows (docstring)"""
    s = 13 if kind == "f16" else 16
    half, keep = 1 << (s - 1), 1 << s
    pos = []
    for base in (0x3F800000, 0x40490000 & ~(2 * keep - 1), 0x3A000000, 0x46FF0000 & ~(2 * keep - 1)):
        for parity in (0, keep):
            tie = base | parity | half
            pos += [tie, tie - 1, tie + 1, base | parity, (base | parity) + keep - 1]
    if kind == "f16":
        top = 0x477FE000                                                  # 65504
        pos += [top, top | 0xFFF, top | 0x1000, top + 0x2000, 0x47800000, 0x7F7FFFFF]          # 65519.996 stays, 65520 does not
        unit = 0x33800000                                                 # 2^-24, the f16 subnormal unit
        pos += [unit, unit - 0x800000, unit - 0x800000 + 1, unit - 0x800000 - 1, 0x33000001, 0x32800000, 0x00000001,
                0x00800000, 0x33C00000, 0x34200000, 0x34600000, 0x387FC000, 0x387FDFFF, 0x387FE000, 0x387FF000, 0x38800000,
                0x38000000, 0x38001000, 0x38003000, 0x36A8A000, 0x36A8B000, 0x36A8B001]
    else:
        pos += [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF]           # the last finite bf16; the tie above it is infinite
        pos += [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x00028000, 0x00017FFF, 0x007F7FFF,
                0x007F8000, 0x007FFFFF, 0x00800000, 0x00808000, 0x00400000, 0x00408000, 0x00418000]
    pos += [0x00000000, 0x7F800000]
    bits = np.array(pos + [p | 0x80000000 for p in pos] + [0x7FC0BEEF, 0xFFC00001, 0x7F800001], np.uint32)
    return bits.view(f32)


def _weights(rng, shape):
    """unrounded f32 weights: normals over six decades with the directed set laid over the front (and rotated, so a short
    tensor sees another part of it)"""
    n = int(np.prod(shape))
    w = (rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 1, n)).astype(f32)
    d = np.roll(directed(), -int(rng.integers(0, 1 << 16)))
    k = min(n, d.size)
    w[:k] = d[:k]
    return w.reshape(shape)


def _out16(shape, device):
    return Guard(shape, O.STORAGE, device)


def _bits16(g):
    assert g.ok(), "written outside the buffer"
    return g.t.view(torch.int16).cpu().numpy().view(np.uint16)


def _same16(got, want, what):
    """bit for bit, a NaN for a NaN; 0xFFFF is the fill of _out16: an element the kernel did not write"""
    nan = _isnan16(want)
    assert not (got == 0xFFFF).any(), "%s: %d elements not written" % (what, int((got == 0xFFFF).sum()))
    assert np.array_equal(_isnan16(got), nan), "%s: NaN pattern" % what
    bad = (got != want) & ~nan
    assert not bad.any(), "%s: %d elements differ, first %s: got %s want %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), [hex(v) for v in got[bad][:4]], [hex(v) for v in want[bad][:4]])


PACK_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (40, 24), (1, 33), (33, 1)]
PACK_ROWS = [(ci, co, t) for ci, co in PACK_SHAPES for t in (1, 4, 9)]


def test_rne_is_the_storage_rounding():
    """the integer restatement against torch's conversion (_h): the directed set, its neighbours, and a random sample"""
    x = np.concatenate([directed(), _weights(_rng("optim", "rne"), (4096,))])
    want = torch.from_numpy(x).to(O.STORAGE).view(torch.int16).numpy().view(np.uint16)
    got = _rne(x)
    nan = np.isnan(x)
    assert np.array_equal(_isnan16(got), nan) and np.array_equal(_isnan16(want), nan)
    assert np.array_equal(got[~nan], want[~nan])


@pytest.mark.parametrize("cin,cout,taps", PACK_ROWS, ids=["%dx%d-t%d" % r for r in PACK_ROWS])
def test_pack(device, cin, cout, taps):
    L, _ = _lib()
    w = _weights(_rng("optim", "pack", cin, cout, taps), (taps, cin, cout))
    want = _rne(w)
    wd = Guard(w.shape, torch.float32, device, w)
    for which in ("both", "kc", "ck"):
        kc = _out16((taps, cout, cin), device) if which != "ck" else None
        ck = _out16((taps, cin, cout), device) if which != "kc" else None
        assert _rc(L, "ocr_pack_weights_f16", wd, taps, cin, cout, kc, ck) == OK
        if kc is not None:
            _same16(_bits16(kc), want.transpose(0, 2, 1), "w_kc (%s)" % which)
        if ck is not None:
            _same16(_bits16(ck), want, "w_ck (%s)" % which)
    assert np.array_equal(wd.raw().view(np.int32), w.view(np.int32))
    _note("ocr_pack_weights_f16", "%dx%d taps %d" % (cin, cout, taps), 0.0)


def _batch_items(which):
    """(taps, cin, cout, ld_ck, layouts) per item"""
    if which == "one":
        return [(4, 33, 40, 0, "both")]
    rng = _rng("optim", "pack_batch", "items")
    items = [(1, 7, 5, 0, "both"), (1, 32, 32, 0, "both")]                  # two single-block items in front
    for _ in range(54):
        single = rng.random() < 0.4
        items.append((1 if single else int(rng.choice([1, 4, 9])), int(rng.integers(1, 33 if single else 71)),
                      int(rng.integers(1, 33 if single else 71)), 0, "both"))
    items += [(1, 13, 5, 32, "both"),                                     # a fuse head's [cin][32] copy: ld_ck > cout
              (4, 40, 24, 0, "kc"), (9, 33, 31, 0, "ck"), (1, 1, 1, 0, "both"), (1, 3, 2, 0, "both")]   # single blocks at the end
    return items


@pytest.mark.parametrize("which", ("one", "many"))
def test_pack_batch(device, which):
    L, _ = _lib()
    items = _batch_items(which)
    n = len(items)
    assert n == (1 if which == "one" else 61)
    blocks = [t * -(-ci // 32) * -(-co // 32) for t, ci, co, _, _ in items]
    assert which == "one" or (sum(b == 1 for b in blocks) >= 12 and blocks[0] == blocks[1] == blocks[-1] == blocks[-2] == 1)
    rng = _rng("optim", "pack_batch", which)
    ws, kcs, cks, wants = [], [], [], []
    for t, ci, co, ld, lay in items:
        w = _weights(rng, (t, ci, co))
        ws.append(Guard(w.shape, torch.float32, device, w))
        wants.append(_rne(w))
        kcs.append(_out16((t, co, ci), device) if lay != "ck" else None)
        cks.append(_out16((t, ci, ld or co), device) if lay != "kc" else None)
    vp, ci_t = ctypes.c_void_p * n, ctypes.c_int * n
    ptr = lambda g: None if g is None else g.t.data_ptr()
    nbytes = int(L._fn("ocr_pack_weights_batch_table_bytes", ctypes.c_size_t)(ctypes.c_int(n)))
    assert nbytes >= n * 48 + (n + 1) * 4
    host = np.full(nbytes + 64, 0x5E, np.uint8)
    grid = ctypes.c_int(-1)
    rc = _raw(L, "ocr_pack_weights_batch_table", ctypes.c_int(n), vp(*[ptr(g) for g in ws]), ci_t(*[i[0] for i in items]),
              ci_t(*[i[1] for i in items]), ci_t(*[i[2] for i in items]), vp(*[ptr(g) for g in kcs]), vp(*[ptr(g) for g in cks]),
              ci_t(*[i[3] for i in items]), ctypes.c_void_p(host.ctypes.data), ctypes.byref(grid))
    assert rc == OK and grid.value == sum(blocks) and (host[nbytes:] == 0x5E).all()
    first = host[:nbytes][-(n + 1) * 4:].view(np.int32)
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(blocks)]))
    table = torch.from_numpy(host[:nbytes].copy()).to(device)
    assert _rc(L, "ocr_pack_weights_batch_f16", table, n, grid.value) == OK
    for i, (t, ci, co, ld, lay) in enumerate(items):
        if kcs[i] is not None:
            _same16(_bits16(kcs[i]), wants[i].transpose(0, 2, 1), "item %d w_kc" % i)
        if cks[i] is not None:
            got = _bits16(cks[i])
            _same16(got[:, :, :co], wants[i], "item %d w_ck" % i)
            assert (got[:, :, co:] == 0xFFFF).all(), "item %d: padding columns of w_ck written" % i
        assert ws[i].ok()
    _note("ocr_pack_weights_batch_f16", which, 0.0)


SMALL_ROWS = [(ci, co) for ci in (1, 13) for co in (1, 31, 32)]


@pytest.mark.parametrize("cin,cout", SMALL_ROWS, ids=["%dx%d" % r for r in SMALL_ROWS])
def test_pack_small(device, cin, cout):
    L, _ = _lib()
    w = _weights(_rng("optim", "pack_small", cin, cout), (cin, cout))
    want = np.zeros((cin, 32), np.uint16)
    want[:, :cout] = _rne(w)
    wd, kc, ck = Guard(w.shape, torch.float32, device, w), _out16((32, cin), device), _out16((cin, 32), device)
    assert _rc(L, "ocr_pack_weights_small_f16", wd, cin, cout, kc, ck) == OK
    _same16(_bits16(ck), want, "w_ck32")
    _same16(_bits16(kc), want.T, "w_kc32")
    assert (_bits16(ck)[:, cout:] == 0).all() and (_bits16(kc)[cout:] == 0).all()
    _note("ocr_pack_weights_small_f16", "%dx%d" % (cin, cout), 0.0)


def test_pack_refusals(device):
    L, _ = _lib()
    w = Guard((4, 8, 40), torch.float32, device, np.ones((4, 8, 40), f32))
    kc, ck = _out16((4, 40, 8), device), _out16((4, 8, 40), device)
    for args in ((None, 4, 8, 40, kc, ck), (w, 4, 8, 40, None, None), (w, 0, 8, 40, kc, ck), (w, 4, 0, 40, kc, ck),
                 (w, 4, 8, 0, kc, ck), (w, -1, 8, 40, kc, ck), (w, 4, -8, 40, kc, ck), (w, 4, 8, -40, kc, ck)):
        assert _rc(L, "ocr_pack_weights_f16", *args) == INVALID_ARG, args[1:4]
    for args in ((None, 8, 32, kc, ck), (w, 8, 32, None, ck), (w, 8, 32, kc, None), (w, 8, 33, kc, ck), (w, 8, 40, kc, ck),
                 (w, 0, 32, kc, ck), (w, 8, 0, kc, ck), (w, -8, 32, kc, ck), (w, 8, -1, kc, ck)):
        assert _rc(L, "ocr_pack_weights_small_f16", *args) == INVALID_ARG, args[1:3]
    vp, ci_t = ctypes.c_void_p * 2, ctypes.c_int * 2
    host = np.zeros(256, np.uint8)
    grid = ctypes.c_int(-7)
    P = lambda g: None if g is None else g.t.data_ptr()

    def table(n=2, w1=w, taps=4, cin=8, cout=40, kc1=kc, ck1=ck, ld=0, hostp=host.ctypes.data, gridp=ctypes.byref(grid)):
        return _raw(L, "ocr_pack_weights_batch_table", ctypes.c_int(n), vp(P(w), P(w1)), ci_t(4, taps), ci_t(8, cin), ci_t(40, cout),
                    vp(P(kc), P(kc1)), vp(P(ck), P(ck1)), ci_t(0, ld), ctypes.c_void_p(hostp), gridp)

    assert table() == OK and grid.value == 2 * 4 * 1 * 2
    assert table(ld=40) == OK and table(ld=64) == OK
    for kw in (dict(ld=39), dict(ld=1), dict(n=0), dict(n=-1), dict(w1=None), dict(taps=0), dict(cin=0), dict(cout=0), dict(taps=-4),
               dict(kc1=None, ck1=None), dict(hostp=None), dict(gridp=None)):
        assert table(**kw) == INVALID_ARG, kw
    t = torch.zeros(256, dtype=torch.uint8, device=device)
    for args in ((None, 2, 16), (t, 0, 16), (t, 2, 0), (t, -1, 16), (t, 2, -16)):
        assert _rc(L, "ocr_pack_weights_batch_f16", *args) == INVALID_ARG, args[1:]
    assert kc.untouched() and ck.untouched() and w.ok()
    _note("ocr_pack_weights_f16", "refusals", 0.0)


# ------------------------------------------------------------------------------------------------ sum of squares, scale, fill
SUMSQ_SIZES = [1, 2, 3, 4, 5, 1023, 4 * 256 * 1024 + 4 * 256 + 3]


def _sumsq_ws(L, n):
    return int(L._fn("ocr_sum_squares_workspace", ctypes.c_size_t)(I64(n)))


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sum_squares(device, n):
    L, _ = _lib()
    rng = _rng("optim", "sumsq", n)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 2, n)).astype(f32)
    scale = f32(0.5 * 1e-5)
    nbytes = _sumsq_ws(L, n)
    assert nbytes == 8 * min(max(-(-(n // 4) // 256), 1), 1024)
    guard, xd = carve((n,), torch.float32, 64, device, torch.from_numpy(x))
    bits = []
    for _ in range(2):
        out, ws = Guard((1,), torch.float32, device), Guard((nbytes // 8,), torch.float64, device)
        assert _rc(L, "ocr_sum_squares_f32", xd, I64(n), FL(scale), out, ws, SZ(nbytes)) == OK
        assert ws.ok() and not np.isnan(ws.raw()).any()
        bits.append(out.np().view(np.int32)[0])
    assert bits[0] == bits[1] and bands_untouched(guard)
    ref = f64(scale) * np.sum(x.astype(f64) ** 2)
    ratio = _ratio(abs(f64(out.np()[0]) - ref), (U32 + (n + 16) * 2.0 ** -53) * abs(ref))
    for where, what in ((n - 1, np.inf), (0, np.nan), (n - 1, np.nan), (n // 2, -np.inf)):      # the n & 3 tail and the float4 body
        y = x.copy()
        y[where] = what
        xd.copy_(torch.from_numpy(y))
        out, ws = Guard((1,), torch.float32, device), Guard((nbytes // 8,), torch.float64, device)
        assert _rc(L, "ocr_sum_squares_f32", xd, I64(n), FL(scale), out, ws, SZ(nbytes)) == OK
        r = out.raw()[0]
        assert (np.isnan(r) if np.isnan(what) else r == np.inf) and ws.ok(), (where, what, r)
    _note("ocr_sum_squares_f32", "n=%d" % n, ratio)


def test_sum_squares_refusals(device):
    L, _ = _lib()
    n = 4 * 256 * 3 + 8
    guard, xd = carve((n,), torch.float32, 64, device, 1.0)
    nbytes = _sumsq_ws(L, n)
    assert nbytes == 4 * 8
    out, ws = Guard((1,), torch.float32, device), Guard((4,), torch.float64, device)
    call = lambda *a: _rc(L, "ocr_sum_squares_f32", *a)
    assert call(xd, I64(n), FL(1.0), out, ws, SZ(nbytes - 1)) == WORKSPACE
    assert call(xd, I64(n), FL(1.0), out, ws, SZ(0)) == WORKSPACE
    for off in (1, 2, 3):
        assert call(xd[off:], I64(n - 4), FL(1.0), out, ws, SZ(nbytes)) == INVALID_ARG, off
    for args in ((None, I64(n), FL(1.0), out, ws, SZ(nbytes)), (xd, I64(n), FL(1.0), None, ws, SZ(nbytes)),
                 (xd, I64(n), FL(1.0), out, None, SZ(nbytes)), (xd, I64(0), FL(1.0), out, ws, SZ(nbytes)),
                 (xd, I64(-4), FL(1.0), out, ws, SZ(nbytes))):
        assert call(*args) == INVALID_ARG
    assert out.untouched() and ws.untouched() and bands_untouched(guard)
    assert call(xd, I64(n), FL(1.0), out, ws, SZ(nbytes)) == OK and out.np()[0] == n
    _note("ocr_sum_squares_f32", "refusals", 0.0)


@pytest.mark.parametrize("n", SIZES)
def test_scale_fill(device, n):
    L, _ = _lib()
    x = _operands("mom", n).g
    for off in range(4):
        s = f32([0.3, -1.0 / 768, 1.0, 0.0][off])
        b = _Buf(n, off, x, device)
        assert _rc(L, "ocr_scale_f32", b.t, I64(n), FL(s)) == OK
        assert np.array_equal(b.get().view(np.int32), (x * s).view(np.int32)), (off, float(s))
        value = f32([1.0 / 3, -0.0, np.inf, 2.0 ** -140][off])
        assert _rc(L, "ocr_fill_f32", b.t, I64(n), FL(value)) == OK
        assert np.array_equal(b.get().view(np.int32), np.full(n, value, f32).view(np.int32)), (off, float(value))
        before = b.get().view(np.int32).copy()
        for name in ("ocr_scale_f32", "ocr_fill_f32"):
            for args in ((None, I64(n), FL(2.0)), (b.t, I64(0), FL(2.0)), (b.t, I64(-1), FL(2.0))):
                assert _rc(L, name, *args) == INVALID_ARG
        assert np.array_equal(b.get().view(np.int32), before)
    _note("ocr_scale_f32", "n=%d" % n, 0.0)
    _note("ocr_fill_f32", "n=%d" % n, 0.0)


# ------------------------------------------------------------------------------------------------ the state machines, one row each
def test_state_entries(device):
    """status and one result per entry of the loss-scale, clip and accumulation families"""
    L, _ = _lib()
    n = 1003
    x = _operands("mom", n).g
    guard, g = carve((n,), torch.float32, 64, device, torch.from_numpy(x))
    ls = Guard((8,), torch.int32, device)
    assert _rc(L, "ocr_loss_scale_init", ls, FL(1024.0)) == OK
    words = ls.raw()
    assert words[:2].view(f32).tolist() == [1024.0, 1.0 / 1024] and not words[2:].any()
    assert _rc(L, "ocr_grad_check_f32", g, I64(n), ls, FL(2.0), FL(0.5), 2, FL(1.0), FL(65536.0)) == OK
    words = ls.raw()
    assert words[:2].view(f32).tolist() == [1024.0, 1.0 / 1024] and words[2:].tolist() == [0, 1, 0, 0, 0, 0]     # clean, 1 good step
    cs = Guard((8,), torch.int32, device)
    assert _rc(L, "ocr_grad_clip_init", cs) == OK and not cs.raw().any()
    nbytes = int(L._fn("ocr_grad_clip_workspace", ctypes.c_size_t)(I64(n)))
    assert nbytes == 8
    base = f32(1.0 / 1536)
    norm = np.sqrt(np.sum((x * base).astype(f64) ** 2))                   # the f32 product the optimiser uses, squared and summed in double
    ws = Guard((1,), torch.float64, device)
    assert _rc(L, "ocr_grad_clip_f32", g, I64(n), cs, FL(norm * 0.5), FL(base), ws, SZ(nbytes)) == OK
    c = cs.raw()
    r1 = _ratio(abs(f64(c.view(f32)[1]) - norm), (U32 + (n + 16) * 2.0 ** -53) * norm)
    assert c[3] == 0 and c[4] == 1 and c.view(f32)[2] < 1 and ws.ok()
    _note("ocr_grad_clip_f32", "norm n=%d" % n, r1)
    assert _rc(L, "ocr_grad_check_clip_f32", g, I64(n), ls, FL(2.0), FL(0.5), 2, FL(1.0), FL(65536.0), cs, FL(norm * 4),
               FL(1024.0 / 1536), ws, SZ(nbytes)) == OK
    c, words = cs.raw(), ls.raw()
    r2 = _ratio(abs(f64(c.view(f32)[1]) - norm), (U32 + (n + 16) * 2.0 ** -53) * norm)      # 1024 / 1536 / 1024: the same products
    assert c[3] == 0 and c.view(f32)[2] == 1 and words[:2].view(f32).tolist() == [2048.0, 1.0 / 1024] and words[3] == 0
    _note("ocr_grad_check_clip_f32", "norm n=%d" % n, r2)
    ga = Guard((8,), torch.int32, device)
    assert _rc(L, "ocr_grad_accum_init", ga, 2) == OK and ga.raw().tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
    guard_a, acc = carve((n,), torch.float32, 64, device)
    assert _rc(L, "ocr_grad_accum_f32", g, acc, I64(n), ga) == OK
    assert np.array_equal(acc.cpu().numpy().view(np.int32), x.view(np.int32)) and bands_untouched(guard_a)
    assert _rc(L, "ocr_grad_accum_advance", ga) == OK and ga.raw().tolist() == [1, 2, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(g.cpu().numpy().view(np.int32), x.view(np.int32)) and bands_untouched(guard)
    for name in ("ocr_loss_scale_init", "ocr_grad_check_f32", "ocr_grad_clip_init", "ocr_grad_accum_init", "ocr_grad_accum_f32",
                 "ocr_grad_accum_advance"):
        _note(name, "one row", 0.0)


# ------------------------------------------------------------------------------------------------ space to depth
S2D_SHAPES = [(1, 2, 2, 8), (2, 6, 10, 16), (3, 4, 6, 24)]


def _h16(rng, shape):
    """storage-type values whose pairwise sums are exact in f32: magnitudes within 2^-6 .. 8"""
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-6, 3, shape)
    return matrix_support._h(v)


def _s2d_np(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)


@pytest.mark.parametrize("shape", S2D_SHAPES, ids=["x".join(map(str, s)) for s in S2D_SHAPES])
def test_s2d(device, shape):
    L, _ = _lib()
    n, h, w, c = shape
    rng = _rng("optim", "s2d", shape)
    x, y = _h16(rng, shape), _h16(rng, shape)
    unit = 2.0 ** -11 if matrix_support.F16 else 2.0 ** -8                # half an ulp of 1: exact ties, both parities
    x.flat[:4], y.flat[:4] = [1.0, 1.0 + 2 * unit, -1.0, 1.0 + 2 * unit], [unit, unit, -unit, -unit]
    xs_want = _s2d_np(x)
    xd = Guard(shape, O.STORAGE, device, x)
    xs = _out16(xs_want.shape, device)
    assert _rc(L, "ocr_space_to_depth_f16", xd, n, h, w, c, xs) == OK
    _same16(_bits16(xs), _rne(xs_want), "xs")
    back = _out16(shape, device)
    assert _rc(L, "ocr_depth_to_space_f16", xs, n, h, w, c, back, 0) == OK
    _same16(_bits16(back), _rne(x), "x")
    acc = Guard(shape, O.STORAGE, device, y)                              # a different tensor: the sum rounds
    assert _rc(L, "ocr_depth_to_space_f16", xs, n, h, w, c, acc, 1) == OK
    total = matrix_support._exact32(x.astype(f64) + y.astype(f64))
    rounds = int((matrix_support._h(total) != total).sum())
    assert rounds > total.size // 4 or total.size < 64
    _same16(_bits16(acc), _rne(total), "x + y")
    assert _bits16(acc).flat[:4].tolist() == _rne(np.array([1.0, 1.0 + 4 * unit, -1.0, 1.0], f32)).tolist()    # ties to even
    assert np.array_equal(_bits16(xd), _rne(x)) and np.array_equal(_bits16(xs), _rne(xs_want))
    _note("ocr_space_to_depth_f16", "x".join(map(str, shape)), 0.0)
    _note("ocr_depth_to_space_f16", "x".join(map(str, shape)) + " (%d sums round)" % rounds, 0.0)


def test_s2d_refusals(device):
    L, _ = _lib()
    x, xs = _out16((2, 6, 10, 16), device), _out16((2, 3, 5, 64), device)
    for shape in ((2, 5, 10, 16), (2, 6, 9, 16), (2, 6, 10, 12), (2, 6, 10, 4)):
        assert _rc(L, "ocr_space_to_depth_f16", x, *shape, xs) == UNSUPPORTED, shape
        for accumulate in (0, 1):
            assert _rc(L, "ocr_depth_to_space_f16", xs, *shape, x, accumulate) == UNSUPPORTED, shape
    for shape in ((0, 6, 10, 16), (2, 0, 10, 16), (2, 6, 0, 16), (2, 6, 10, 0), (-2, 6, 10, 16)):
        assert _rc(L, "ocr_space_to_depth_f16", x, *shape, xs) == INVALID_ARG, shape
        assert _rc(L, "ocr_depth_to_space_f16", xs, *shape, x, 0) == INVALID_ARG, shape
    for a, b in ((None, xs), (x, None)):
        assert _rc(L, "ocr_space_to_depth_f16", a, 2, 6, 10, 16, b) == INVALID_ARG
        assert _rc(L, "ocr_depth_to_space_f16", b, 2, 6, 10, 16, a, 0) == INVALID_ARG
    w = Guard((16,), torch.float32, device)
    for name in ("ocr_weights_s2d_f32", "ocr_weights_s2d_grad_f32"):
        for args in ((None, 1, 1, w), (w, 1, 1, None), (w, 0, 1, w), (w, 1, 0, w), (w, -1, 1, w)):
            assert _rc(L, name, *args) == INVALID_ARG
    assert x.untouched() and xs.untouched() and w.untouched()
    _note("ocr_space_to_depth_f16", "refusals", 0.0)


def _tap_source(c, k):
    """for every element of w22 [2][2][4c][k] the flat index of its source in w33 [3][3][c][k], -1 for a zero: the map of
    the header of csrc/s2d.hip, (k2, a) -> tap: (0, 1) -> 0, (1, 0) -> 1, (1, 1) -> 2, nothing for (0, 0)"""
    tap = {(0, 1): 0, (1, 0): 1, (1, 1): 2}
    inner = np.arange(c * k, dtype=np.int64).reshape(c, k)
    src = np.full((2, 2, 2, 2, c, k), -1, np.int64)                       # [ky2][kx2][a][b][ch][co]
    for ky2 in range(2):
        for kx2 in range(2):
            for a in range(2):
                for b in range(2):
                    if (ky2, a) in tap and (kx2, b) in tap:
                        src[ky2, kx2, a, b] = (tap[(ky2, a)] * 3 + tap[(kx2, b)]) * c * k + inner
    return src.reshape(-1)


W_S2D = [(1, 1), (16, 8), (512, 512), (520, 512)]


@pytest.mark.parametrize("c,k", W_S2D, ids=["%dx%d" % r for r in W_S2D])
def test_weights_s2d(device, c, k):
    L, _ = _lib()
    assert (c, k) != (512, 512) or 16 * c * k == 16384 * 256              # the item count IS the cap of sgrid
    rng = _rng("optim", "weights_s2d", c, k)
    src = _tap_source(c, k)
    assert (np.bincount(src[src >= 0], minlength=9 * c * k) == 1).all()   # every 3x3 tap has exactly one image
    w33 = rng.standard_normal(9 * c * k).astype(f32)
    w33[w33 == 0] = 1.0
    w33d = Guard((9 * c * k,), torch.float32, device, w33)
    w22 = Guard((16 * c * k,), torch.float32, device)
    assert _rc(L, "ocr_weights_s2d_f32", w33d, c, k, w22) == OK
    want = np.where(src >= 0, w33[np.maximum(src, 0)], f32(0))
    assert np.array_equal(w22.np().view(np.int32), want.view(np.int32))   # +0 in the (0, 0) phase
    dw22 = rng.standard_normal(16 * c * k).astype(f32)                    # non-zero in the (0, 0) phase too
    dw22d = Guard((16 * c * k,), torch.float32, device, dw22)
    dw33 = Guard((9 * c * k,), torch.float32, device)
    assert _rc(L, "ocr_weights_s2d_grad_f32", dw22d, c, k, dw33) == OK
    adj = np.zeros(9 * c * k, f32)
    adj[src[src >= 0]] = dw22[src >= 0]                                   # the transpose of a one-to-one gather is a gather
    got = dw33.np()
    assert np.array_equal(got.view(np.int32), adj.view(np.int32))
    lhs, rhs = np.dot(want.astype(f64), dw22.astype(f64)), np.dot(w33.astype(f64), got.astype(f64))
    assert abs(lhs - rhs) <= 2.0 ** -40 * np.abs(want.astype(f64) * dw22).sum()      # <A w, d> = <w, A^T d>, sums in double
    assert np.array_equal(w33d.raw().view(np.int32), w33.view(np.int32)) and np.array_equal(dw22d.raw().view(np.int32), dw22.view(np.int32))
    _note("ocr_weights_s2d_f32", "%dx%d" % (c, k), 0.0)
    _note("ocr_weights_s2d_grad_f32", "%dx%d" % (c, k), 0.0)


N_TESTS = (len(UPDATE_ROWS) + 3 * len(KINDS) * len(FORMS) - 2 + 1 + len(PACK_ROWS) + 2 + len(SMALL_ROWS) + 1 + len(SUMSQ_SIZES) + 1
           + len(SIZES) + 1 + len(S2D_SHAPES) + 1 + len(W_S2D))
