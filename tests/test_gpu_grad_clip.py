"""GPU: global-norm gradient clipping decided on the device (train.GradClip; ocr_grad_clip_state in include/ocr_hip.h).

The norm against float64, the range of the f64 sum, the clip rule bit for bit against a NumPy float32 model, non-finite
elements wherever they sit, the fused check + clip pass against ocr_grad_check_f32 and the static pass, the `_clip`
optimiser steps bit for bit against the plain and the `_dyn` ones, and whole training steps: clipping that never bites IS
the unclipped run, clipping that does equals the plain optimiser driven with the factor read back, eager and replayed."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT_I = 0x5A5A5A5A
SENT_D = -7.25e77
GUARD = 16


# ------------------------------------------------------------------------------------------------ helpers
class _Guarded:
    """A clip state block and a partials workspace, each between two sentinel guard bands."""

    def __init__(self, device, n):
        from tensorflow_ocr_amd import ops
        self.slots = ops.grad_clip_workspace(n) // 8
        self._s = torch.full((GUARD + 8 + GUARD,), SENT_I, dtype=torch.int32, device=device)
        self._w = torch.full((GUARD + self.slots + GUARD,), SENT_D, dtype=torch.float64, device=device)
        self.state = self._s[GUARD:GUARD + 8]
        self.ws = self._w[GUARD:GUARD + self.slots]
        ops.grad_clip_init(self.state)

    def intact(self):
        s, w = self._s.cpu().numpy(), self._w.cpu().numpy()
        return bool((s[:GUARD] == SENT_I).all() and (s[GUARD + 8:] == SENT_I).all() and
                    (w[:GUARD] == SENT_D).all() and (w[GUARD + self.slots:] == SENT_D).all())


def _words(state):
    return state.cpu().numpy().copy()


def _read(state):
    w = _words(state)
    f = w.view(F32)
    return {"g_mul": f[0], "norm": f[1], "coef": f[2], "skip": int(w[3]), "clipped_total": int(w[4]),
            "nonfinite_total": int(w[5]), "ticket": int(w[6]), "reserved": int(w[7])}


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.int32)


def _ls_state(device, scale):
    w = np.zeros(8, dtype=np.int32)
    w[0:1].view(F32)[0] = scale
    w[1:2].view(F32)[0] = F32(1) / F32(scale)
    return torch.from_numpy(w).to(device)


LS = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=1000, min_scale=1.0, max_scale=2.0 ** 24)


def _fused(grad, ls, gd, clip_norm, grad_scale, **kw):
    from tensorflow_ocr_amd import ops
    c = dict(LS, **kw)
    ops.grad_check_clip(grad, ls, c["growth_factor"], c["backoff_factor"], c["growth_interval"], c["min_scale"],
                        c["max_scale"], gd.state, clip_norm, grad_scale, gd.ws)


def _grid_cap():
    from tensorflow_ocr_amd import ops
    return ops.grad_clip_workspace(1 << 40) // 8


def _sizes():
    # the size list of tests/test_gpu_loss_scale.py; the last makes more than one grid-stride sweep of the clip
    # kernel's own grid cap AND has an n & 3 tail
    return [1, 3, 4, 5, 255, 256, 257, 4 * 256 * _grid_cap() + 5]


SIZE_IDS = list(range(8))
BAR = 2.5e-7              # the f32 store (2^-24 = 6e-8) plus the f32 product rounding under the root (<= 6e-8), doubled


def _ref_norm(x32, base):
    return float(np.sqrt(np.sum((x32.astype(np.float64) * float(F32(base))) ** 2)))


# ------------------------------------------------------------------------------------- 0. entry points
def test_init_zeroes_the_block_and_bad_arguments_are_refused(device):
    from tensorflow_ocr_amd import _lib, ops
    gd = _Guarded(device, 1000)
    gd.state.fill_(0x7FFFFFFF)
    ops.grad_clip_init(gd.state)
    assert not _words(gd.state).any() and gd.intact()
    x = torch.ones(1000, dtype=torch.float32, device=device)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.OcrHipError):
            ops.grad_clip(x, gd.state, bad, 1.0, gd.ws)
        with pytest.raises(_lib.OcrHipError):
            _fused(x, _ls_state(device, 8.0), gd, bad, 1.0)
    big = torch.ones(4096, dtype=torch.float32, device=device)            # four workgroups, the workspace holds one partial
    with pytest.raises(_lib.OcrHipError, match="(?i)workspace"):
        ops.grad_clip(big, gd.state, 1.0, 1.0, gd.ws)
    with pytest.raises(_lib.OcrHipError):
        _fused(x, _ls_state(device, 8.0), gd, 1.0, 1.0, growth_interval=0)
    st = _lib.stream_ptr()
    null = ctypes.c_void_p(0)
    args = lambda g, n, s, w: (g, ctypes.c_int64(n), s, ctypes.c_float(1.0), ctypes.c_float(1.0), w, ctypes.c_size_t(8), st)
    for a in (args(null, 1000, _lib.ptr(gd.state), _lib.ptr(gd.ws)), args(_lib.ptr(x), 1000, null, _lib.ptr(gd.ws)),
              args(_lib.ptr(x), 1000, _lib.ptr(gd.state), null), args(_lib.ptr(x), 0, _lib.ptr(gd.state), _lib.ptr(gd.ws)),
              args(ctypes.c_void_p(x.data_ptr() + 2), 8, _lib.ptr(gd.state), _lib.ptr(gd.ws))):
        with pytest.raises(_lib.OcrHipError):
            _lib.call("ocr_grad_clip_f32", *a)
    w = torch.zeros(8, device=device)
    with pytest.raises(_lib.OcrHipError):
        ops.adam_step_clip(w, w, w, w, None, 9, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, gd.state)       # n_reg > n
    with pytest.raises(_lib.OcrHipError):
        _lib.call("ocr_momentum_step_clip", _lib.ptr(w), _lib.ptr(w), _lib.ptr(w), null, ctypes.c_int64(8), ctypes.c_int64(0),
                  ctypes.c_float(1e-3), ctypes.c_float(0.9), ctypes.c_float(0.0), ctypes.c_float(0.0), null, st)
    assert not _words(gd.state).any() and gd.intact()                    # a refused call launches nothing


# ------------------------------------------------------------------------------------- 1. norm against float64
# (multiplier of N(0, 1), base): un-scaling a 1024 loss scale; values near the top of what a 2^24 scale produces; and a
# base that is no reciprocal of the multiplier
DISTS = [(1024.0, 1.0 / 1024), (30.0 * 2.0 ** 24, 2.0 ** -24), (65.536, 0.5 / 65536)]


@pytest.mark.parametrize("k", SIZE_IDS)
def test_norm_matches_float64_and_is_reproducible(device, k):
    from tensorflow_ocr_amd import ops
    n = _sizes()[k]
    gd = _Guarded(device, n)
    rng = np.random.default_rng(100 + k)
    worst = 0.0
    for mult, base in DISTS:
        host = (rng.standard_normal(n + 3) * mult).astype(F32)
        buf = torch.from_numpy(host).to(device)
        for off in range(4):
            x = buf[off:off + n]
            assert x.data_ptr() % 16 == 4 * off
            ref = _ref_norm(host[off:off + n], base)
            ops.grad_clip(x, gd.state, 1e30, base, gd.ws)
            a = _words(gd.state)
            ops.grad_clip(x, gd.state, 1e30, base, gd.ws)
            b = _words(gd.state)
            s = _read(gd.state)
            err = abs(float(s["norm"]) - ref) / ref
            worst = max(worst, err)
            print("n %d off %d mult %g: norm %.9g ref %.9g rel %.3g" % (n, off, mult, s["norm"], ref, err))
            assert err <= BAR, (n, off, mult, s, ref)
            assert (a == b).all(), (n, off, a, b)                          # the same bits from call to call
            assert s["skip"] == 0 and s["ticket"] == 0 and s["coef"] == F32(1) and _bits(s["g_mul"]) == _bits(F32(base))
            assert s["clipped_total"] == 0 and s["nonfinite_total"] == 0 and s["reserved"] == 0
            # the fused form sums the same partials: scale 1 / base, grad_scale 1
            ls = _ls_state(device, 1.0 / base)
            gf = _Guarded(device, n)
            _fused(x, ls, gf, 1e30, 1.0)
            assert (_words(gf.state) == a).all() and gf.intact()
    assert gd.intact()
    print("worst relative error at n = %d: %.3g" % (n, worst))


# ------------------------------------------------------------------------------------- 2. range
def test_squares_are_summed_in_f64_and_a_norm_above_f32_is_skipped(device):
    from tensorflow_ocr_amd import ops
    gd = _Guarded(device, 4)
    x = torch.full((4,), 3e19, dtype=torch.float32, device=device)         # sum of squares 3.6e39 > f32's maximum
    ops.grad_clip(x, gd.state, 1e30, 1.0, gd.ws)
    s = _read(gd.state)
    assert s["skip"] == 0 and s["nonfinite_total"] == 0 and abs(float(s["norm"]) - 6e19) <= BAR * 6e19, s
    assert s["coef"] == F32(1) and s["g_mul"] == F32(1)
    x.fill_(3e38)                                                          # finite elements, true norm 6e38 > 3.4e38
    ops.grad_clip(x, gd.state, 1e30, 1.0, gd.ws)
    s = _read(gd.state)
    assert s["skip"] == 1 and s["nonfinite_total"] == 1 and np.isinf(s["norm"]) and s["clipped_total"] == 0, s
    ops.grad_clip(x, gd.state, 1e30, 0.25, gd.ws)                          # 1.5e38: in range again, the skip clears
    s = _read(gd.state)
    assert s["skip"] == 0 and s["nonfinite_total"] == 1 and abs(float(s["norm"]) - 1.5e38) <= BAR * 1.5e38, s
    assert gd.intact()


# ------------------------------------------------------------------------------------- 3. rule
@pytest.mark.parametrize("base", [1.0 / 1024, 0.3, 1.0 / 3.0])
def test_clip_rule_bit_for_bit(device, base):
    from tensorflow_ocr_amd import ops
    n = 1000
    gd = _Guarded(device, n)
    x = torch.from_numpy((np.random.default_rng(7).standard_normal(n) * 50).astype(F32)).to(device)
    ops.grad_clip(x, gd.state, 1e30, base, gd.ws)
    norm = _read(gd.state)["norm"]
    assert np.isfinite(norm) and norm > 0
    clipped = 0
    cases = [("above", F32(norm) * F32(2)), ("equal", F32(norm)), ("just above", np.nextafter(F32(norm), F32(np.inf))),
             ("just below", np.nextafter(F32(norm), F32(0))), ("below", F32(norm) / F32(3)), ("far below", F32(1e-3))]
    for name, c in cases:
        ops.grad_clip(x, gd.state, float(c), base, gd.ws)
        s = _read(gd.state)
        assert _bits(s["norm"]) == _bits(norm) and s["skip"] == 0, (name, s)
        if name in ("above", "equal", "just above"):
            assert _bits(s["coef"]) == _bits(F32(1)), (name, s)
        else:
            clipped += 1
            assert _bits(s["coef"]) == _bits(F32(c) / F32(s["norm"])) and s["coef"] < 1, (name, s)
        assert _bits(s["g_mul"]) == _bits(F32(base) * s["coef"]), (name, s)
        assert s["clipped_total"] == clipped and s["nonfinite_total"] == 0 and s["ticket"] == 0, (name, s)
    assert clipped == 3 and gd.intact()


# ------------------------------------------------------------------------------------- 4. non-finite elements
def _opt_set(device, n, seed, with_ema=True):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(F32)).to(device)
    w, m, v = t(rng.standard_normal(n) * 0.1), t(rng.standard_normal(n) * 0.01), t(rng.uniform(size=n) * 1e-3)
    ema = t(rng.standard_normal(n) * 0.1) if with_ema else None
    return w, m, v, ema


def _same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


ADAM = dict(lr_t=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5, ema_decay=0.99)


@pytest.mark.parametrize("form", ["static", "fused"])
@pytest.mark.parametrize("k", SIZE_IDS)
def test_nonfinite_anywhere_skips_and_the_guarded_steps_write_nothing(device, k, form):
    from tensorflow_ocr_amd import ops
    n = _sizes()[k]
    off = 1                                               # 3 head elements in front of the 16-byte boundary (n allowing)
    head = min(3, n)
    tail = (n - head) & 3
    pos = {0, min(1, n - 1), n // 2, n - 1}               # first, a head element, the body, the last
    if tail:
        pos.add(n - tail)                                 # first element of the tail
    buf = torch.from_numpy(np.random.default_rng(k).standard_normal(n + 3).astype(F32)).to(device)
    x = buf[off:off + n]
    assert x.data_ptr() % 16 == 4
    gd = _Guarded(device, n)
    ls = _ls_state(device, 4.0)
    kw = dict(min_scale=4.0, max_scale=4.0)               # the scale stays put: every fused call sees base 0.25

    def run():
        if form == "static":
            ops.grad_clip(x, gd.state, 1e30, 0.25, gd.ws)
        else:
            _fused(x, ls, gd, 1e30, 1.0, **kw)
    run()
    s = _read(gd.state)
    assert s["skip"] == 0 and s["nonfinite_total"] == 0, s
    count = 0
    for p in sorted(pos):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = x[p].clone()
            x[p] = bad
            run()
            s = _read(gd.state)
            count += 1
            assert s["skip"] == 1 and s["nonfinite_total"] == count and s["ticket"] == 0, (n, p, bad, s)
            assert s["coef"] == 0 and s["g_mul"] == 0 and not np.isfinite(s["norm"]) and s["clipped_total"] == 0, (n, p, bad, s)
            if form == "fused":
                assert int(ls[2]) == 1 and int(ls[5]) == 0 and int(ls[6]) == 0         # the loss-scale state skips too
            if p == n - 1 and bad != bad:
                # the guarded steps, on the poisoned gradients themselves: not one word is written
                n_reg = n // 2
                for seed in (1, 2):
                    a, b = _opt_set(device, n, seed), _opt_set(device, n, seed)
                    if seed == 1:
                        ops.adam_step_clip(b[0], x, b[1], b[2], b[3], n_reg, ADAM["lr_t"], ADAM["beta1"], ADAM["beta2"],
                                           ADAM["eps"], ADAM["wd"], ADAM["ema_decay"], gd.state)
                    else:
                        ops.momentum_step_clip(b[0], x, b[1], b[3], n_reg, 1e-3, 0.9, 5e-4, 0.99, gd.state)
                    assert all(_same_bits(u, v) for u, v in zip(a, b)), (n, seed)
            x[p] = keep
            run()                                          # the next clean call clears the skip
            s = _read(gd.state)
            assert s["skip"] == 0 and s["nonfinite_total"] == count and s["coef"] == F32(1), (n, p, bad, s)
    assert gd.intact()


# ------------------------------------------------------------------------------------- 5. fused form
# clean = 0, poisoned = 1; from 8 with min 2, max 32, interval 3, growth 2, backoff 1/4 (tests/test_gpu_loss_scale.py):
# growth at the third clean step, an overflow, back-off down to min_scale, growth up to max_scale
SCRIPT = [0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1] + [0] * 15


def test_fused_pass_is_the_check_kernel_plus_the_static_clip(device):
    from tensorflow_ocr_amd import ops
    cfg = dict(growth_factor=2.0, backoff_factor=0.25, growth_interval=3, min_scale=2.0, max_scale=32.0)
    n, grad_scale, clip_norm = 1003, 0.5, 2.0
    A = torch.empty(8, dtype=torch.int32, device=device)
    B = torch.empty(8, dtype=torch.int32, device=device)
    ops.loss_scale_init(A, 8.0)
    ops.loss_scale_init(B, 8.0)
    cf, cs = _Guarded(device, n), _Guarded(device, n)
    clean = torch.ones(n + 1, dtype=torch.float32, device=device)[1:]            # 4 bytes past a boundary
    poisoned = [clean.clone(), clean.clone()]
    poisoned[0][777] = float("nan")
    poisoned[1][2] = float("inf")
    scales, clipped, skipped = set(), 0, 0
    for i, found in enumerate(SCRIPT):
        x = poisoned[i & 1] if found else clean
        ops.grad_check(x, A, cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"], cfg["min_scale"], cfg["max_scale"])
        _fused(x, B, cf, clip_norm, grad_scale, **cfg)
        a, b = _words(A), _words(B)
        assert (a == b).all(), (i, a, b)                                      # the loss-scale state, all eight words
        inv_used = b.view(F32)[1]
        scales.add(float(1 / inv_used))
        ops.grad_clip(x, cs.state, clip_norm, float(F32(grad_scale) * inv_used), cs.ws)
        f, s = _words(cf.state), _words(cs.state)
        assert (f == s).all(), (i, _read(cf.state), _read(cs.state))          # the clip state, all eight words
        r = _read(cf.state)
        assert r["skip"] == found == int(b[2])
        skipped += found
        clipped += (not found) and bool(r["coef"] < 1)
        assert r["nonfinite_total"] == skipped and r["clipped_total"] == clipped
    # the script went through growth, back-off to min_scale and growth to max_scale, and clipped some steps but not all
    assert {2.0, 8.0, 16.0, 32.0} <= scales and 0 < clipped < len(SCRIPT) - skipped
    assert cf.intact() and cs.intact()


# ------------------------------------------------------------------------------------- 6. optimisers
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("with_ema", [True, False])
@pytest.mark.parametrize("n", [1, 5, 257, 256 * 4096 + 5])
def test_clip_steps_equal_the_plain_and_dyn_steps_bitwise(device, n, with_ema, grad_scale):
    from tensorflow_ocr_amd import ops
    S = 512.0
    n_reg = n * 3 // 5
    g = torch.from_numpy((np.random.default_rng(n).standard_normal(n) * 300).astype(F32)).to(device)
    ls = _ls_state(device, S)
    static, fused = _Guarded(device, n), _Guarded(device, n)
    A = ADAM

    def adam(kind, state=None, inv=None):
        w, m, v, ema = _opt_set(device, n, 1, with_ema)
        if kind == "plain":
            ops.adam_step(w, g, m, v, ema, n_reg, A["lr_t"], A["beta1"], A["beta2"], A["eps"], A["wd"], inv, A["ema_decay"])
        elif kind == "dyn":
            ops.adam_step_dyn(w, g, m, v, ema, n_reg, A["lr_t"], A["beta1"], A["beta2"], A["eps"], A["wd"], grad_scale,
                              A["ema_decay"], state)
        else:
            ops.adam_step_clip(w, g, m, v, ema, n_reg, A["lr_t"], A["beta1"], A["beta2"], A["eps"], A["wd"], A["ema_decay"], state)
        return w, m, v, ema

    def mom(kind, state=None, inv=None):
        w, m, _, ema = _opt_set(device, n, 2, with_ema)
        if kind == "plain":
            ops.momentum_step(w, g, m, ema, n_reg, 1e-3, 0.9, 5e-4, inv, 0.99)
        elif kind == "dyn":
            ops.momentum_step_dyn(w, g, m, ema, n_reg, 1e-3, 0.9, 5e-4, grad_scale, 0.99, state)
        else:
            ops.momentum_step_clip(w, g, m, ema, n_reg, 1e-3, 0.9, 5e-4, 0.99, state)
        return w, m, ema

    def equal(a, b):
        return all(_same_bits(u, v) for u, v in zip(a, b))
    untouched = _opt_set(device, n, 1, with_ema)
    for clip_norm in (1e30, None):                     # never clipped; then a quarter of the norm
        if clip_norm is None:
            clip_norm = float(_read(static.state)["norm"]) / 4
        ops.grad_clip(g, static.state, clip_norm, grad_scale / S, static.ws)
        _fused(g, ls, fused, clip_norm, grad_scale, min_scale=S, max_scale=S)
        s, f = _read(static.state), _read(fused.state)
        assert (_words(static.state)[:4] == _words(fused.state)[:4]).all() and s["skip"] == 0, (s, f)
        if clip_norm == 1e30:
            assert s["coef"] == F32(1)
            refs = [(adam("plain", inv=grad_scale / S), mom("plain", inv=grad_scale / S)), (adam("dyn", ls), mom("dyn", ls))]
        else:
            assert s["coef"] < 1 and _bits(s["coef"]) == _bits(F32(clip_norm) / s["norm"])
            refs = [(adam("plain", inv=float(s["g_mul"])), mom("plain", inv=float(s["g_mul"])))]
        for st in (static.state, fused.state):
            ca, cm = adam("clip", st), mom("clip", st)
            for ra, rm in refs:
                assert equal(ca, ra) and equal(cm, rm), (n, clip_norm)
            assert not torch.equal(ca[0], untouched[0])                     # (and it did step)
    assert static.intact() and fused.intact()


# ------------------------------------------------------------------------------------- 7, 8, 9. whole steps
# nets/model_vgg_16.model_vgg at full width on 64x64 images, batch 2, as in tests/test_gpu_loss_scale.py
def _loss_scale(mode):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    return 1024.0 if mode == "numeric" else DynamicLossScale(init_scale=1024, growth_interval=1000)


def _make(device, mode, replay, clip_norm, opt_cls=None, learning_rate=1e-3):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=_loss_scale(mode), seed=3)
    batch = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(5), 2, 64)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    kw = {} if clip_norm is None else {"clip_norm": clip_norm}
    return g, batch, TrainStep(g, fl, lambda gr: (opt_cls or AdamOptimizer)(gr, learning_rate=learning_rate, **kw), replay=replay)


def _snapshot(g, step):
    return {"w": g.store.flat.clone(), "m": step.opt.m.clone(), "v": step.opt.v.clone(), "ema": step.opt.ema.clone()}


def _recorded(step, batch):
    """Run one step and return the names of the C-ABI calls its host callbacks (optimiser, re-pack) made: in a replayed
    step the plan's own entries are issued directly, everything else goes through `_lib.call` and is recorded here."""
    from tensorflow_ocr_amd import _lib
    if step.plan is None:                      # an eager (or the recording) step installs a recorder of its own
        return step(*batch), None
    rec = _lib.Recorder()
    _lib.RECORDER = rec
    try:
        loss = step(*batch)
    finally:
        _lib.RECORDER = None
    return loss, [e[3] for e in rec.entries if e[0] == "c"]


NEW = ("ocr_grad_clip_f32", "ocr_grad_check_clip_f32", "ocr_adam_step_clip", "ocr_momentum_step_clip", "ocr_grad_clip_init")


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("mode", ["numeric", "dynamic"])
def test_clipping_that_never_bites_is_the_unclipped_run_bit_for_bit(device, mode, replay):
    g0, b0, s0 = _make(device, mode, replay, None)
    g1, b1, s1 = _make(device, mode, replay, 1e30)
    steps = 5 if replay else 3                   # replayed: steps 1-2 eager, 3 recorded, 4-5 replayed
    l0, l1 = [], []
    for k in range(steps):
        if k == steps - 1:
            a, n0 = _recorded(s0, b0)
            b, n1 = _recorded(s1, b1)
            l0.append(a.item())
            l1.append(b.item())
        else:
            l0.append(s0(*b0).item())
            l1.append(s1(*b1).item())
    assert (s0.plan is not None) == replay and (s1.plan is not None) == replay
    assert l0 == l1
    a, b = _snapshot(g0, s0), _snapshot(g1, s1)
    for name in a:
        assert _same_bits(a[name], b[name]), name
    assert s1.opt.clipped_steps() == 0 and s1.opt.nonfinite_steps() == 0 and 0 < s1.opt.grad_norm() < float("inf")
    if replay:
        # 9: the default launches what it launched before; with clip_norm the pass and the guarded step take their place
        base = ["ocr_adam_step"] if mode == "numeric" else ["ocr_grad_check_f32", "ocr_adam_step_dyn"]
        clip = ["ocr_grad_clip_f32" if mode == "numeric" else "ocr_grad_check_clip_f32", "ocr_adam_step_clip"]
        assert n0[:len(base)] == base and not [x for x in n0 if x in NEW], n0
        assert n1[:2] == clip and n1[2:] == n0[len(base):], (n0, n1)


@pytest.mark.parametrize("which", ["adam", "momentum"])
@pytest.mark.parametrize("mode", ["numeric", "dynamic"])
def test_default_optimisers_launch_none_of_the_new_entry_points(device, mode, which):
    from tensorflow_ocr_amd import _lib, graph as G
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer

    def names(clip_norm):
        g = G.Graph(device, loss_scale=_loss_scale(mode), seed=2)
        with g.variable_scope("feature_fusion"):
            g.get_variable("Conv/weights", (1, 1, 4, 3), G.xavier_uniform(g.rng), regularized=True)
            g.get_variable("Conv/biases", (3,), G.constant(0.5))
        opt = (AdamOptimizer if which == "adam" else MomentumOptimizer)(g, clip_norm=clip_norm)
        if g.loss_scaler is not None:
            g.loss_scaler.state                    # (created outside the recording, as in a real step)
        rec = _lib.Recorder()
        _lib.RECORDER = rec
        try:
            opt.apply_gradients()
        finally:
            _lib.RECORDER = None
        return [e[3] for e in rec.entries]
    step = "ocr_adam_step" if which == "adam" else "ocr_momentum_step"
    assert names(None) == ([step] if mode == "numeric" else ["ocr_grad_check_f32", step + "_dyn"])
    assert names(3.0) == ["ocr_grad_clip_f32" if mode == "numeric" else "ocr_grad_check_clip_f32", step + "_clip"]


def _plain_adam():
    """AdamOptimizer whose step is the PLAIN kernel with `inv_loss_scale = self.g_mul()` (a device read the test
    supplies: the factor the clipped twin has just used): the third twin of the real-clipping test."""
    import math
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.train import AdamOptimizer

    class PlainAdam(AdamOptimizer):
        g_mul = None

        def apply_gradients(self, grad_scale=1.0):
            st = self.g.store
            t = self.global_step + 1
            lr_t = self.learning_rate() * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
            ema_d = min(self.mad, (1.0 + self.global_step) / (10.0 + self.global_step)) if self.mad else 0.0
            ops.adam_step(st.flat, st.flat_grad, self.m, self.v, self.ema, st.n_reg, lr_t, self.b1, self.b2, self.eps, self.wd,
                          type(self).g_mul(), ema_d)
            st.version += 1
            self.global_step += 1
    return PlainAdam


@pytest.mark.parametrize("mode", ["numeric", "dynamic"])
def test_real_clipping_equals_the_plain_step_with_the_factor_read_back(device, mode):
    """Every one of the five steps must be clipped at norm0 / 4, so the gradient norm must stay above a quarter of its
    first value.  Adam's first updates move EVERY weight by about the learning rate whatever the gradient's size (m / sqrt(v)
    is +-1 at t = 1) and all in the descent direction, and the freshly initialised weights are of the order 1e-2: at the
    1e-3 of the other whole-step tests the second gradient has a fifth of the first one's norm (on an MI355X: 152.4, then
    31.7).  The oracle's float32 model_vgg under sign steps of the same size, on the CPU, shows the same fall (154.6, 32.8)
    and gives, over five steps, a smallest norm of 98.6 at 1e-5 and of 113.0 at 1e-6: three times norm0 / 4.  At 1e-6 an
    update is still a thousand ulps of a weight, and m and v carry g_mul whatever the rate."""
    lr = 1e-6
    g, b, s = _make(device, mode, False, 1e30, learning_rate=lr)
    s(*b)
    norm0 = s.opt.grad_norm()
    assert 0 < norm0 < float("inf")
    c = norm0 / 4
    gr, br, sr = _make(device, mode, True, c, learning_rate=lr)  # replayed
    ge, be, se = _make(device, mode, False, c, learning_rate=lr) # eager
    plain = _plain_adam()
    plain.g_mul = staticmethod(lambda: float(_read(sr.opt.clip.state)["g_mul"]))
    gp, bp, sp = _make(device, mode, False, None, opt_cls=plain, learning_rate=lr)
    steps, launches = 5, []
    for k in range(steps):
        _, names = _recorded(sr, br)
        launches.append(names)
        se(*be)
        r = _read(sr.opt.clip.state)
        # the norm of what the optimiser used: flat_grad * base in float64
        base = F32(1.0 / 1024) if mode == "numeric" else _words(gr.loss_scaler.state).view(F32)[1]
        ref = float(torch.sqrt(torch.sum((gr.store.flat_grad.double() * float(base)) ** 2)).item())
        print("step %d: norm %.9g ref %.9g coef %.6g" % (k, r["norm"], ref, r["coef"]))
        assert abs(sr.opt.grad_norm() - ref) <= BAR * ref, (k, r, ref)
        assert r["skip"] == 0 and r["coef"] < 1 and _bits(r["g_mul"]) == _bits(F32(base) * r["coef"]), (k, r)
        assert (_words(se.opt.clip.state) == _words(sr.opt.clip.state)).all()
        sp(*bp)
        a, p, e = _snapshot(gr, sr), _snapshot(gp, sp), _snapshot(ge, se)
        for name in a:
            assert _same_bits(a[name], p[name]), (k, name)
            assert _same_bits(a[name], e[name]), (k, name)
    assert sr.plan is not None and se.plan is None
    assert sr.opt.clipped_steps() == se.opt.clipped_steps() == steps and sr.opt.nonfinite_steps() == 0
    first = ["ocr_grad_clip_f32" if mode == "numeric" else "ocr_grad_check_clip_f32", "ocr_adam_step_clip"]
    assert launches[:3] == [None] * 3 and launches[3][:2] == first, launches
    assert launches[3] == launches[4]                            # the replayed steps: the same launches every time
