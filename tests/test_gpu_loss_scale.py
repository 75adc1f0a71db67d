"""GPU: dynamic loss scaling decided on the device (graph.DynamicLossScale; ocr_loss_scale_state in include/ocr_hip.h).

The check kernel's detection and its state machine against a pure-Python model, the guarded optimiser steps and the
`_dyn` loss gradients bit for bit against the static kernels, and whole training steps: without an overflow the dynamic
mode IS the static one; with one, steps are skipped until the scale has backed off, nothing is damaged, and an eager and
a replayed run end in the same bits (nothing of the decision is frozen into the recorded plan)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32MAX = float(np.finfo(np.float32).max)           # 3.4028235e38


# ------------------------------------------------------------------------------------------------ helpers
def _state(device, scale, skip=0, good=0, skipped=0, inv_used=None):
    """An ocr_loss_scale_state written from the host: [scale, inv_scale_used, skip, good_steps, skipped_total, 0, 0, 0]."""
    w = np.zeros(8, dtype=np.int32)
    w[0:1].view(np.float32)[0] = scale
    w[1:2].view(np.float32)[0] = (np.float32(1) / np.float32(scale)) if inv_used is None else inv_used
    w[2], w[3], w[4] = skip, good, skipped
    return torch.from_numpy(w).to(device)


def _read(state):
    w = state.cpu().numpy()
    f = w.view(np.float32)
    return {"scale": float(f[0]), "inv_scale_used": float(f[1]), "skip": int(w[2]), "good_steps": int(w[3]),
            "skipped_total": int(w[4]), "found": int(w[5]), "ticket": int(w[6])}


CFG = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=1000, min_scale=1.0, max_scale=2.0 ** 24)


def _check(grad, state, **kw):
    from tensorflow_ocr_amd import ops
    c = dict(CFG, **kw)
    ops.grad_check(grad, state, c["growth_factor"], c["backoff_factor"], c["growth_interval"], c["min_scale"], c["max_scale"])


# ------------------------------------------------------------------------------------- 1. detection
SIZES = [1, 3, 4, 5, 255, 256, 257, 4 * 256 * 4096 + 5]     # the last: more than one grid-stride sweep of the 4096-block
                                                            # cap (the loop iterates) AND an n & 3 tail


def _positions(n):
    pos = {0, n - 1, n // 2}
    if n & 3:
        pos.add(n - (n & 3))              # first element of the n & 3 tail
    return sorted(pos)


@pytest.mark.parametrize("n", SIZES)
def test_check_kernel_flags_every_nonfinite_wherever_it_sits(device, n):
    """One of +inf / -inf / NaN at the first element, the last, inside the n & 3 tail and in the middle, on a 16-byte
    aligned buffer and on slices that start 4, 8 and 12 bytes past a boundary (the entry point takes any 4-byte aligned
    pointer: head and tail elements are read one by one).  The largest finite values, denormals and -0.0 are clean."""
    rng = np.random.default_rng(n)
    base = torch.from_numpy(rng.standard_normal(n + 3).astype(np.float32)).to(device)
    # clean values that must NOT be flagged, spread over head, middle and tail
    clean = [F32MAX, -F32MAX, 1e-45, -1e-45, float(np.float32(1.1754942e-38)), -0.0]
    for k, v in enumerate(clean):
        base[(k * 7919) % (n + 3)] = v
    base[0], base[n + 2] = F32MAX, -F32MAX
    offsets = (0, 1, 2, 3) if n < 1000 else (0, 1)
    state = _state(device, 1024.0)
    for off in offsets:
        x = base[off:off + n]
        assert x.data_ptr() % 16 == 4 * off
        _check(x, state)
        s = _read(state)
        assert s["skip"] == 0 and s["found"] == 0 and s["ticket"] == 0, (n, off, s)
        for p in _positions(n):
            for bad in (float("inf"), float("-inf"), float("nan")):
                keep = x[p].clone()
                x[p] = bad
                _check(x, state)
                s = _read(state)
                x[p] = keep
                assert s["skip"] == 1 and s["found"] == 0 and s["ticket"] == 0, (n, off, p, bad, s)
        _check(x, state)
        assert _read(state)["skip"] == 0            # and clean again


def test_check_kernel_rejects_what_it_cannot_read(device):
    from tensorflow_ocr_amd import _lib, ops
    state = _state(device, 2.0)
    x = torch.zeros(16, dtype=torch.float32, device=device)
    with pytest.raises(_lib.OcrHipError):
        _check(x, state, growth_interval=0)
    with pytest.raises(_lib.OcrHipError):
        _check(x, state, min_scale=4.0, max_scale=2.0)
    with pytest.raises(_lib.OcrHipError):
        ops.loss_scale_init(state, 0.0)
    u8 = torch.zeros(64, dtype=torch.uint8, device=device)
    with pytest.raises(_lib.OcrHipError):           # 2 bytes past a word: not an f32 pointer
        _lib.call("ocr_grad_check_f32", ctypes.c_void_p(u8.data_ptr() + 2), ctypes.c_int64(4), _lib.ptr(state),
                  ctypes.c_float(2.0), ctypes.c_float(0.5), ctypes.c_int(3), ctypes.c_float(1.0), ctypes.c_float(4.0),
                  _lib.stream_ptr())


# ------------------------------------------------------------------------------------- 2. state machine
class _Model:
    """The transition of ocr_grad_check_f32 in float32, as include/ocr_hip.h states it."""

    def __init__(self, init, growth, backoff, interval, lo, hi):
        f = np.float32
        self.scale, self.growth, self.backoff, self.lo, self.hi = f(init), f(growth), f(backoff), f(lo), f(hi)
        self.interval = interval
        self.inv_used, self.skip, self.good, self.skipped = f(1) / f(init), 0, 0, 0

    def step(self, found):
        f = np.float32
        self.inv_used = f(1) / self.scale
        if found:
            self.skip = 1
            self.scale = max(f(self.scale * self.backoff), self.lo)
            self.good = 0
            self.skipped += 1
        else:
            self.skip = 0
            self.good += 1
            if self.good == self.interval:
                self.scale = min(f(self.scale * self.growth), self.hi)
                self.good = 0

    def dict(self):
        return {"scale": float(self.scale), "inv_scale_used": float(self.inv_used), "skip": self.skip,
                "good_steps": self.good, "skipped_total": self.skipped, "found": 0, "ticket": 0}


# clean = 0, poisoned = 1.  From 8 with min 2, max 32, interval 3, growth 2, backoff 1/4:
#   0 0 0  growth exactly at the third clean step (16)
#   0 0 1  backoff with two clean steps counted (4): the count starts again ...
#   0 0 0  ... so growth comes three steps later, not one (8)
#   1 1    2, then 0.5 clamped at min_scale (2)
#   0 x 15 4, 8, 16, 32, then 64 clamped at max_scale (32)
SCRIPT = [0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1] + [0] * 15


def test_state_machine_follows_the_model_exactly(device):
    from tensorflow_ocr_amd import ops
    init, growth, backoff, interval, lo, hi = 8.0, 2.0, 0.25, 3, 2.0, 32.0
    state = torch.empty(8, dtype=torch.int32, device=device)
    ops.loss_scale_init(state, init)
    m = _Model(init, growth, backoff, interval, lo, hi)
    assert _read(state) == m.dict()
    clean = torch.ones(1000, dtype=torch.float32, device=device)
    poisoned = clean.clone()
    poisoned[777] = float("nan")
    seen = set()
    for k, found in enumerate(SCRIPT):
        before = m.scale
        ops.grad_check(poisoned if found else clean, state, growth, backoff, interval, lo, hi)
        m.step(found)
        assert _read(state) == m.dict(), (k, _read(state), m.dict())       # exact: every value is a float32 / an integer
        if m.scale > before:
            seen.add("growth")
        if found and m.scale < before:
            seen.add("backoff")
        if found and m.scale == lo and before * np.float32(backoff) < lo:
            seen.add("min clamp")
        if not found and m.good == 0 and m.scale == hi and before == hi:
            seen.add("max clamp")
    assert len(SCRIPT) >= 12 and seen == {"growth", "backoff", "min clamp", "max clamp"}, seen
    # a scale that is no power of two: the reciprocal and the products are single float32 operations, the model's too
    ops.loss_scale_init(state, 1000.0)
    m = _Model(1000.0, 1.7, 0.3, 2, 1.0, 1e6)
    for found in (0, 0, 1, 0, 1, 0, 0):
        ops.grad_check(poisoned if found else clean, state, 1.7, 0.3, 2, 1.0, 1e6)
        m.step(found)
        assert _read(state) == m.dict()


# ------------------------------------------------------------------------------------- 3. guarded optimisers
def _opt_buffers(device, seed, with_ema):
    rng = np.random.default_rng(seed)
    n = 1000
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(device)
    w = t(rng.standard_normal(n) * 0.1)
    g = t(rng.standard_normal(n) * 300.0)                 # "scaled" gradients
    m = t(rng.standard_normal(n) * 0.01)
    v = t(rng.uniform(size=n) * 1e-3)
    ema = t(rng.standard_normal(n) * 0.1) if with_ema else None
    return w, g, m, v, ema


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("with_ema", [True, False])
def test_guarded_steps_equal_the_static_steps_bitwise_and_skip_writes_nothing(device, with_ema, grad_scale):
    """skip = 0, scale S = 2^9: the guarded kernels multiply g by grad_scale * (1 / S), the static ones by the host's
    grad_scale / S.  With S and grad_scale powers of two both factorings of the reciprocal are exact, so the two
    factors are the same float32 and every output must agree bit for bit.  skip = 1: nothing is written."""
    from tensorflow_ocr_amd import ops
    S, n_reg = 512.0, 600
    adam = dict(lr_t=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5, ema_decay=0.99)
    for skip in (0, 1):
        state = _state(device, S * 2 if skip else S, skip=skip, inv_used=np.float32(1.0 / S))   # the scale word itself is not read
        # Adam
        a, b = _opt_buffers(device, 1, with_ema), _opt_buffers(device, 1, with_ema)
        ops.adam_step(a[0], a[1], a[2], a[3], a[4], n_reg, adam["lr_t"], adam["beta1"], adam["beta2"], adam["eps"], adam["wd"],
                      grad_scale / S, adam["ema_decay"])
        ops.adam_step_dyn(b[0], b[1], b[2], b[3], b[4], n_reg, adam["lr_t"], adam["beta1"], adam["beta2"], adam["eps"],
                          adam["wd"], grad_scale, adam["ema_decay"], state)
        ref = a if not skip else _opt_buffers(device, 1, with_ema)           # skipped: the initial values
        for name, x, y in zip("w g m v ema".split(), ref, b):
            if x is not None:
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("adam", skip, name)
        if not skip:
            assert not torch.equal(b[0], _opt_buffers(device, 1, with_ema)[0])      # (and it did step)
        # Momentum
        a, b = _opt_buffers(device, 2, with_ema), _opt_buffers(device, 2, with_ema)
        ops.momentum_step(a[0], a[1], a[2], a[4], n_reg, 1e-3, 0.9, 5e-4, grad_scale / S, 0.99)
        ops.momentum_step_dyn(b[0], b[1], b[2], b[4], n_reg, 1e-3, 0.9, 5e-4, grad_scale, 0.99, state)
        ref = a if not skip else _opt_buffers(device, 2, with_ema)
        for name, x, y in zip("w g acc v ema".split(), ref, b):
            if x is not None:
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("momentum", skip, name)
        assert _read(state)["skip"] == skip                                   # the state is read only


# ------------------------------------------------------------------------------------- 4. loss gradients
S_LOSS = 256.0
GRAD_SCALES = [1.0, 0.5, 1.0 / 3.0]       # x 256 commutes with the rounding to float32: host and device seeds are one value


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("pc,G", [(2, 16), (1, 8), (2, 2), (1, 1)])
def test_dice_bwd_dyn_equals_static_bitwise(device, pc, G):
    """pc pixel channels, G link channels per direction, P = 2*16*16: (2, 16) and (1, 8) run the general kernel, (2, 2) and
    (1, 1) — the 2 + 16 and 1 + 8 channel heads of the nets — the two specialised ones."""
    from tensorflow_ocr_amd import ops
    rng = np.random.default_rng(pc)
    P = 2 * 16 * 16
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    ytp, ytl = t(rng.uniform(size=P) < 0.3), t(rng.uniform(size=(P, 8)) < 0.3)
    ypp, ypl, mask = t(rng.uniform(size=(P, pc))), t(rng.uniform(size=(P, 8 * G))), t(rng.uniform(size=P) < 0.9)
    sums, out = torch.empty(27, device=device), torch.empty(10, device=device)
    ops.dice_loss_fwd(ytp, ypp, ytl, ypl, mask, sums, out, ops.Workspace(device, 1 << 20))
    state = _state(device, S_LOSS)
    scale = state[0:1].view(torch.float32)
    for gs in GRAD_SCALES:
        d0, l0 = torch.zeros_like(ypp), torch.zeros_like(ypl)
        d1, l1 = torch.zeros_like(ypp), torch.zeros_like(ypl)
        ops.dice_loss_bwd(ytp, ytl, mask, sums, gs * S_LOSS, d0, l0)
        ops.dice_loss_bwd_dyn(ytp, ytl, mask, sums, gs, scale, d1, l1)
        assert _bits_equal(d0, d1) and _bits_equal(l0, l1) and float(l0.abs().max()) > 0


@pytest.mark.parametrize("pixel_rule", [0, 1, 2])
def test_softmax_bwd_dyn_equals_static_bitwise(device, pixel_rule):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd._lib import SoftmaxLossDesc
    rng = np.random.default_rng(10 + pixel_rule)
    n, hw = 2, 16 * 16
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    pl, ll = t(rng.standard_normal((n, hw, 2)) * 2), t(rng.standard_normal((n, hw, 16)) * 2)
    plab, llab = t(rng.uniform(size=(n, hw)) < 0.25), t(rng.uniform(size=(n, hw, 8)) < 0.4)
    # rule 0 = nets/model.py (OHNM), 1 = model_vgg_16.ohem_loss, 2 = PixelLinkNet.build_loss with focal links
    d = SoftmaxLossDesc(n, hw, pixel_rule, 1 if pixel_rule == 2 else 0, 0 if pixel_rule == 2 else 1,
                        1 if pixel_rule == 2 else 0, 3.0, 0.25, 2.0)
    thr, sums, out = torch.zeros(n, device=device), torch.empty(34, device=device), torch.empty(10, device=device)
    ops.softmax_loss_fwd(d, pl, ll, plab, llab, thr, sums, out, ops.Workspace(device, 1 << 20))
    state = _state(device, S_LOSS)
    scale = state[0:1].view(torch.float32)
    for gs in GRAD_SCALES:
        a0, b0, a1, b1 = torch.zeros_like(pl), torch.zeros_like(ll), torch.zeros_like(pl), torch.zeros_like(ll)
        ops.softmax_loss_bwd(d, pl, ll, plab, llab, thr, sums, gs * S_LOSS, a0, b0)
        ops.softmax_loss_bwd_dyn(d, pl, ll, plab, llab, thr, sums, gs, scale, a1, b1)
        assert _bits_equal(a0, a1) and _bits_equal(b0, b1)
        assert float(a0.abs().max()) > 0 and float(b0.abs().max()) > 0


def test_link_ce_bwd_dyn_equals_static_bitwise(device):
    from tensorflow_ocr_amd import ops
    rng = np.random.default_rng(20)
    P = 512
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    gt, pred, W = t(rng.uniform(size=P) < 0.4), t(rng.standard_normal((P, 2)) * 2), t(rng.uniform(size=P) < 0.5)
    sums, out = torch.empty(4, device=device), torch.empty(1, device=device)
    ops.link_ce_fwd(gt, 1, pred, 2, W, P, sums, out, ops.Workspace(device, 1 << 20))
    state = _state(device, S_LOSS)
    scale = state[0:1].view(torch.float32)
    for gs in GRAD_SCALES:
        d0, d1 = torch.zeros_like(pred), torch.zeros_like(pred)
        ops.link_ce_bwd(gt, 1, pred, 2, W, P, sums, gs * S_LOSS, d0, 2)
        ops.link_ce_bwd_dyn(gt, 1, pred, 2, W, P, sums, gs, scale, d1, 2)
        assert _bits_equal(d0, d1) and float(d0.abs().max()) > 0


def test_loss_call_sites_take_the_scale_from_the_device(device):
    """The three host call sites (model_vgg_16.loss, losses.softmax_loss, model_vgg_16.cal_link_loss): a graph with a
    DynamicLossScale seeds the backward pass with 1 / loss_div times the DEVICE scale — change the device word and the
    gradient follows, with nothing rebuilt on the host."""
    from tensorflow_ocr_amd import losses
    from tensorflow_ocr_amd.graph import Act, DynamicLossScale, Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    rng = np.random.default_rng(30)
    n, h, w = 2, 16, 16
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    arrays = dict(pl=t(rng.standard_normal((n, h, w, 2))), ll=t(rng.standard_normal((n, h, w, 16))),
                  pp=t(rng.uniform(size=(n, h, w, 2))), lp=t(rng.uniform(size=(n, h, w, 16))),
                  plab=t(rng.uniform(size=(n, h, w, 1)) < 0.3), llab=t(rng.uniform(size=(n, h, w, 8)) < 0.4),
                  mask=t(rng.uniform(size=(n, h, w, 1)) < 0.9))

    def grads(g):
        a = arrays
        out = []
        hp, hl = Act(a["pl"]), Act(a["ll"])
        losses.softmax_loss(g, hp, hl, a["plab"], a["llab"], pixel_rule=0, label_rule=0, link_gate=True)
        dp, dl = Act(a["pp"]), Act(a["lp"])
        M.loss(a["plab"], dp, a["llab"], dl, a["mask"], graph=g)
        lk = Act(a["ll"][..., 0:2].contiguous())
        M.cal_link_loss(a["llab"][..., 0], lk, a["plab"].reshape(-1), graph=g)
        g.backward()
        for x in (hp, hl, dp, dl, lk):
            out.append(x.grad.clone())
        return out
    gs = Graph(device, loss_scale=64.0)
    gs.loss_div = 2.0
    gd = Graph(device, loss_scale=DynamicLossScale(init_scale=64.0))
    gd.loss_div = 2.0
    ref = grads(gs)
    for a, b in zip(ref, grads(gd)):
        assert _bits_equal(a, b)
    gd.loss_scaler.load_state_dict({"scale": 128.0, "good_steps": 0})        # (writes the device word)
    assert gd.loss_scaler.scale() == 128.0
    for a, b in zip(ref, grads(gd)):
        assert _bits_equal(a * 2, b)


# ------------------------------------------------------------------------------------- 5, 6. whole steps
# The net: nets/model_vgg_16.model_vgg on 64x64 images, batch 2 — the step tests/test_gpu_train_step.py records.  (The
# package builds model_vgg at full width only; the width/8 variant behind tests/golden/model_vgg_w8_64.npz exists in the
# oracle alone, so the full-width net at the same 64x64 size stands in for it.)
def _make(device, loss_scale, replay):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=loss_scale, seed=3)
    batch = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(5), 2, 64)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, batch, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3), replay=replay)


def _snapshot(g, step):
    return {"w": g.store.flat.clone(), "m": step.opt.m.clone(), "v": step.opt.v.clone(), "ema": step.opt.ema.clone()}


def test_training_without_overflow_is_the_static_path_bit_for_bit(device):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    gs, bs, ss = _make(device, 1024.0, True)
    gd, bd, sd = _make(device, DynamicLossScale(init_scale=1024, growth_interval=1000), True)
    assert gs.loss_scaler is None and gd.loss_scaler is not None
    ls, ld = [], []
    for _ in range(5):                       # steps 1-2 eager, 3 recorded, 4-5 replayed
        ls.append(ss(*bs).item())
        ld.append(sd(*bd).item())
    assert ss.plan is not None and sd.plan is not None
    assert ls == ld
    a, b = _snapshot(gs, ss), _snapshot(gd, sd)
    for k in a:
        assert _bits_equal(a[k], b[k]), k
    assert _bits_equal(gs.store.flat_aux, gd.store.flat_aux)
    assert gd.loss_scaler.skipped_steps() == 0 and gd.loss_scaler.good_steps() == 5 and gd.loss_scaler.scale() == 1024.0


def _overflow_run(device, replay):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    # (max_scale: the default 2^24 would reject an initial 2^30; nothing grows within these 8 steps)
    g, batch, step = _make(device, DynamicLossScale(init_scale=2.0 ** 30, backoff_factor=2.0 ** -4, max_scale=2.0 ** 30), replay)
    step.build(*batch)                        # variables, optimiser and EMA exist before the first update
    first = _snapshot(g, step)
    scaler = g.loss_scaler
    skipped, applied_at = 0, None
    for k in range(8):
        step(*batch)
        now = scaler.skipped_steps()
        if k == 0:
            # an f16 activation gradient seeded with 2^30 overflows: the run must START with a skip, or this test shows nothing
            assert now >= 1, "the first step was not skipped: 2^30 did not overflow"
        if now == k + 1:                      # every step so far was skipped
            skipped = now
            assert scaler.scale() == 2.0 ** (30 - 4 * now)              # down by exactly 2^-4 per skip
            for name, t in _snapshot(g, step).items():
                assert _bits_equal(t, first[name]), (k, name)             # and nothing was touched
        elif applied_at is None:
            applied_at = k
            assert not torch.equal(g.store.flat, first["w"])
    assert skipped >= 1 and applied_at is not None, (skipped, applied_at)
    last = _snapshot(g, step)
    for name, t in last.items():
        assert bool(torch.isfinite(t).all()), name
    return last, (scaler.scale(), scaler.skipped_steps(), scaler.good_steps()), step


def test_overflow_skips_steps_backs_off_and_recovers_the_same_eager_and_replayed(device):
    from tensorflow_ocr_amd import _lib
    if _lib.STORAGE == "bf16":
        pytest.skip("bfloat16 storage has the range of float32: a 2^30 seed does not overflow, the scale never has to back off")
    ra, sa, step_r = _overflow_run(device, True)
    rb, sb, step_e = _overflow_run(device, False)
    assert step_r.plan is not None and step_e.plan is None
    assert sa == sb, (sa, sb)
    for name in ra:
        assert _bits_equal(ra[name], rb[name]), name
