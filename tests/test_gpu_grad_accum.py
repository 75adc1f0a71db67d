"""GPU: gradient accumulation decided on the device (train.GradAccum; ocr_grad_accum_state in include/ocr_hip.h).

The three rules bit for bit against torch at every alignment with guard words around both buffers, the walk of the state
block, inf / NaN propagation and the argument checks; then whole training steps: a window over one batch K times IS the
plain step, a window over K batches equals the optimiser applied to the sequential sum of separately computed gradients,
eager and replayed, with the dynamic loss scale, clipping, the one-rank exchange and reset_window()."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 16
SENT = -7.25e30
BAR = 2.5e-7              # tests/test_gpu_grad_clip.py: the f32 store plus the f32 product rounding under the root, doubled


# ------------------------------------------------------------------------------------------------ helpers
def _grid_cap():
    # the accumulate kernel runs on the clip kernel's capped grid (csrc/optim.hip: clip_grid); its workspace query tells the cap
    from tensorflow_ocr_amd import ops
    return ops.grad_clip_workspace(1 << 40) // 8


def _sizes():
    # the last makes more than one grid-stride sweep of the capped grid AND has an n & 3 tail
    return [1, 3, 4, 5, 63, 64, 65, 1023, 4099, 4 * 256 * _grid_cap() + 5]


SIZE_IDS = list(range(10))


def _same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def _state(device, k, micro=0):
    from tensorflow_ocr_amd import ops
    st = torch.full((GUARD + 8 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    ops.grad_accum_init(st[GUARD:GUARD + 8], k)
    for _ in range(micro):
        ops.grad_accum_advance(st[GUARD:GUARD + 8])
    return st


def _words(st):
    w = st.cpu().numpy()
    assert (w[:GUARD] == 0x5A5A5A5A).all() and (w[GUARD + 8:] == 0x5A5A5A5A).all()
    return [int(x) for x in w[GUARD:GUARD + 8]]


def _guarded(device, n, off, rng):
    """A buffer of n random f32 values `off` words past a 16-byte boundary, sentinel guard words on both sides."""
    full = torch.full((GUARD + n + GUARD + 4,), SENT, dtype=torch.float32, device=device)
    lo = GUARD + off
    vals = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    full[lo:lo + n] = torch.from_numpy(vals).to(device)
    view = full[lo:lo + n]
    assert view.data_ptr() % 16 == 4 * off
    return full, view


# ------------------------------------------------------------------------------------- 1. the three rules
@pytest.mark.parametrize("k", SIZE_IDS)
def test_three_rules_bit_for_bit_against_torch_at_every_alignment(device, k):
    from tensorflow_ocr_amd import ops
    n = _sizes()[k]
    rng = np.random.default_rng(40 + k)
    states = [_state(device, 3, m) for m in range(3)]
    for off in range(4):
        for micro in range(3):
            gfull, g = _guarded(device, n, off, rng)
            afull, a = _guarded(device, n, off, rng)
            g0, a0 = gfull.clone(), afull.clone()
            lo = GUARD + off
            ops.grad_accum(g, a, states[micro][GUARD:GUARD + 8])
            want_g, want_a = g0.clone(), a0.clone()
            if micro == 0:
                want_a[lo:lo + n] = g0[lo:lo + n]
            elif micro == 1:
                want_a[lo:lo + n] = a0[lo:lo + n] + g0[lo:lo + n]
            else:
                want_g[lo:lo + n] = a0[lo:lo + n] + g0[lo:lo + n]
            # slice, guard words and the buffer the rule does not write: all of both allocations, bit for bit
            assert _same_bits(gfull, want_g), (n, off, micro, "grad")
            assert _same_bits(afull, want_a), (n, off, micro, "acc")
    for m, st in enumerate(states):
        assert _words(st) == [m, 3, 0, 0, 0, 0, 0, 0]              # the accumulate kernel writes nothing to the state


# ------------------------------------------------------------------------------------- 2. state walk
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_state_walk_and_window_sums(device, K):
    from tensorflow_ocr_amd import ops
    n = 1031
    rng = np.random.default_rng(K)
    st = _state(device, K)
    s = st[GUARD:GUARD + 8]
    assert _words(st) == [0, K, 0, 0, 0, 0, 0, 0]
    buf = torch.empty(n + 1, dtype=torch.float32, device=device)
    abuf = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=device)    # never zeroed: the first rule stores
    g, a = buf[1:], abuf[1:]
    for window in range(2):
        gs = [torch.from_numpy(rng.standard_normal(n).astype(F32)).to(device) for _ in range(K)]
        total = gs[0].clone()
        for m in range(K):
            g.copy_(gs[m])
            ops.grad_accum(g, a, s)
            assert _words(st) == [m, K, window, 0, 0, 0, 0, 0]
            if m > 0:
                total = total + gs[m]                              # ((g1 + g2) + g3) + ...
            if m == K - 1:
                assert _same_bits(g, total) and bool(torch.isfinite(g).all())
            else:
                assert _same_bits(g, gs[m]) and _same_bits(a, total)
            ops.grad_accum_advance(s)
            assert _words(st) == [(m + 1) % K, K, window + (m == K - 1), 0, 0, 0, 0, 0]
    if K == 1:
        assert bool(torch.isnan(abuf).all())                       # K = 1 neither reads nor writes acc; grad was left as it was
    ops.grad_accum_init(s, K)
    assert _words(st) == [0, K, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------- 3. propagation, arguments
def test_inf_and_nan_in_any_micro_gradient_reach_the_closing_sum(device):
    from tensorflow_ocr_amd import ops
    K, n = 3, 1033
    st = _state(device, K)
    s = st[GUARD:GUARD + 8]
    g = torch.empty(n + 1, dtype=torch.float32, device=device)[1:]       # three head elements, a body, a two-element tail
    a = torch.zeros(n + 1, dtype=torch.float32, device=device)[1:]
    assert g.data_ptr() % 16 == 4 and a.data_ptr() % 16 == 4 and (n - 3) % 4 == 2
    for m_bad in range(K):
        for bad in (float("inf"), float("-inf"), float("nan")):
            for pos in (0, 2, n // 2, n - 1):
                for m in range(K):
                    g.fill_(1.0)
                    if m == m_bad:
                        g[pos] = bad
                    ops.grad_accum(g, a, s)
                    ops.grad_accum_advance(s)
                out = g.cpu().numpy()
                assert not np.isfinite(out[pos]), (m_bad, bad, pos)
                ok = np.delete(out, pos)
                assert (ok == K).all(), (m_bad, bad, pos)
    assert _words(st)[:3] == [0, K, 3 * 3 * 4]


def test_bad_arguments_are_refused_and_nothing_is_written(device):
    from tensorflow_ocr_amd import _lib, ops
    st = _state(device, 2, 1)                                            # micro 1 of 2: an accepted call would write grad
    s = st[GUARD:GUARD + 8]
    rng = np.random.default_rng(9)
    gfull, g = _guarded(device, 64, 0, rng)
    afull, a = _guarded(device, 64, 0, rng)
    g0, a0 = gfull.clone(), afull.clone()
    stream = _lib.stream_ptr()
    null = ctypes.c_void_p(0)
    for k in (0, -1):
        with pytest.raises(_lib.OcrHipError):
            ops.grad_accum_init(s, k)
    with pytest.raises(_lib.OcrHipError):
        _lib.call("ocr_grad_accum_init", null, ctypes.c_int(2), stream)
    with pytest.raises(_lib.OcrHipError):
        _lib.call("ocr_grad_accum_advance", null, stream)
    P = _lib.ptr
    shifted = lambda t, words: ctypes.c_void_p(t.data_ptr() + 4 * words)
    cases = [(null, P(a), 64, P(s)), (P(g), null, 64, P(s)), (P(g), P(a), 64, null), (P(g), P(a), -1, P(s)), (P(g), P(a), 0, P(s)),
             (shifted(g, 1), P(a), 32, P(s)), (P(g), shifted(a, 2), 32, P(s)), (shifted(g, 3), shifted(a, 1), 32, P(s)),
             (ctypes.c_void_p(g.data_ptr() + 2), ctypes.c_void_p(a.data_ptr() + 2), 32, P(s))]
    for gp, ap, n, sp in cases:
        with pytest.raises(_lib.OcrHipError):
            _lib.call("ocr_grad_accum_f32", gp, ap, ctypes.c_int64(n), sp, stream)
    assert _same_bits(gfull, g0) and _same_bits(afull, a0) and _words(st) == [1, 2, 0, 0, 0, 0, 0, 0]
    # equal offsets are accepted, whatever they are
    _lib.call("ocr_grad_accum_f32", shifted(g, 3), shifted(a, 3), ctypes.c_int64(32), P(s), stream)
    assert _same_bits(gfull[GUARD + 3:GUARD + 35], a0[GUARD + 3:GUARD + 35] + g0[GUARD + 3:GUARD + 35])


# ------------------------------------------------------------------------------------- whole steps
# nets/model_vgg_16.model_vgg at full width on 64x64 images, batch 2: the net and shapes of tests/test_gpu_grad_clip.py::_make
def _loss_scale(mode):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    return 1024.0 if mode == "numeric" else DynamicLossScale(init_scale=1024, growth_interval=1000)


def _fl(gr, im, px, lk, mk):
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    a, b = M.model_vgg(im, graph=gr)
    return M.loss(px, a, lk, b, mk, graph=gr)


_BATCHES = {}


def _batch(device, i):
    """Batch number i (i = 0: the batch of the other whole-step test files); made once, never written: every call hands
    out copies, because a recording step keeps its batch tensors as the plan's input buffers and replays write them."""
    from tensorflow_ocr_amd import synthetic
    key = (str(device), i)
    if key not in _BATCHES:
        _BATCHES[key] = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(5 + i), 2, 64)]
    return [t.clone() for t in _BATCHES[key]]


def _make(device, mode, replay, K=None, clip_norm=None, which="adam", **step_kw):
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer, TrainStep
    g = Graph(device, loss_scale=_loss_scale(mode), seed=3)
    kw = {} if clip_norm is None else {"clip_norm": clip_norm}
    if which == "adam":
        factory = lambda gr: AdamOptimizer(gr, learning_rate=1e-3, **kw)
    else:
        factory = lambda gr: MomentumOptimizer(gr, base_lr=0.01, moving_average_decay=0.99, **kw)
    if K is not None:
        step_kw["accumulate_steps"] = K
    return g, TrainStep(g, _fl, factory, replay=replay, **step_kw)


def _snapshot(g, step):
    o = step.opt
    snap = {"w": g.store.flat.clone(), "ema": o.ema.clone()}
    if hasattr(o, "m"):
        snap.update(m=o.m.clone(), v=o.v.clone())
    else:
        snap.update(acc=o.acc.clone())
    return snap


def _assert_same(a, b, what):
    for name in a:
        assert _same_bits(a[name], b[name]), (what, name)


class _Reference:
    """The window built from existing pieces on a graph of its own: forward and backward per micro-batch without an
    optimiser, the gradients cloned and added one after the other with torch, the sum written into flat_grad and
    `apply_gradients(1 / K)`."""

    def __init__(self, device, mode, which="adam", clip_norm=None):
        self.g, self.step = _make(device, mode, False, None, clip_norm, which)
        self.step.build(*_batch(device, 0))

    def grad(self, batch):
        g = self.g
        g.reset_tape()
        _fl(g, *batch)
        g.backward(None)
        g.reset_tape()
        return g.store.flat_grad.clone()

    def apply(self, grads, poison=None):
        """poison = (micro-step, index, value): written into that micro-gradient's clone."""
        total = None
        for m, gr in enumerate(grads):
            if poison is not None and poison[0] == m:
                gr[poison[1]] = poison[2]
            total = gr if total is None else total + gr
        self.g.store.flat_grad.copy_(total)
        self.step.opt.apply_gradients(1.0 / len(grads))
        self.step._repack()
        return total

    def window(self, batches, poison=None):
        return self.apply([self.grad(b) for b in batches], poison)


def _recorded(step, batch):
    """tests/test_gpu_grad_clip.py::_recorded: the C-ABI calls the host callbacks of a REPLAYED step made."""
    from tensorflow_ocr_amd import _lib
    if step.plan is None:
        return step(*batch), None
    rec = _lib.Recorder()
    _lib.RECORDER = rec
    try:
        loss = step(*batch)
    finally:
        _lib.RECORDER = None
    return loss, [e[3] for e in rec.entries if e[0] == "c"]


NEW = ("ocr_grad_accum_init", "ocr_grad_accum_f32", "ocr_grad_accum_advance")


def _windows(replay, K):
    """Enough windows that replayed calls close at least one: the recording is the first closing call >= 3."""
    if not replay:
        return 2
    rec_call = K * -(-3 // K)                 # the first multiple of K that is >= 3
    return rec_call // K + 1


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("K", [2, 4])
def test_window_over_the_same_batch_is_the_plain_step_bit_for_bit(device, K, replay):
    b = _batch(device, 0)
    g0, s0 = _make(device, "numeric", replay)
    g1, s1 = _make(device, "numeric", replay, K)
    s0.build(*b)
    s1.build(*b)
    aux0 = g0.store.flat_aux.clone()
    assert s1.accum is not None and s1.accum.acc.shape == g1.store.flat_grad.shape and s0.accum is None
    for w in range(_windows(replay, K) + (1 if replay else 0)):
        s0(*b)
        for m in range(K):
            assert s1.micro_step == m
            s1(*b)
            assert s1.closes_window == (m == K - 1)
        # sum of K equal gradients = K g exactly (K a power of two), times grad_scale / K: the plain step's product
        _assert_same(_snapshot(g0, s0), _snapshot(g1, s1), "window %d" % w)
        assert s1.opt.global_step == s0.opt.global_step == w + 1 and s1.steps == K * (w + 1)
    assert (s1.plan is not None) == replay and s1.accum.windows() == s1.opt.global_step
    # the BN moving statistics advanced on every micro-step: K forward passes per window against one
    assert not torch.equal(g0.store.flat_aux, aux0) and not torch.equal(g1.store.flat_aux, g0.store.flat_aux)


@pytest.mark.parametrize("replay", [False, True])
def test_window_over_three_batches_equals_the_optimiser_on_the_sequential_sum(device, replay):
    K = 3
    g, s = _make(device, "numeric", replay, K)
    s.build(*_batch(device, 0))
    ref = _Reference(device, "numeric")
    _assert_same(_snapshot(ref.g, ref.step), _snapshot(g, s), "built")
    for w in range(_windows(replay, K)):
        bs = [_batch(device, K * w + m) for m in range(K)]
        total = ref.window(bs)
        for m in range(K):
            before = _snapshot(g, s)
            counters = (s.opt.global_step, g.store.version)
            s(*bs[m])
            if m < K - 1:
                # a micro-step inside its window changes nothing but the gradients and the moving statistics
                _assert_same(before, _snapshot(g, s), "window %d micro %d" % (w, m))
                assert counters == (s.opt.global_step, g.store.version) and not s.closes_window
        assert s.closes_window and _same_bits(g.store.flat_grad, total)
        _assert_same(_snapshot(ref.g, ref.step), _snapshot(g, s), "window %d" % w)
        assert _same_bits(ref.g.store.flat_aux, g.store.flat_aux), w
    assert (s.plan is not None) == replay


@pytest.mark.parametrize("which", ["adam", "momentum"])
def test_replay_equals_eager_over_three_windows(device, which):
    K = 2
    ge, se = _make(device, "numeric", False, K, which=which)
    gr, sr = _make(device, "numeric", True, K, which=which)
    for w in range(3):
        for m in range(K):
            b = _batch(device, K * w + m)
            le, lr = se(*b), sr(*b)
            assert le.item() == lr.item()
        _assert_same(_snapshot(ge, se), _snapshot(gr, sr), "window %d" % w)
        assert _same_bits(ge.store.flat_aux, gr.store.flat_aux)
    assert sr.plan is not None and se.plan is None and sr.steps == 6       # calls 5 and 6 were replayed


@pytest.mark.parametrize("mode", ["numeric", "dynamic"])
def test_replayed_micro_steps_inside_a_window_launch_no_optimiser(device, mode):
    K = 3
    g, s = _make(device, mode, True, K, clip_norm=1e30 if mode == "dynamic" else None)
    for i in range(6):                                # calls 1-5 eager, call 6 closes a window and is recorded
        s(*_batch(device, i))
    assert s.plan is not None
    tags = [e[4][0] for e in s.recorded if e[0] == "c" and e[4] is not None]
    names = [e[3] for e in s.recorded if e[0] == "c"]
    assert names.count("ocr_grad_accum_f32") == 1 and names.count("ocr_grad_accum_advance") == 1 and tags.count("accum") == 2
    assert [e[2] for e in s.plan if e[0] == "py" and len(e) > 2] == ["opt", "repack"]
    launched = []
    for m in range(K):
        before, counters = _snapshot(g, s), (s.opt.global_step, g.store.version)
        _, host = _recorded(s, _batch(device, 6 + m))
        launched.append(host)
        if m < K - 1:
            assert host == [], host                   # no optimiser, no check or clip pass, no re-pack
            _assert_same(before, _snapshot(g, s), m)
            assert counters == (s.opt.global_step, g.store.version)
    first = ["ocr_adam_step"] if mode == "numeric" else ["ocr_grad_check_clip_f32", "ocr_adam_step_clip"]
    assert launched[2][:len(first)] == first, launched[2]
    assert not [x for x in launched[2] if x in NEW]   # the accumulate entries are the plan's own, not a host callback's


def test_default_step_launches_none_of_the_new_entry_points(device):
    g, s = _make(device, "numeric", True)
    b = _batch(device, 0)
    for _ in range(3):
        s(*b)
    assert s.plan is not None and s.accum is None and s.accumulate_steps == 1
    assert not [e[3] for e in s.recorded if e[0] == "c" and e[3] in NEW]
    assert not [e for e in s.recorded if e[0] == "c" and e[4] is not None and e[4][0] == "accum"]
    _, host = _recorded(s, b)
    assert host[0] == "ocr_adam_step" and not [x for x in host if x in NEW]
    assert s.closes_window and s.micro_step == 0 and s.steps == 4
    s.reset_window()                                  # nothing to reset: no launch, no error
    # (and with accumulation the recorded step does hold them: the check above can fail)
    g2, s2 = _make(device, "numeric", True, 2)
    for _ in range(4):
        s2(*b)
    assert s2.plan is not None and {"ocr_grad_accum_f32", "ocr_grad_accum_advance"} <= {e[3] for e in s2.recorded if e[0] == "c"}


@pytest.mark.parametrize("replay", [False, True])
def test_overflow_in_one_micro_gradient_skips_the_window(device, replay):
    K, bad_window, j = 3, 2, 12345
    g, s = _make(device, "dynamic", replay, K)
    s.build(*_batch(device, 0))
    ref = _Reference(device, "dynamic")
    scaler = g.loss_scaler
    for w in range(4):                                # replayed: calls 1-5 eager, 6 recorded, windows 2 and 3 replayed
        bs = [_batch(device, K * w + m) for m in range(K)]
        ref.window(bs, poison=(1, j, float("inf")) if w == bad_window else None)
        before = _snapshot(g, s)
        scale0 = scaler.scale()
        for m in range(K):
            s(*bs[m])
            if m == 1 and w == bad_window:
                # the second micro-gradient's element j is inf: the running sum g1 + g2 holds it
                s.accum.acc[j] = float("inf")
            if m < K - 1:
                assert scaler.scale() == scale0       # the scale moves in the check pass only: once per window
        if w == bad_window:
            _assert_same(before, _snapshot(g, s), "skipped window")            # nothing was written
            assert scaler.skipped_steps() == 1 and scaler.scale() == scale0 / 2   # backed off once
            assert not bool(torch.isfinite(g.store.flat_grad[j]))
        else:
            assert scaler.scale() == scale0 and not _same_bits(before["w"], g.store.flat)
        # every window, the one behind the skip included: the reference run skipped the same step
        _assert_same(_snapshot(ref.g, ref.step), _snapshot(g, s), "window %d" % w)
        assert _same_bits(ref.g.store.flat_aux, g.store.flat_aux)
    assert ref.g.loss_scaler.skipped_steps() == 1 and ref.g.loss_scaler.scale() == scaler.scale() == 512.0
    assert (s.plan is not None) == replay and s.opt.global_step == 4


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("mode", ["numeric", "dynamic"])
def test_clip_norm_is_the_norm_of_the_mean_gradient(device, mode, replay):
    K = 2
    g, s = _make(device, mode, replay, K, clip_norm=1e30)
    s.build(*_batch(device, 0))
    ref = _Reference(device, mode)
    for w in range(_windows(replay, K)):
        bs = [_batch(device, K * w + m) for m in range(K)]
        total = ref.window(bs)
        for b in bs:
            s(*b)
        base = F32((1.0 / K) / 1024.0)                # grad_scale / K over the loss scale: what the optimiser multiplies with
        want = float(torch.sqrt(torch.sum((total.double() * float(base)) ** 2)).item())
        got = s.opt.grad_norm()
        print("window %d: norm %.9g ref %.9g" % (w, got, want))
        assert abs(got - want) <= BAR * want, (w, got, want)
        _assert_same(_snapshot(ref.g, ref.step), _snapshot(g, s), "window %d" % w)     # a clip that never bites
    assert s.opt.clipped_steps() == 0 and s.opt.nonfinite_steps() == 0 and (s.plan is not None) == replay


@pytest.mark.parametrize("replay", [False, True])
def test_reset_window_restarts_the_window(device, replay):
    K = 3
    g, s = _make(device, "numeric", replay, K)
    s.build(*_batch(device, 0))
    ref = _Reference(device, "numeric")
    n = 0
    for w in range(_windows(replay, K)):
        # two calls of a window that is then abandoned
        for m in range(2):
            s(*_batch(device, 20 + m))
        assert s.micro_step == 2 and not s.closes_window
        s.reset_window()
        assert s.micro_step == 0 and s.accum.micro == 0
        assert s.accum.state.cpu().tolist()[:3] == [0, K, 0]
        bs = [_batch(device, K * w + m) for m in range(K)]
        # the reference's moving statistics see the same five forward passes; its window is the last three gradients
        total = ref.apply([ref.grad(b) for b in [_batch(device, 20), _batch(device, 21)] + bs][2:])
        for b in bs:
            s(*b)
        n += 1
        assert s.closes_window and s.opt.global_step == n and _same_bits(g.store.flat_grad, total)
        _assert_same(_snapshot(ref.g, ref.step), _snapshot(g, s), "window %d" % w)
        assert _same_bits(ref.g.store.flat_aux, g.store.flat_aux)
    assert (s.plan is not None) == replay


# ------------------------------------------------------------------------------------- one-rank exchange
_RCCL1_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as td
from tensorflow_ocr_amd import _lib, dist, synthetic
from tensorflow_ocr_amd.graph import Graph
from tensorflow_ocr_amd.nets import model_vgg_16 as M
from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
rank, world, local = dist.init_process_group_from_env("nccl", force=True)      # ONE-rank RCCL communicator
assert (rank, world) == (0, 1) and td.get_backend() == "nccl"
dev = torch.device("cuda:0")
K = 2
batches = [[torch.from_numpy(a).to(dev) for a in synthetic.make_batch(np.random.default_rng(50 + i), 2, 64)] for i in range(8)]
def fl(gr, im, px, lk, mk):
    a, b = M.model_vgg(im, graph=gr)
    return M.loss(px, a, lk, b, mk, graph=gr)
def make(force):
    g = Graph(dev, loss_scale=1024.0, seed=3)
    return g, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3), world_size=world, bucket_bytes=8 << 20,
                        force_reduce=force, accumulate_steps=K)
reached = []                                         # the comm entry point, however it is reached
real_call, real_ar = _lib.call, td.all_reduce
def call(name, *args):
    if name == "ocr_allreduce_bucket":
        reached.append(name)
    return real_call(name, *args)
def all_reduce(*args, **kw):
    reached.append("td.all_reduce")
    return real_ar(*args, **kw)
_lib.call, td.all_reduce = call, all_reduce
def counting(fn):
    def f(*args):
        reached.append("ocr_allreduce_bucket")
        return fn(*args)
    return f
for mode in ("abi", "torch"):
    os.environ["OCR_EXCHANGE"] = mode
    g0, s0 = make(False)
    g1, s1 = make(True)
    wrapped = False
    for w in range(4):                               # calls 1-3 eager, 4 recorded, windows 2 and 3 replayed
        for m in range(K):
            b = batches[K * w + m]
            s0(*b)
            if s1.plan is not None and not wrapped:
                for e in s1.plan:                    # a replayed step issues the plan's entries directly
                    if e[0] == "c" and e[3] == "ocr_allreduce_bucket":
                        e[1] = counting(e[1])
                wrapped = True
            before = len(reached)
            s1(*b)
            red = s1.reducer
            if m < K - 1:
                assert len(reached) == before, (mode, w, m, reached[before:])      # no exchange inside a window
            else:
                assert len(reached) - before == len(red.buckets), (mode, w, len(reached) - before)      # once per window
        torch.cuda.synchronize()
        assert torch.equal(g0.store.flat, g1.store.flat), (mode, w, (g0.store.flat - g1.store.flat).abs().max().item())
        assert torch.equal(s0.opt.m, s1.opt.m) and torch.equal(s0.opt.v, s1.opt.v) and torch.equal(s0.opt.ema, s1.opt.ema)
    assert s1.plan is not None and red.active and red.mode == mode and len(red.buckets) >= 2 and not s0.reducer.active
    acc = [e for e in s1.recorded if e[0] == "c" and e[3] == "ocr_grad_accum_f32"]
    if mode == "abi":
        # one accumulate entry per bucket, tagged to replay in every phase, each in front of its bucket's all-reduce
        assert len(acc) == len(red.buckets) and all(e[4] == ("accum",) for e in acc)
        pos = {id(e): i for i, e in enumerate(s1.plan)}
        ars = [e for e in s1.plan if e[0] == "c" and e[3] == "ocr_allreduce_bucket"]
        assert len(ars) == len(acc)
        firsts = sorted(pos[id(e)] for e in acc)
        for i, e in enumerate(sorted(ars, key=lambda e: pos[id(e)])):
            assert firsts[i] < pos[id(e)]
    else:
        assert not acc                               # the bucket hooks are host callbacks and run it themselves
    print("mode", mode, "ok")
td.barrier(); td.destroy_process_group()
print("rccl-1 accum ok")
"""


def test_one_rank_exchange_runs_once_per_window(device, tmp_path):
    """The bucketed exchange (one-rank RCCL group, as tests/test_gpu_train_step.py sets it up) with K = 2: parameters
    bit-identical to the run without it, the comm entry point reached once per bucket and WINDOW, in both exchange modes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl1_accum.py"
    script.write_text(_RCCL1_WORKER % root)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "OCR_EXCHANGE")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=540)
    out = r.stdout.decode()
    assert r.returncode == 0 and "rccl-1 accum ok" in out and "mode abi ok" in out and "mode torch ok" in out, out[-3000:]
