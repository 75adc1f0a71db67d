"""Training-step assembly: mirror of multigpu_train.py:27-36,70-85,103-142 (tower loss ->
mean of tower gradients -> Adam with staircase exponential decay -> EMA) and of
train_pixellink.py:179-194,222-243 (sum of pre-divided gradients -> Momentum).

One process drives one GPU ("tower"); the cross-tower gradient mean of `average_gradients`
(multigpu_train.py:70-85) is an RCCL all-reduce over the flat gradient buffer, issued by
`dist.GradientAllReduce` on a side stream.

The recorded step's plan — its tags, `schedule_guests`, the replay walk — is `step_plan`; the names below are imported
so that `train.schedule_guests` and the switches `train.GUEST_*` stay what callers read and set: TrainStep passes
THIS module's switch values to the scheduler.
"""
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import ops, step_plan
from .graph import F32
from .step_plan import (GUEST_BALANCE, GUEST_COVER, GUEST_MIN_US, GUEST_PAIRED_GRID, USE_GUESTS, XCHG_AT_FORK,  # noqa: F401
                        _VIEW_OPS, _record_audit, schedule_guests)

def exponential_decay(learning_rate, global_step, decay_steps=5000, decay_rate=0.94, staircase=True):
    """tf.train.exponential_decay (multigpu_train.py:104)."""
    e = global_step // decay_steps if staircase else global_step / decay_steps
    return learning_rate * decay_rate ** e


def pixellink_lr(global_step, base_lr=0.01):
    """train_pixellink.py:222-237: base_lr * {0.1 if step<20k, 0.01 if <40k, 0.001 if <60k, else 1}."""
    if global_step < 20000:
        f = 0.1
    elif global_step < 40000:
        f = 0.01
    elif global_step < 60000:
        f = 0.001
    else:
        f = 1.0
    return base_lr * f


class GradClip:
    """Global-norm gradient clipping decided on the device (ocr_grad_clip_state, include/ocr_hip.h): the optimisers'
    `clip_norm=c`.  Per step one pass over the reduced flat gradient buffer leaves norm = |g * base|, coef =
    min(1, c / norm) and g_mul = base * coef in an 8-word device block — fused into the dynamic loss scale's check pass
    where one runs, a pass of its own with a numeric loss scale — and the `_clip` optimiser kernel multiplies g with
    g_mul, or writes nothing when the norm is not finite.  `base` is the factor the optimiser applies anyway (grad_scale /
    loss_scale), so the clipped quantity is the un-scaled gradient of the DATA loss; the L2 term weight_decay * w is
    added inside the optimiser kernel and is not part of the norm.  No host read on the path.

    The state block and the f64 partials are allocated here, once: a recorded plan replays their addresses.  Nothing of
    this is checkpointed: `clip_norm` is a flag, the counters are diagnostics."""

    def __init__(self, clip_norm, flat_grad):
        self.clip_norm = check_clip_norm(clip_norm)
        self.state = torch.zeros(ops.GRAD_CLIP_WORDS, dtype=torch.int32, device=flat_grad.device)     # = ocr_grad_clip_init
        self.ws = torch.empty(max(1, ops.grad_clip_workspace(flat_grad.numel()) // 8), dtype=torch.float64,
                              device=flat_grad.device)

    def _words(self):
        return self.state.cpu().numpy()

    def grad_norm(self):
        return float(self._words()[ops.GC_NORM:ops.GC_NORM + 1].view(np.float32)[0])

    def clipped_steps(self):
        return int(self._words()[ops.GC_CLIPPED_TOTAL])

    def nonfinite_steps(self):
        return int(self._words()[ops.GC_NONFINITE_TOTAL])


def check_clip_norm(clip_norm):
    """A finite number > 0 as a float, ValueError otherwise."""
    v = clip_norm
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v <= 0:
        raise ValueError("clip_norm must be a positive finite number (or None: no clipping), got %r" % (clip_norm,))
    if float(v) > float(np.finfo(np.float32).max) or float(v) < float(np.finfo(np.float32).tiny):
        raise ValueError("clip_norm %r is outside float32's range" % (clip_norm,))
    return float(v)


def check_accumulate_steps(k):
    """An int >= 1, ValueError otherwise."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("accumulate_steps must be an integer >= 1, got %r" % (k,))
    return int(k)


class StaticFactor:
    """The gradient factor policy of a constant loss scale.  A policy says which factor multiplies the gradients in the
    optimiser step and where it lives: the pass over the flat gradient buffer in front of the step (`pre_step`), the
    suffix of the step entry and that entry's trailing arguments (`suffix`, `step_args`), the (mul_host, mul_dev) pair
    of `TrainStep.summary_factor`, and what the drivers log and write of it.  An optimiser picks one, once (`grad_factor`).

    Constant scale: no pass; the step entry takes grad_scale / loss_scale."""
    suffix = ""

    def __init__(self, graph):
        self.g = graph

    def pre_step(self, grad, grad_scale):
        pass

    def clip_pass(self, clip, grad, grad_scale):
        """The pass of a `ClippedFactor` around this policy: one launch more than without clipping."""
        ops.grad_clip(grad, clip.state, clip.clip_norm, grad_scale / self.g.loss_scale, clip.ws)

    def step_args(self, grad_scale, ema_decay):
        return grad_scale / self.g.loss_scale, ema_decay

    def summary_factor(self, grad_scale):
        return grad_scale / self.g.loss_scale, None

    def log_lines(self):
        """What a driver prints behind its loss line (READS THE DEVICE, like `scalars`: for logging only)."""
        return []

    def scalars(self):
        return {}


class DynamicFactor(StaticFactor):
    """Dynamic loss scaling (graph.DynamicLossScale): the check sees the REDUCED gradients (inf / NaN survive a sum
    all-reduce, so every rank decides alike), the guarded `_dyn` step reads 1 / scale from the scaler's block and writes
    nothing when the check found one.  The optimiser's host counters advance either way: no device read in the step."""
    suffix = "_dyn"

    def __init__(self, graph):
        self.scaler = graph.loss_scaler

    def pre_step(self, grad, grad_scale):
        self.scaler.check(grad)

    def clip_pass(self, clip, grad, grad_scale):
        """The check pass also sums the norm: two launches, as without clipping."""
        sc = self.scaler
        ops.grad_check_clip(grad, sc.state, sc.growth_factor, sc.backoff_factor, sc.growth_interval, sc.min_scale,
                            sc.max_scale, clip.state, clip.clip_norm, grad_scale, clip.ws)

    def step_args(self, grad_scale, ema_decay):
        return grad_scale, ema_decay, self.scaler.state

    def summary_factor(self, grad_scale):
        return grad_scale, self.scaler.state[ops.LS_INV_SCALE_USED:ops.LS_INV_SCALE_USED + 1].view(torch.float32)

    def log_lines(self):
        return ['loss scale {:g}, {:d} steps skipped'.format(self.scaler.scale(), self.scaler.skipped_steps())]

    def scalars(self):
        return {'loss_scale': self.scaler.scale()}


class ClippedFactor:
    """Global-norm clipping (`GradClip`) around either policy above: the inner policy's clip pass leaves g_mul and skip in
    the clip block, and the `_clip` step takes no factor but that block."""
    suffix = "_clip"

    def __init__(self, inner, clip):
        self.inner, self.clip = inner, clip

    def pre_step(self, grad, grad_scale):
        self.inner.clip_pass(self.clip, grad, grad_scale)

    def step_args(self, grad_scale, ema_decay):
        return ema_decay, self.clip.state

    def summary_factor(self, grad_scale):
        return 1.0, self.clip.state[ops.GC_G_MUL:ops.GC_G_MUL + 1].view(torch.float32)

    def log_lines(self):
        return self.inner.log_lines() + ['grad norm {:.4g}, {:d} steps clipped'.format(self.clip.grad_norm(),
                                                                                     self.clip.clipped_steps())]

    def scalars(self):
        return dict(self.inner.scalars(), grad_norm=self.clip.grad_norm())


def grad_factor(graph, clip):
    """The policy of (graph.loss_scaler, clip): the one place that tells the cases apart."""
    inner = DynamicFactor(graph) if graph.loss_scaler is not None else StaticFactor(graph)
    return ClippedFactor(inner, clip) if clip is not None else inner


class GradAccum:
    """Gradient accumulation decided on the device (ocr_grad_accum_state, include/ocr_hip.h): `TrainStep(accumulate_steps=K)`.
    `acc` mirrors the flat gradient buffer; `run(s, e)` applies to the slice [s, e) of both the rule of the running
    micro-step — store on the first, add in between, and on the closing one grad = acc + grad, so that the window's sum
    ((g1 + g2) + ...) + gK stands where the exchange and the optimiser read it — and `advance()` moves the phase, once per
    step behind every `run` of it.  The kernel reads the phase from the 8-word device block: a recorded plan holds one
    entry that is right in every phase.  `micro` is the host's mirror of it (no device read in a step); with the buffers
    on the CPU (the gloo path) the same three rules run as torch operators on the mirror.

    The buffer and the block are allocated here, once: a recorded plan replays their addresses.  Nothing of this is
    checkpointed: a restored run starts a fresh window (`TrainStep.reset_window`)."""

    def __init__(self, k, flat_grad):
        self.k = check_accumulate_steps(k)
        self.grad = flat_grad
        self.acc = torch.zeros_like(flat_grad)
        self.state = torch.zeros(ops.GRAD_ACCUM_WORDS, dtype=torch.int32, device=flat_grad.device)
        self.micro = 0
        self.reset()

    @property
    def closing(self):
        return self.micro == self.k - 1

    def _unrecorded(self, fn, *args):
        from . import _lib
        rec, _lib.RECORDER = _lib.RECORDER, None           # an initialising launch is no part of a replayed plan
        try:
            fn(*args)
        finally:
            _lib.RECORDER = rec

    def reset(self):
        """micro = 0, windows_total = 0 on the device and in the mirror."""
        self.micro = 0
        if self.state.is_cuda:
            self._unrecorded(ops.grad_accum_init, self.state, self.k)
        else:
            self.state.zero_()
            self.state[ops.GA_K] = self.k

    def run(self, s=0, e=None, record=True):
        """The running micro-step's rule on grad[s:e] / acc[s:e]; in a recording the entry is tagged ("accum",).
        record=False: the caller's host callback re-runs this call on every replay (dist: torch mode)."""
        e = self.grad.numel() if e is None else e
        g, a = self.grad[s:e], self.acc[s:e]
        if g.is_cuda:
            if not record:
                return self._unrecorded(ops.grad_accum, g, a, self.state)
            from . import _lib
            ops.grad_accum(g, a, self.state)
            if _lib.RECORDER is not None:
                _lib.RECORDER.tag_last(step_plan.accum_tag())
        elif self.k == 1:
            pass
        elif self.micro >= self.k - 1:
            g.add_(a)                          # (f32 addition commutes: the bits of acc + grad)
        elif self.micro == 0:
            a.copy_(g)
        else:
            a.add_(g)

    def advance(self):
        if self.state.is_cuda:
            from . import _lib
            ops.grad_accum_advance(self.state)
            if _lib.RECORDER is not None:
                _lib.RECORDER.tag_last(step_plan.accum_tag(advance=True))
        else:
            self.state[ops.GA_MICRO] = (self.micro + 1) % self.k
            if self.micro + 1 >= self.k:
                self.state[ops.GA_WINDOWS_TOTAL] += 1
        self.micro = (self.micro + 1) % self.k

    def windows(self):
        """Windows closed since the last reset (READS THE DEVICE: a sync)."""
        return int(self.state.cpu().numpy()[ops.GA_WINDOWS_TOTAL])


class Optimizer:
    """What the two optimisers share: the construction order (clip check, flat buffers, slots, EMA shadows, clip block,
    gradient factor policy), the EMA warm-up, the checkpoint dictionaries and the step's skeleton.  A subclass names its
    step entry (`STEP`), its checkpoint slots and the attribute each lives in (`SLOTS`, `BUFFERS`), and has
    `learning_rate()`, `scalar_state_dict()` and `_launch(entry, st, tail)`: the one step launch, `tail` being the
    policy's trailing arguments."""
    STEP, SLOTS, BUFFERS = None, (), {}

    def __init__(self, graph, moving_average_decay, weight_decay, clip_norm):
        if clip_norm is not None:
            check_clip_norm(clip_norm)               # before anything is allocated
        self.g = graph
        graph.ensure_materialised()
        st = graph.store
        for name in self.SLOTS:
            setattr(self, self.BUFFERS[name], torch.zeros_like(st.flat))
        self.ema = st.flat.clone() if moving_average_decay else None
        self.mad, self.wd = moving_average_decay, weight_decay
        self.clip = GradClip(clip_norm, st.flat_grad) if clip_norm is not None else None
        self.factor = grad_factor(graph, self.clip)
        self.global_step = 0
        self._reg_out = None

    def ema_decay(self):
        """ExponentialMovingAverage(decay, num_updates=global_step): the warm-up min(decay, (1 + n) / (10 + n)); 0 = no shadows."""
        return min(self.mad, (1.0 + self.global_step) / (10.0 + self.global_step)) if self.mad else 0.0

    def apply_gradients(self, grad_scale=1.0):
        st = self.g.store
        self.factor.pre_step(st.flat_grad, grad_scale)
        self._launch(getattr(ops, self.STEP + self.factor.suffix), st, self.factor.step_args(grad_scale, self.ema_decay()))
        st.version += 1
        self.global_step += 1

    def shadow_state_dict(self):
        """EMA shadows by variable name (what test.py:149-150 restores)."""
        return self.g.store.by_variable(self.ema)

    def slot_state_dict(self):
        return {name: self.g.store.by_variable(getattr(self, self.BUFFERS[name])) for name in self.SLOTS}

    def load_state(self, global_step=None, slots=None, ema=None):
        st = self.g.store
        if slots:
            for name in self.SLOTS:
                st.load_by_variable(getattr(self, self.BUFFERS[name]), slots.get(name, {}))
        if ema and self.ema is not None:
            st.load_by_variable(self.ema, ema)
        if global_step is not None:
            self.global_step = int(global_step)

    def regularization_loss(self):
        """Sum of tf.GraphKeys.REGULARIZATION_LOSSES (multigpu_train.py:36): slim.l2_regularizer(wd) on
        every regularised variable = wd/2 * sum(w^2) over the head of the flat buffer.  One device
        reduction; returns a 1-element f32 device tensor (read it with .item() where the loss is logged)."""
        st = self.g.store
        if self._reg_out is None:
            self._reg_out = torch.zeros(1, dtype=F32, device=st.flat.device)
        if st.n_reg > 0 and self.wd:
            self.g.workspace()
            ops.sum_squares(st.flat[:st.n_reg], 0.5 * self.wd, self._reg_out, self.g.ws_small)
        return self._reg_out

    # grad_norm() / clipped_steps() / nonfinite_steps() of an optimiser built with clip_norm: each READS THE DEVICE (a
    # sync), for logging only
    def _clip_or_raise(self):
        if self.clip is None:
            raise RuntimeError("this optimiser was built without clip_norm")
        return self.clip

    def grad_norm(self):
        """Global norm of the un-scaled gradients of the LAST step (inf / NaN: that step was skipped)."""
        return self._clip_or_raise().grad_norm()

    def clipped_steps(self):
        return self._clip_or_raise().clipped_steps()

    def nonfinite_steps(self):
        return self._clip_or_raise().nonfinite_steps()


class AdamOptimizer(Optimizer):
    """tf.train.AdamOptimizer + ExponentialMovingAverage(decay, num_updates=global_step) + slim L2
    regulariser gradient, as ONE fused launch over the tower's flat parameter buffer."""
    # `tf.train.Saver(tf.global_variables())` (multigpu_train.py:144) also saves the optimiser's slot
    # variables `<var>/Adam`, `<var>/Adam_1`, the scalars `beta1_power`, `beta2_power` and
    # `global_step`; a resumed run continues the LR staircase, the bias correction and the EMA warm-up
    STEP, SLOTS, BUFFERS = "adam_step", ("Adam", "Adam_1"), {"Adam": "m", "Adam_1": "v"}

    def __init__(self, graph, learning_rate=1e-4, decay_steps=5000, decay_rate=0.94,
                 moving_average_decay=0.997, weight_decay=1e-5, beta1=0.9, beta2=0.999, epsilon=1e-8,
                 clip_norm=None):
        super().__init__(graph, moving_average_decay, weight_decay, clip_norm)
        self.lr0, self.decay_steps, self.decay_rate = learning_rate, decay_steps, decay_rate
        self.b1, self.b2, self.eps = beta1, beta2, epsilon

    def learning_rate(self):
        return exponential_decay(self.lr0, self.global_step, self.decay_steps, self.decay_rate, True)

    def _launch(self, entry, st, tail):
        t = self.global_step + 1
        lr_t = self.learning_rate() * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
        entry(st.flat, st.flat_grad, self.m, self.v, self.ema, st.n_reg, lr_t, self.b1, self.b2, self.eps, self.wd, *tail)

    def scalar_state_dict(self):
        t = self.global_step
        return {"beta1_power": np.float32(self.b1 ** (t + 1)), "beta2_power": np.float32(self.b2 ** (t + 1))}


class MomentumOptimizer(Optimizer):
    """tf.train.MomentumOptimizer(lr, 0.9) with the PixelLink schedule (train_pixellink.py:222-243)."""
    STEP, SLOTS, BUFFERS = "momentum_step", ("Momentum",), {"Momentum": "acc"}

    def __init__(self, graph, base_lr=0.01, momentum=0.9, weight_decay=5e-4, moving_average_decay=None, clip_norm=None):
        super().__init__(graph, moving_average_decay, weight_decay, clip_norm)
        self.base_lr, self.momentum = base_lr, momentum

    def learning_rate(self):
        return pixellink_lr(self.global_step, self.base_lr)

    def _launch(self, entry, st, tail):
        entry(st.flat, st.flat_grad, self.acc, self.ema, st.n_reg, self.learning_rate(), self.momentum, self.wd, *tail)

    def scalar_state_dict(self):
        return {}


class TrainStep:
    """One data-parallel training step of `multigpu_train.py`'s hot loop (:118-142,171-174) for
    this process's tower: forward -> loss -> backward (gradient buckets all-reduced while the rest
    of backward runs) -> optimiser + EMA.

    `forward_loss(graph, *batch) -> loss`.  The step has static shapes, buffers and launch order,
    so after two eager steps (variable creation, optimiser creation) the third is RECORDED as a
    flat list of C-ABI calls (`_lib.Recorder`) and every later step REPLAYS that list: the Python
    graph/tape logic, ~700 ctypes marshalling round trips and all per-step allocations disappear
    from the hot loop (the host was the bottleneck at ~40 ms/step).  New input data is copied into
    the recorded input buffers; `replay=False` keeps every step eager.

    Everything between the batch tensors and the loss must therefore be C-ABI calls: input
    preprocessing written with torch operators belongs in the input pipeline, before the step (where
    the reference has it too — its queues deliver preprocessed images).  The recording runs under an
    audit that raises if a torch operator touched device memory inside `forward_loss`.

    `accumulate_steps=K` (gradient accumulation, `GradAccum`): one optimiser step per WINDOW of K calls, on the mean of
    the K micro-batch gradients.  A call that does not close its window runs forward, loss, backward, the accumulate
    calls and the phase's advance, and nothing else: no exchange, no check or clip pass, no optimiser, no re-pack.  The
    closing call adds the window's sum into the flat gradient buffer and then runs everything on it, with 1 / K in the
    optimiser's factor.  The step is recorded on a closing call, and a non-closing replay skips the plan's exchange,
    optimiser and re-pack entries by their tags; the accumulate entries are the same in every phase (the device picks
    the rule).  K = 1, the default, allocates and launches nothing of this."""

    def __init__(self, graph, forward_loss, optimizer_factory, world_size=1, bucket_bytes=32 << 20,
                 replay=True, grad_op="mean", force_reduce=False, comm_proxy=None, accumulate_steps=1):
        """grad_op: "mean" = multigpu_train.py's `average_gradients` (each tower differentiates its own
        loss, the gradients are averaged); "sum" = train_pixellink.py's `sum_gradients`: each clone
        differentiates loss / num_clones (:264) and the gradients are summed (:179-194).
        force_reduce: run the bucketed exchange at world 1 too (needs a one-rank process group)."""
        if grad_op not in ("mean", "sum"):
            raise ValueError("grad_op must be 'mean' or 'sum'")
        self.accumulate_steps = check_accumulate_steps(accumulate_steps)        # before anything is allocated
        self.accum = None                 # GradAccum, created with the optimiser and the reducer when accumulate_steps > 1
        self.window_pos = 0               # calls since the first window opened (or since reset_window)
        self.closes_window = False        # whether the call just made stepped the optimiser
        self.g = graph
        self.grad_op = grad_op
        self.force_reduce = force_reduce
        self.comm_proxy = comm_proxy      # (workgroups, link GB/s): dist.GradientAllReduce(proxy=...), a measurement aid
        self.backward_end_event = None    # bench.py: recorded on the compute stream in front of the first wait for a bucket
        if grad_op == "sum":
            graph.loss_div = float(world_size)       # total_clone_loss = sum(losses) / num_clones
        self.forward_loss = forward_loss
        self.optimizer_factory = optimizer_factory
        self.world = world_size
        self.bucket_bytes = bucket_bytes
        self.opt = None
        self.reducer = None
        self.replay = replay
        self.steps = 0
        self.plan = None                  # the list of entries replayed (bench.py reads it); plan_kinds: step_plan.kinds of it
        self.plan_kinds = None
        self.static_batch = None
        self.loss = None
        self.guest_stream = self.guest_ptr = self.guest_event = None      # schedule_guests: the paired guest passes' stream
        self._packed_version = None

    def build(self, *batch):
        """Create the variables, the flat buffers, the optimiser and the reducer WITHOUT taking a
        step: one forward pass on `batch` whose side effects (BN moving-statistics update) are undone.
        After it `graph.store` / `self.opt` can be restored from a checkpoint before the first update
        (the reference restores before its first `sess.run(train_op)`, multigpu_train.py:153-158)."""
        if self.opt is not None:
            return self
        g = self.g
        g.reset_tape()
        # the dry-run forward updates the BN moving statistics: put back what was there BEFORE it (variables that
        # exist already may hold loaded statistics; the ones the dry run creates start from their initial value)
        before = {n: g.store.vars[n].data.clone() for n in g.store.order if not g.store.vars[n].trainable}
        self.forward_loss(g, *batch)
        g.reset_tape()
        self.opt = self.optimizer_factory(g)
        g.store.reset_non_trainable()
        for n, t in before.items():
            g.store.vars[n].data.copy_(t)
        self._make_reducer()
        return self

    def _make_reducer(self):
        from .dist import GradientAllReduce
        if self.accumulate_steps > 1:
            self.accum = GradAccum(self.accumulate_steps, self.g.store.flat_grad)
        self.reducer = GradientAllReduce(self.g.store, self.world, self.bucket_bytes, op=self.grad_op,
                                         fold_mean=True, force=self.force_reduce, proxy=self.comm_proxy, accum=self.accum)

    @property
    def micro_step(self):
        """Host mirror of the phase: the index, inside its window, of the NEXT call (0 .. accumulate_steps - 1)."""
        return self.window_pos % self.accumulate_steps

    def reset_window(self):
        """Start a fresh window with the next call (after restoring a checkpoint mid-run): the device block and the
        host mirror go back to micro-step 0; whatever the abandoned window had accumulated is overwritten by the
        first micro-step's store rule."""
        self.window_pos = 0
        if self.accum is not None:
            self.accum.reset()

    def _grad_scale(self):
        """The optimiser's host factor: the reducer's (1 or 1 / world), over K for the window's mean."""
        gs = self.reducer.grad_scale
        return gs if self.accumulate_steps == 1 else gs / self.accumulate_steps

    def summary_factor(self):
        """(mul_host, mul_dev) for `summary.TensorStats.run(store.flat_grad, ...)` behind a call that stepped the
        optimiser: the factor that step's optimiser kernel multiplied the gradients with, its device part left on the
        device (a 1-element f32 view of the clip state's g_mul or of the loss-scale state's inv_scale_used; None: 1).
        No device read."""
        return self.opt.factor.summary_factor(self._grad_scale())

    # -- eager / recording path --------------------------------------------------------------
    def _eager(self, batch, record):
        from . import _lib
        g = self.g
        g.reset_tape()
        if record:
            rec = _lib.Recorder()
            _lib.RECORDER = rec
            g.keepalive = []
            if self.accumulate_steps > 1:
                # the call before this one ran at the same store version and refreshed the lazily packed operands (conv1_1's
                # among them); recorded as it stands, this step would hold no refresh of them and replay stale weights
                g.stale_lazy_packs()
        audit = _record_audit() if record else contextlib.nullcontext()
        try:
            with audit:
                loss = self.forward_loss(g, *batch)
            if record and audit.offenders:
                raise RuntimeError(
                    "torch operators inside the recorded step would not be replayed: %s — move them "
                    "before the step (input pipeline) or use replay=False" % sorted(set(audit.offenders)))
            if self.opt is None:
                self.opt = self.optimizer_factory(g)           # materialises the flat buffers
                self._make_reducer()
            closing = self.accum is None or self.accum.closing
            self.reducer.closing = closing
            g.backward(self.reducer.on_grads_ready if self.reducer.active else None)
            if self.accum is not None and not self.reducer.active:
                self.accum.run()            # no buckets: one call over the whole buffer (an active reducer: per bucket, _fire)
            self.reducer.finish()           # records itself: host callback (torch mode) or C-ABI stream waits (abi mode)
            if self.accum is not None:
                self.accum.advance()        # behind every accumulate call of the step
        finally:
            _lib.RECORDER = None
        self.loss = loss
        if not closing:                     # (never a recording step)
            return loss
        self.opt.apply_gradients(self._grad_scale())
        self._repack()                      # the conv operand packs of the new weights, one launch
        if record:
            rec.py(lambda: self.opt.apply_gradients(self._grad_scale()))
            rec.entries[-1].append("opt")
            rec.py(self._repack)
            rec.entries[-1].append("repack")
            self.recorded = rec.entries                       # (kept: reschedule() derives another plan from the same recording)
            self._set_plan(self._schedule(rec.entries) if USE_GUESTS else rec.entries)
            self.static_batch = list(batch)
            self.keepalive, g.keepalive = g.keepalive, None
            g.reset_tape()
        self.loss = loss
        return loss

    def reschedule(self, **kw):
        """Another guest / exchange placement of the SAME recorded step (schedule_guests keywords): bench.py's A/B arms."""
        if self.plan is not None and USE_GUESTS:
            self._set_plan(self._schedule(self.recorded, **kw))

    def _schedule(self, entries, **kw):
        """schedule_guests under this module's switches (a caller's keywords first)."""
        sw = dict(cover=GUEST_COVER, min_us=GUEST_MIN_US, xchg_at_fork=XCHG_AT_FORK, balance=GUEST_BALANCE,
                  paired_grid=GUEST_PAIRED_GRID)
        sw.update((k, v) for k, v in kw.items() if v is not None)
        return schedule_guests(entries, **sw)

    def _set_plan(self, plan):
        self.plan, self.plan_kinds = plan, step_plan.kinds(plan)

    def _repack(self):
        """Batched re-pack of the [tap][cout][cin] / [tap][cin][cout] operand copies from the f32 masters, stamped
        with the store version it saw: a replayed plan holds no lazy refresh of these packs, so `_replay` compares
        the stamp and re-packs first when the masters changed outside the step (load_state_dict, a restored
        checkpoint, an EMA swap)."""
        self.g.repack_all()
        self._packed_version = self.g.store.version

    def _replay(self, batch):
        if self.g.store.version != self._packed_version:
            self._repack()
        for dst, src in zip(self.static_batch, batch):
            if src is not dst:
                dst.copy_(src, non_blocking=True)
        closing = self.accum is None or self.accum.closing
        self.reducer.closing = closing      # (torch mode: the exchange's host callbacks ask it)
        if self.guest_stream is None and "fork" in self.plan_kinds:
            # a weight gradient and the guest pass paired with it (schedule_guests) run on two streams
            self.guest_stream = torch.cuda.Stream()
            self.guest_ptr = ctypes.c_void_p(self.guest_stream.cuda_stream)
            self.guest_event = torch.cuda.Event()
        step_plan.run_plan(self.plan, self.plan_kinds, step_plan.Replay(
            torch.cuda.current_stream(), self.guest_stream, self.guest_ptr, self.guest_event, self.reducer, closing,
            self.backward_end_event, ops.KERNEL_TIMING))
        if self.accum is not None:
            self.accum.micro = (self.accum.micro + 1) % self.accum.k      # the plan's advance entry has moved the device's
        return self.loss

    def __call__(self, *batch):
        self.steps += 1
        closing = self.micro_step == self.accumulate_steps - 1
        if self.plan is not None:
            loss = self._replay(batch)
        else:
            # step 1 creates variables, step 2 runs with the flat buffers; step 3 is steady state.  With accumulation the
            # recording waits for a call that closes its window: every entry of the plan is then executed as it is recorded
            loss = self._eager(batch, record=self.replay and self.steps >= 3 and closing)
        self.window_pos += 1
        self.closes_window = closing
        return loss
