"""Host-side plumbing that stands in for the TF-1.4 graph/session the reference drives
(`tf.variable_scope`, `tf.get_variable`, `opt.compute_gradients`): a variable store with
TF-slim variable names, activation handles, and a reverse-mode tape.

Nothing here computes: every FLOP happens in libocr_hip.so via `ops`.  torch is used for
device memory only.
"""
import collections
import contextlib
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import ops

# F16 = the library's 16-bit storage dtype (IEEE half, or bfloat16 under OCR_STORAGE=bf16)
F16, F32 = (torch.bfloat16 if L.STORAGE == "bf16" else torch.float16), torch.float32


class Variable:
    """A TF variable: f32 master copy in the store's flat buffer, optional gradient view."""

    def __init__(self, name, shape, init, trainable, regularized):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.init = init            # numpy f32 until the store is materialised
        self.trainable = trainable
        self.regularized = regularized
        self.data = None            # torch f32 view
        self.grad = None            # torch f32 view (trainable only)
        self.packed = {}            # kind -> (version, tensor)

    @property
    def size(self):
        return int(np.prod(self.shape)) if self.shape else 1


class VariableStore:
    """Name -> Variable, materialised as flat f32 device buffers:
    [regularised trainables | other trainables] for params / grads (one Adam launch, one
    all-reduce bucket list) and a second flat buffer for non-trainables (BN moving stats)."""

    def __init__(self, device):
        self.vars = {}
        self.order = []
        self.device = device
        self.version = 0            # bumped by every optimiser step -> f16 packs are stale
        self.flat = self.flat_grad = self.flat_aux = None
        self.n_reg = 0

    def get(self, name, shape, initializer, trainable=True, regularized=False):
        v = self.vars.get(name)
        if v is not None:
            if tuple(shape) != v.shape:
                raise ValueError("variable %s exists with shape %s, requested %s" % (name, v.shape, tuple(shape)))
            return v
        if self.flat is not None:
            raise RuntimeError("variable %s created after the store was materialised" % name)
        init = np.ascontiguousarray(np.asarray(initializer(tuple(shape)), dtype=np.float32).reshape(shape))
        # non-trainables (BN moving statistics: small vectors) keep their initial value so that a
        # variable-creating dry run can be undone (train.TrainStep.build)
        v = Variable(name, shape, None if trainable else init, trainable, regularized)
        v.data = torch.from_numpy(init).to(self.device)
        if trainable:
            v.grad = torch.zeros_like(v.data)
        self.vars[name] = v
        self.order.append(name)
        return v

    def materialise(self):
        """Gather every variable into the flat buffers (idempotent); views replace the
        per-variable tensors used while the graph was being built."""
        if self.flat is not None:
            return
        tr = [self.vars[n] for n in self.order if self.vars[n].trainable]
        reg = [v for v in tr if v.regularized]
        oth = [v for v in tr if not v.regularized]
        aux = [self.vars[n] for n in self.order if not self.vars[n].trainable]

        def pack(vs, pad=4):
            offs, o = [], 0
            for v in vs:
                offs.append(o)
                o += (v.size + pad - 1) // pad * pad   # keep every view 16-byte aligned
            return offs, o

        offs_r, nr = pack(reg)
        offs_o, no = pack(oth)
        offs_a, na = pack(aux)
        self.n_reg = nr
        self.flat = torch.zeros(max(nr + no, 1), dtype=F32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.flat_aux = torch.zeros(max(na, 1), dtype=F32, device=self.device)
        for v, o in list(zip(reg, offs_r)) + [(v, nr + o) for v, o in zip(oth, offs_o)]:
            view = self.flat[o:o + v.size].view(v.shape)
            view.copy_(v.data)
            gview = self.flat_grad[o:o + v.size].view(v.shape)
            gview.copy_(v.grad)
            v.data, v.grad = view, gview
        for v, o in zip(aux, offs_a):
            view = self.flat_aux[o:o + v.size].view(v.shape)
            view.copy_(v.data)
            v.data = view

    def trainable(self):
        return [self.vars[n] for n in self.order if self.vars[n].trainable]

    def reset_non_trainable(self):
        """Moving statistics back to their initial values (0 / 1)."""
        for n in self.order:
            v = self.vars[n]
            if not v.trainable and v.init is not None:
                v.data.copy_(torch.from_numpy(v.init))

    def by_variable(self, flat_like):
        """{variable name: numpy copy} of a buffer laid out like `flat` (gradients, optimiser slots, EMA)."""
        base = self.flat.data_ptr()
        out = {}
        for v in self.trainable():
            off = (v.data.data_ptr() - base) // 4
            out[v.name] = flat_like[off:off + v.size].view(v.shape).detach().cpu().numpy().copy()
        return out

    def load_by_variable(self, flat_like, sd):
        """Inverse of `by_variable` for the names present in `sd`; returns the names loaded."""
        base = self.flat.data_ptr()
        done = []
        for v in self.trainable():
            if v.name in sd:
                off = (v.data.data_ptr() - base) // 4
                a = np.asarray(sd[v.name], dtype=np.float32).reshape(v.shape)
                flat_like[off:off + v.size].view(v.shape).copy_(torch.from_numpy(a))
                done.append(v.name)
        return done

    def state_dict(self):
        return {n: self.vars[n].data.detach().cpu().numpy().copy() for n in self.order}

    def load_state_dict(self, sd, strict=True):
        for n, arr in sd.items():
            if n not in self.vars:
                if strict:
                    raise KeyError(n)
                continue
            v = self.vars[n]
            a = np.asarray(arr, dtype=np.float32).reshape(v.shape)
            v.data.copy_(torch.from_numpy(a))
        self.version += 1


class BnCtx(NamedTuple):
    """Act.bn_ctx / Act.bias_ctx: what a consumer's input-gradient epilogue needs to sum the producer's BN-backward terms."""
    y: object
    scale: object
    shift: object
    mean: object
    invstd: object
    relu: bool

    @classmethod
    def of_bias(cls, g, y, cout):
        """A bias + ReLU producer in the same form: `y` is the activation, scale 1, shift 0, mean 0, 1/std 1."""
        one, zero = g.const_vec(cout, 1.0), g.const_vec(cout, 0.0)
        return cls(y, one, zero, zero, one, True)

    def first(self):
        """conv1_1 whose `y` is an ops.LazyFirstY: (x4, w_first, scale, shift, mean, invstd, relu), the order in which
        ocr_conv2d_bnred_first_f16 takes them (y is evaluated again from the image, not read)."""
        return (self.y.x4, self.y.w_first) + self[1:]


class TailCtx(NamedTuple):
    """Act.tail_ctx: the unit's last conv (y, mean, invstd), the unit's output and its ReLU-mask bits (None: read `out`)."""
    y: object
    mean: object
    invstd: object
    out: object
    bits: object = None


class TailFwd(NamedTuple):
    """Act.tail_fwd: the deferred relu(bn(y) + bn?(shortcut)) of a bottleneck output."""
    y: object
    scale: object
    shift: object
    shortcut: object
    sc_scale: object
    sc_shift: object
    bits: object


class BnFwd(NamedTuple):
    """Act.bn_fwd: a deferred relu?(bn(y))."""
    y: object
    scale: object
    shift: object
    relu: bool


class PoolGrad(NamedTuple):
    """Act.pool_grad: a max-pool's backward left to the producer; pad = (top, left)."""
    grad: object
    argmax: object
    k: int
    stride: int
    pad: tuple


class Partial(NamedTuple):
    """Act.bn_partial / bias_partial / tail_partial: [T, 2, channels] f32 rows of a fused input-gradient epilogue."""
    rows: object
    T: int


class Act:
    """Activation handle: device tensor + (lazily created) gradient.

    `data` may be DEFERRED: a ResNet bottleneck's output relu(bn(conv3) + shortcut) is not computed when the unit is
    built — the next 1x1 convolution that consumes it computes it while loading its operand and writes it back
    (resnet_layers.conv_bn_raw, ocr_conv2d_pw_bnaddrelu_f16).  Any other access to `.data` runs the plain
    element-wise pass first, so consumers that know nothing about this stay correct."""

    __slots__ = ("_data", "grad", "requires_grad", "name", "deferred", "consumed", "sole_consumer",
                 # the handshake between the layer that produced this activation and the layers that read it (below)
                 "bn_fwd", "tail_fwd", "bn_ctx", "bias_ctx", "tail_ctx", "takes_pool_grad", "pending", "pending_owner",
                 "bn_partial", "bias_partial", "tail_partial", "first_s1", "sub_grad", "pool_grad", "bias_done")

    def __init__(self, data, requires_grad=True, name=""):
        self._data = data
        self.grad = None
        self.requires_grad = requires_grad
        self.name = name
        self.deferred = None      # callable that fills _data (the plain pass), while nobody has computed it yet
        self.consumed = False     # a convolution has read it already (tail fusion must then stay off: build order)
        self.sole_consumer = False  # set by the NET for activations read by exactly one convolution (nets/vgg.py)
        # --- The fusion handshake.  Three groups of slots, all None / False until somebody speaks:
        # OFFERS, set once by the PRODUCER when it is built and never cleared.  Forward: a deferred activation that a
        # fusing reader (a 1x1 convolution, a max-pool) evaluates itself.  Backward: what the reader's input-gradient
        # launch needs to do part of the producer's backward in its epilogue (layers.select_input_grad picks the route).
        self.bn_fwd = None        # BnFwd: relu?(bn(y))                                  (conv_bn_act(defer), root_block)
        self.tail_fwd = None      # TailFwd: relu(bn(y3) + shortcut)                     (bottleneck)
        self.bn_ctx = None        # BnCtx of the conv + BN that made it                  (conv2d, conv_bn_act)
        self.bias_ctx = None      # BnCtx.of_bias of the conv + bias + ReLU that made it (conv2d); honoured for a sole_consumer
        self.tail_ctx = None      # TailCtx of the bottleneck that made it
        self.takes_pool_grad = False   # the producer's backward can gather its gradient from a max-pool's operands
        # COUNTDOWN, set by the bottleneck that READS a bottleneck output twice (conv1 + shortcut): its `pending`
        # contributions are counted down by count_contribution (only those made for `pending_owner`) and by the
        # shortcut's backward; the one that reaches 0 is the LAST contribution and takes the tail route.  The producer's
        # backward sets `pending` back to None.
        self.pending = None
        self.pending_owner = None
        # ANSWERS, left by a READER's backward and cleared by the PRODUCER's backward when it has used them:
        self.bn_partial = None    # Partial: the BN-backward sums over the gradient the reader stored ...
        self.bias_partial = None  # Partial: ... or the bias-gradient sums; `grad` is then dz, past the ReLU
        self.tail_partial = None  # Partial: `grad` is complete and past the output's ReLU, conv3's BN-backward sums
        self.first_s1 = None      # conv1_1's activation: the sums its weight gradient is finished from, left INSTEAD of
                                  # the gradient (`grad` stays None) together with bn_partial
        self.sub_grad = None      # gradient of this output's stride-2 subsample, waiting for the tail launch to add it
        self.pool_grad = None     # PoolGrad: the pool wrote nothing, the producer gathers (takes_pool_grad)
        self.bias_done = False    # the layer's own pool already produced dz and the bias gradient (layers.max_pool2d)
        # bn_partial and bias_partial describe the FIRST contribution only: a contribution that accumulates into `grad`
        # drops them (open_grad), and the producer then reduces (masks: idempotent) the whole sum itself.  tail_partial
        # and first_s1 need no such rule: the countdown / the net's sole_consumer say that nothing follows them.

    def open_grad(self, g):
        """-> (grad, accumulating): the buffer the next gradient contribution goes into — allocated here by the first
        one; a later one adds to it, and what the first one's fused epilogue left no longer covers the whole gradient."""
        accumulating = self.grad is not None
        if accumulating:
            self.bn_partial = self.bias_partial = None
        else:
            self.grad = g.empty(self.shape)
        return self.grad, accumulating

    def count_contribution(self, owner):
        """-> whether this is the LAST gradient contribution to a bottleneck output.  Only the owning unit's two are
        counted (any other consumer was built later, runs earlier in the backward pass and has added its share)."""
        if self.pending is None or owner is None or owner is not self.pending_owner:
            return False
        self.pending -= 1
        assert self.pending >= 0, "more gradient contributions than the owning unit has consumers"
        return self.pending == 0

    @property
    def data(self):
        if self.deferred is not None:
            fill, self.deferred = self.deferred, None
            fill()
        return self._data

    @data.setter
    def data(self, value):
        self._data = value

    @property
    def shape(self):
        return tuple(self._data.shape)


class DynamicLossScale:
    """Dynamic loss scaling for f16 training, decided ON THE DEVICE: `Graph(..., loss_scale=DynamicLossScale(...))`.

    The scale, the per-step overflow flag and the skip decision live in one small device block (`ocr_loss_scale_state`,
    include/ocr_hip.h).  The loss kernels read the scale from it (`ops.*_bwd_dyn`), `ops.grad_check` — one pass over the
    flat gradient buffer behind the all-reduce — looks for inf / NaN and moves the state, and the optimiser kernel
    (`ops.adam_step_dyn` / `ops.momentum_step_dyn`) returns without a single store when the step is to be skipped.  No
    host read happens anywhere on that path, so a recorded step plan (train.TrainStep) never changes.

    State machine, once per step: an overflow skips the step, multiplies the scale by `backoff_factor` (not below
    `min_scale`) and clears the run of clean steps; `growth_interval` clean steps in a row multiply it by `growth_factor`
    (not above `max_scale`).

    HOST counters do not know about skips: `global_step` — hence the learning-rate staircase, Adam's bias correction and
    the EMA warm-up — advances on a skipped step too, as a learning-rate schedule usually does under dynamic scaling (the
    alternative is a device-to-host sync in every step; skips are rare).  `store.version` advances as well; the re-pack
    that follows re-creates the same operand copies.

    `scale()`, `skipped_steps()`, `good_steps()` and `state_dict()` READ THE DEVICE (a sync): for logging and
    checkpoints, never inside a step.  The Graph works on its own bound copy (`graph.loss_scaler`), so one instance can
    configure several graphs."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0,
                 max_scale=2.0 ** 24):
        vals = dict(init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor, min_scale=min_scale,
                    max_scale=max_scale)
        for k, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v <= 0:
                raise ValueError("%s must be a positive finite number, got %r" % (k, v))
        if not (backoff_factor < 1.0 < growth_factor):
            raise ValueError("need backoff_factor < 1 < growth_factor, got %r, %r" % (backoff_factor, growth_factor))
        if not (min_scale <= init_scale <= max_scale):
            raise ValueError("need min_scale <= init_scale <= max_scale, got %r, %r, %r" % (min_scale, init_scale, max_scale))
        if isinstance(growth_interval, bool) or int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError("growth_interval must be a positive integer, got %r" % (growth_interval,))
        f32 = lambda v: float(np.float32(v))           # what the kernels will see
        self.init_scale, self.growth_factor, self.backoff_factor = f32(init_scale), f32(growth_factor), f32(backoff_factor)
        self.min_scale, self.max_scale = f32(min_scale), f32(max_scale)
        self.growth_interval = int(growth_interval)
        self.device = None
        self._state = None                                      # int32 [8] on the device, created on first use
        self._host = {"scale": self.init_scale, "good_steps": 0, "skipped_total": 0}    # the values until then

    def bind(self, device):
        """A copy of the configuration with device state of its own (Graph.__init__)."""
        b = DynamicLossScale(self.init_scale, self.growth_factor, self.backoff_factor, self.growth_interval, self.min_scale,
                             self.max_scale)
        b.device = torch.device(device)
        return b

    @property
    def state(self):
        """The device block (ops.LOSS_SCALE_WORDS 32-bit words).  Created outside any recording: the initialising launch
        must not become part of a replayed plan."""
        if self._state is None:
            if self.device is None:
                raise RuntimeError("this DynamicLossScale is a configuration only: Graph(loss_scale=...) binds a copy to its device")
            st = torch.empty(ops.LOSS_SCALE_WORDS, dtype=torch.int32, device=self.device)
            rec, L.RECORDER = L.RECORDER, None
            try:
                ops.loss_scale_init(st, self._host["scale"])
            finally:
                L.RECORDER = rec
            if self._host["good_steps"] or self._host["skipped_total"]:
                st[ops.LS_GOOD_STEPS:ops.LS_SKIPPED_TOTAL + 1].copy_(
                    torch.tensor([self._host["good_steps"], self._host["skipped_total"]], dtype=torch.int32))
            self._state = st
        return self._state

    @property
    def scale_ptr(self):
        """1-element f32 view of the state's `scale` word: what the *_bwd_dyn loss kernels take."""
        return self.state[ops.LS_SCALE:ops.LS_SCALE + 1].view(torch.float32)

    def _words(self):
        if self._state is None:
            return None
        return self._state.cpu().numpy()

    def scale(self):
        """The scale the NEXT backward pass will use (device read: a sync)."""
        w = self._words()
        return self._host["scale"] if w is None else float(w[ops.LS_SCALE:ops.LS_SCALE + 1].view(np.float32)[0])

    def skipped_steps(self):
        w = self._words()
        return self._host["skipped_total"] if w is None else int(w[ops.LS_SKIPPED_TOTAL])

    def good_steps(self):
        w = self._words()
        return self._host["good_steps"] if w is None else int(w[ops.LS_GOOD_STEPS])

    def check(self, grad):
        """ops.grad_check on `grad` with this configuration (the optimisers call it behind the all-reduce)."""
        ops.grad_check(grad, self.state, self.growth_factor, self.backoff_factor, self.growth_interval, self.min_scale,
                       self.max_scale)

    def state_dict(self):
        return {"scale": np.float32(self.scale()), "good_steps": np.int64(self.good_steps())}

    def load_state_dict(self, sd=None):
        """Restore `scale` and `good_steps`; None / a dict without them (an older checkpoint) restores `init_scale`."""
        sd = sd or {}
        scale = float(np.float32(sd["scale"])) if "scale" in sd else self.init_scale
        good = int(sd["good_steps"]) if "good_steps" in sd and "scale" in sd else 0
        if not (math.isfinite(scale) and scale > 0):
            raise ValueError("loss scale must be positive and finite, got %r" % scale)
        scale = min(max(scale, self.min_scale), self.max_scale)
        good = max(0, min(good, self.growth_interval - 1))
        self._host.update(scale=scale, good_steps=good, skipped_total=self.skipped_steps())
        if self._state is not None:
            host = np.zeros(2, dtype=np.int32)
            host[:1].view(np.float32)[0] = scale
            host[1:2].view(np.float32)[0] = np.float32(1.0) / np.float32(scale)
            self._state[ops.LS_SCALE:ops.LS_INV_SCALE_USED + 1].copy_(torch.from_numpy(host))
            self._state[ops.LS_GOOD_STEPS:ops.LS_GOOD_STEPS + 1].copy_(torch.tensor([good], dtype=torch.int32))


def parse_loss_scale(text):
    """The training scripts' `--loss_scale` value: "dynamic" -> DynamicLossScale() with its defaults, a number -> that
    constant scale (a float)."""
    if isinstance(text, str) and text.strip().lower() == "dynamic":
        return DynamicLossScale()
    try:
        v = float(text)
    except (TypeError, ValueError):
        raise ValueError("loss_scale must be 'dynamic' or a number, got %r" % (text,))
    if not (math.isfinite(v) and v > 0):
        raise ValueError("loss_scale must be positive and finite, got %r" % (text,))
    return v


LossSeed = collections.namedtuple("LossSeed", "factor scale_ptr")


class Graph:
    """One tower: variable store + tape + scratch.  `loss_scale` multiplies the loss gradient so
    that f16 activation gradients stay in range; the optimiser divides it out."""

    def __init__(self, device="cuda:0", loss_scale=1024.0, seed=1, precision="f16", fold_bn=False):
        """precision: "f16" = the product path (f16 storage, f32 accumulate, MFMA kernels);
        "f32" = forward-only f32 INFERENCE precision (f32 storage and arithmetic, the convolutions on the matrix
        cores with v_mfma_f32_32x32x2_f32: layers_f32.py, csrc/f32_infer.hip): whole-graph outputs within 1e-3 of the
        f32 reference (the north star's tolerance), ~10x the time of the 16-bit path;
        "f16x2" = the same forward-only f32 graph (f32 storage, the same element-wise kernels) with every convolution on
        the 16-bit matrix cores: each f32 operand is carried as two IEEE halves (hi, and the residual scaled by 2^11) and
        a product costs three v_mfma_f32_16x16x32_f16 (ocr_conv2d_f32_split, csrc/f16x2_infer.hip): the accuracy of "f32",
        faster.  Operand range: |x|, |w| < 65504; larger values saturate (finite, wrong); NaN stays NaN.
        `precision` holds the STORAGE family the layer modules dispatch on ("f16" | "f32"; "f16x2" is stored as "f32"),
        `precision_name` the name given here, `f32_conv_route` the ops.conv2d_f32 route of the f32 family (None: the
        process default ops.F32_CONV; "split").
        fold_bn ("f32" / "f16x2" only): a layer whose batch norm runs in inference mode (moving statistics) launches ONE
        convolution that applies the normalisation, the bottleneck's residual add and the ReLU in its epilogue, and
        conv2d_same layers run at their real stride (layers_f32.py; ocr_conv2d_f32_mfma_ep / ocr_conv2d_f32_split_ep).
        False: every graph launches what it always launched.
        loss_scale: a number = the constant f16 loss scale; a `DynamicLossScale` ("f16" only) = a scale kept on the device
        that backs off when a gradient overflows (the step is skipped) and grows after a run of clean steps:
        `loss_scaler` is then this graph's bound copy of it (None for a constant), `loss_scale` its initial value."""
        if precision not in ("f16", "f32", "f16x2"):
            raise ValueError("precision must be 'f16', 'f32' or 'f16x2'")
        if fold_bn and precision not in ("f32", "f16x2"):
            raise ValueError("fold_bn needs precision 'f32' or 'f16x2' (the f16 path carries its batch norm already)")
        self.fold_bn = bool(fold_bn)
        self.precision_name = precision
        self.precision = "f32" if precision == "f16x2" else precision
        self.f32_conv_route = "split" if precision == "f16x2" else None
        self.device = torch.device(device)
        self.store = VariableStore(self.device)
        self.tape = []
        self.scope = []
        if isinstance(loss_scale, DynamicLossScale):
            if precision != "f16":
                raise ValueError("DynamicLossScale needs precision 'f16' (the %s inference precision has no backward pass)"
                                 % precision)
            self.loss_scaler = loss_scale.bind(self.device)
            self.loss_scale = self.loss_scaler.init_scale
        else:
            self.loss_scaler = None
            self.loss_scale = float(loss_scale)
        self.loss_div = 1.0          # train_pixellink.py:264: each clone's loss is divided by num_clones
        self.rng = np.random.default_rng(seed)
        self.ws = None
        self.ws_small = None
        self.ws_wgrad = None
        self.ws_split = None
        self.collections = {"losses": [], "update_ops": []}
        self.keepalive = None        # list while a step is being recorded (train.TrainStep)
        self._const_vecs = {}

    # --- scopes / variables (tf.variable_scope, tf.get_variable) ---
    @contextlib.contextmanager
    def variable_scope(self, name):
        if name:
            self.scope.append(name)
        try:
            yield
        finally:
            if name:
                self.scope.pop()

    def full_name(self, name):
        return "/".join(self.scope + [name])

    def get_variable(self, name, shape, initializer, trainable=True, regularized=False):
        return self.store.get(self.full_name(name), shape, initializer, trainable, regularized)

    def seed_scale(self):
        """d(loss)/d(loss) the loss kernels start the backward pass from: the f16 loss scale, over
        the clone count when the caller pre-divides its loss (grad_op="sum")."""
        return self.loss_scale / self.loss_div

    def loss_seed(self):
        """The same seed as a record, for either kind of loss scale: `factor` is the host's share of it (the whole seed
        for a constant scale, 1 / loss_div for a dynamic one), `scale_ptr` the device's (the scaler's scale word, or None).
        `losses.launch_seed` starts a loss family's backward entry from it."""
        if self.loss_scaler is not None:
            return LossSeed(1.0 / self.loss_div, self.loss_scaler.scale_ptr)
        return LossSeed(self.seed_scale(), None)

    # --- device memory ---
    def workspace(self):
        if self.ws is None:
            self.ws = ops.Workspace(self.device, 256 << 20)
            self.ws_small = ops.Workspace(self.device, 8 << 20)
            self.ws_wgrad = ops.Workspace(self.device, 160 << 20)   # weight-gradient slabs (side stream)
        return self.ws

    def split_workspace(self):
        """The tower's packed-weight arena of the "split" convolution route (ops.conv2d_f32), created on first use."""
        if self.ws_split is None:
            self.ws_split = ops.Workspace(self.device, 1 << 20)
        return self.ws_split

    def empty(self, shape, dtype=F16):
        t = torch.empty(shape, dtype=dtype, device=self.device)
        if self.keepalive is not None:
            self.keepalive.append(t)
        return t

    def zeros(self, shape, dtype=F32):
        """Zero-filled scratch.  NOT replay-safe inside a recorded step (the fill is a torch op):
        ops that need zeros on every step must clear through a recorded kernel."""
        t = torch.zeros(shape, dtype=dtype, device=self.device)
        if self.keepalive is not None:
            self.keepalive.append(t)
        return t

    def const_vec(self, n, value):
        """A cached constant f32 vector (filled once, outside any recorded step)."""
        t = self._const_vecs.get((n, value))
        if t is None:
            t = self._const_vecs[(n, value)] = torch.full((n,), float(value), dtype=F32, device=self.device)
        return t

    def ensure_materialised(self):
        self.store.materialise()

    def packed(self, var, kind, fn):
        """f16 re-pack of a variable, refreshed when the optimiser has stepped."""
        ent = var.packed.get(kind)
        if ent is None or ent[0] != self.store.version:
            t = fn(ent[1] if ent is not None else None)
            var.packed[kind] = (self.store.version, t)
            return t
        return ent[1]

    def repack_all(self):
        """Refresh every [tap][cout][cin] / [tap][cin][cout] operand pack — and the fuse heads' zero-padded [32][cin] /
        [cin][32] pairs — in ONE launch (after the optimiser step; the packs' own lazy refresh in `packed` then finds
        them current).  Other pack kinds stay lazy."""
        from . import ops
        ents = []
        for v in self.store.vars.values():
            pk = getattr(v, "packed", {})
            if "kc_ck" in pk:
                ents.append((v, "kc_ck", pk["kc_ck"], 0))
            if "small" in pk:
                ents.append((v, "small", pk["small"], 32))
        if not ents:
            return
        key = tuple(id(e[2][1]) for e in ents)
        pb = getattr(self, "_pack_batch", None)
        if pb is None or pb[0] != key:
            pb = (key, ops.PackBatch([(v.data, e[1][0], e[1][1], ld) for v, _, e, ld in ents], self.device))
            self._pack_batch = pb
        pb[1].run()
        for v, kind, e, _ in ents:
            v.packed[kind] = (self.store.version, e[1])

    def stale_lazy_packs(self):
        """Mark the pack kinds that `repack_all` leaves lazy as out of date (their buffers stay): the next forward and
        backward refresh them again.  A step recorded with gradient accumulation needs it: the call in front of the
        recorded one ran at the same store version and left them current, and a plan recorded without their refresh
        would replay stale weights for ever (train.TrainStep._eager)."""
        for v in self.store.vars.values():
            pk = getattr(v, "packed", None)
            for kind in list(pk or ()):
                if kind not in ("kc_ck", "small"):
                    pk[kind] = (None, pk[kind][1])

    # --- tape ---
    def record(self, fn, produces=()):
        """`produces`: the variables whose gradients are complete once `fn` has run."""
        self.tape.append((fn, tuple(produces)))

    def backward(self, on_grads_ready=None):
        """Run the tape in reverse (the loss op seeds its own gradient).  `on_grads_ready(vars)` is
        called as soon as a closure has finished a set of parameter gradients — the hook the
        data-parallel all-reduce uses to overlap communication with the rest of backward."""
        if self.precision != "f16":
            raise NotImplementedError("the %s inference precision is forward-only" % self.precision_name)
        for fn, produces in reversed(self.tape):
            fn()
            if on_grads_ready is not None and produces:
                on_grads_ready(produces)      # while a step is recorded the hook records itself (dist.py)
        self.tape.clear()

    def reset_tape(self):
        self.tape.clear()
        self.collections["losses"].clear()


_default = None


def get_default_graph():
    global _default
    if _default is None:
        _default = Graph()
    return _default


def set_default_graph(g):
    global _default
    _default = g
    return g


# --- initialisers (slim defaults) -------------------------------------------------------
def xavier_uniform(rng):
    def init(shape):
        if len(shape) == 4:
            fan_in, fan_out = shape[0] * shape[1] * shape[2], shape[0] * shape[1] * shape[3]
        else:
            fan_in, fan_out = shape[0], shape[-1]
        lim = math.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, size=shape)
    return init


def variance_scaling(rng, factor=2.0):
    """slim.variance_scaling_initializer(): truncated normal, FAN_IN, factor 2."""
    def init(shape):
        fan_in = shape[0] * shape[1] * shape[2] if len(shape) == 4 else shape[0]
        std = math.sqrt(1.3 * factor / fan_in)
        x = rng.normal(0.0, std, size=shape)
        bad = np.abs(x) > 2 * std
        while bad.any():
            x[bad] = rng.normal(0.0, std, size=int(bad.sum()))
            bad = np.abs(x) > 2 * std
        return x
    return init


def constant(value):
    return lambda shape: np.full(shape, value, dtype=np.float32)
