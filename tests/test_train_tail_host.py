"""CPU: what the training tail launches, call for call, against tests/golden/train_tail_trace.json — recorded by
tests/golden/make_train_tail_trace.py from THIS file on the commit from before the loss seeds, the optimiser ladders and
the two optimiser classes were pulled together.  Every `ops` entry the tail reaches is replaced by a recorder on CPU
tensors: the five loss families' forward and backward entries, the scaler's init and check, the clip passes and the six
step entries.  The recorder keeps every call in order — its name, scalars by value, descriptors by their fields, tensors as
(shape, dtype) and, where a tensor lies in the loss scaler's or the clip's state block, that block's name and the word it
starts at."""
import contextlib
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_tail_trace.json")

LOSS_ENTRIES = [fam + suffix for fam in ("softmax_loss", "balanced_loss", "dice_loss", "rbox_loss", "link_ce")
                for suffix in ("_fwd", "_bwd", "_bwd_dyn")]
STEP_ENTRIES = ["loss_scale_init", "grad_check", "grad_clip", "grad_check_clip", "adam_step", "adam_step_dyn", "adam_step_clip",
                "momentum_step", "momentum_step_dyn", "momentum_step_clip"]
FAMILIES = ("softmax", "balanced", "dice", "rbox", "link_ce")
SCALES = ("const", "dynamic")
MODES = ("static", "dynamic", "clip_static", "clip_dynamic")
OPTS = ("adam", "momentum")


class Recorder:
    """`blocks()` names the state blocks of the case at hand: [(name, tensor or None)]."""

    def __init__(self, blocks=lambda: ()):
        self.log, self.blocks = [], blocks

    def desc(self, a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, (np.integer, np.floating)):
            return a.item()
        if isinstance(a, torch.Tensor):
            d = [list(a.shape), str(a.dtype).replace("torch.", "")]
            for name, block in self.blocks():
                if block is not None and a.untyped_storage().data_ptr() == block.untyped_storage().data_ptr():
                    d += [name, a.storage_offset() * a.element_size() // 4]
            return d
        if isinstance(a, ctypes.Structure):
            return [type(a).__name__] + [getattr(a, f[0]) for f in a._fields_]
        return type(a).__name__

    def stub(self, name):
        def f(*args):
            self.log.append([name] + [self.desc(a) for a in args])
        return f

    @contextlib.contextmanager
    def installed(self):
        from tensorflow_ocr_amd import ops
        names = LOSS_ENTRIES + STEP_ENTRIES
        saved = [(n, getattr(ops, n)) for n in names]
        for n in names:
            setattr(ops, n, self.stub(n))
        try:
            yield self
        finally:
            for n, orig in saved:
                setattr(ops, n, orig)


def _scale(which):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    return DynamicLossScale() if which == "dynamic" else 1024.0


def _graph(scale, variables=True):
    from tensorflow_ocr_amd import graph as G
    g = G.Graph("cpu", loss_scale=_scale(scale), seed=2)
    g.ws = g.ws_small = g.ws_wgrad = "Workspace"            # the stubs take it and never look inside
    if variables:
        with g.variable_scope("feature_fusion"):
            g.get_variable("Conv/weights", (1, 1, 4, 2), G.xavier_uniform(g.rng), regularized=True)
            g.get_variable("Conv/biases", (8,), G.constant(0.5))
    return g


def _blocks(g, opt=None):
    def blocks():
        sc = g.loss_scaler
        return (("loss_scale_state", sc._state if sc is not None else None),
                ("clip_state", opt.clip.state if opt is not None and opt.clip is not None else None))
    return blocks


def _head(*shape):
    return types.SimpleNamespace(data=torch.zeros(shape), grad=None)


def run_loss_seed(family, scale, loss_div):
    """the backward closure of one loss family at n = 1, h = w = 2 -> its calls (the forward's included)"""
    from tensorflow_ocr_amd import losses
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    g = _graph(scale, variables=False)
    g.loss_div = float(loss_div)
    z = lambda *s: torch.zeros(s)
    rec = Recorder(_blocks(g))
    with rec.installed():
        if family == "softmax":
            losses.softmax_loss(g, _head(1, 2, 2, 2), _head(1, 2, 2, 16), z(1, 2, 2), z(1, 2, 2, 8), pixel_rule=1, label_rule=0,
                                link_gate=True)
        elif family == "balanced":
            losses.balanced_loss(g, _head(1, 2, 2, 2), _head(1, 2, 2, 16), z(1, 2, 2), z(1, 2, 2, 8), z(1, 2, 2))
        elif family == "dice":
            M.loss(z(1, 2, 2, 1), _head(1, 2, 2, 2), z(1, 2, 2, 8), _head(1, 2, 2, 16), z(1, 2, 2, 1), graph=g)
        elif family == "rbox":
            M.loss_rbox(z(1, 2, 2, 1), _head(1, 2, 2, 1), z(1, 2, 2, 5), _head(1, 2, 2, 5), z(1, 2, 2, 1), graph=g)
        else:
            M.cal_link_loss(z(1, 2, 2, 1), _head(1, 2, 2, 2), z(4), graph=g)
        assert len(g.tape) == 1
        g.tape[0][0]()
    return rec.log


def _optimizer(which, g, mode, ema):
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer
    clip = 2.5 if mode.startswith("clip") else None
    if which == "adam":
        return AdamOptimizer(g, learning_rate=1e-3, moving_average_decay=0.997 if ema else None, clip_norm=clip)
    return MomentumOptimizer(g, base_lr=1e-2, moving_average_decay=0.9999 if ema else None, clip_norm=clip)


def _mode_scale(mode):
    return "dynamic" if mode.endswith("dynamic") else "const"


def run_steps(which, mode, grad_scale, ema):
    """two apply_gradients calls on the 16-element tower -> the calls, and the counters behind each"""
    g = _graph(_mode_scale(mode))
    rec = Recorder(_blocks(g))
    with rec.installed():
        opt = _optimizer(which, g, mode, ema)
        rec.blocks = _blocks(g, opt)
        st = g.store
        assert st.flat.numel() == 16 and st.n_reg == 8
        for _ in range(2):
            opt.apply_gradients(grad_scale)
            rec.log.append(["counters", opt.global_step, st.version])
    return rec.log


def run_summary_factor(mode, k):
    from tensorflow_ocr_amd.train import TrainStep
    g = _graph(_mode_scale(mode))
    rec = Recorder()
    with rec.installed():
        opt = _optimizer("adam", g, mode, True)
        rec.blocks = _blocks(g, opt)
        step = TrainStep(g, None, None, accumulate_steps=k)
        step.opt, step.reducer = opt, types.SimpleNamespace(grad_scale=0.5)
        mul_host, mul_dev = step.summary_factor()
        return {"mul_host": mul_host, "mul_dev": rec.desc(mul_dev), "calls": rec.log}


def run_state_round_trip(which):
    """slots, scalars and shadows of an optimiser at global_step 7, and what a fresh one holds after load_state"""
    def lists(d):
        return {k: lists(v) if isinstance(v, dict) else np.asarray(v).reshape(-1).tolist() for k, v in sorted(d.items())}
    with Recorder().installed():
        a = _optimizer(which, _graph("const"), "static", True)
        a.global_step = 7
        for i, name in enumerate(a.SLOTS + ("ema",)):
            buf = {"Adam": "m", "Adam_1": "v", "Momentum": "acc", "ema": "ema"}[name]
            getattr(a, buf).copy_(torch.arange(16, dtype=torch.float32) + 100 * (i + 1))
        saved = {"slots": lists(a.slot_state_dict()), "scalars": lists(a.scalar_state_dict()), "ema": lists(a.shadow_state_dict())}
        b = _optimizer(which, _graph("const"), "static", True)
        b.load_state(global_step=7, slots=a.slot_state_dict(), ema=a.shadow_state_dict())
        loaded = {"slots": lists(b.slot_state_dict()), "scalars": lists(b.scalar_state_dict()), "ema": lists(b.shadow_state_dict())}
        return {"SLOTS": list(a.SLOTS), "saved": saved, "loaded": loaded, "global_step": b.global_step,
                "learning_rate": b.learning_rate()}


def seed_name(family, scale, loss_div):
    return "%s %s div%d" % (family, scale, loss_div)


def step_name(which, mode, grad_scale, ema):
    return "%s %s gs%g %s" % (which, mode, grad_scale, "ema" if ema else "noema")


def factor_name(mode, k):
    return "%s K%d" % (mode, k)


SEED_CASES = [(f, s, d) for f in FAMILIES for s in SCALES for d in (1, 2)]
STEP_CASES = [(w, m, gs, e) for w in OPTS for m in MODES for gs in (1.0, 0.25) for e in (True, False)]
FACTOR_CASES = [(m, k) for m in MODES for k in (1, 4)]


def record_all():
    return json.loads(json.dumps({
        "seeds": {seed_name(*c): run_loss_seed(*c) for c in SEED_CASES},
        "steps": {step_name(*c): run_steps(*c) for c in STEP_CASES},
        "summary_factor": {factor_name(*c): run_summary_factor(*c) for c in FACTOR_CASES},
        "state": {w: run_state_round_trip(w) for w in OPTS}}))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["tail"]


def _same_calls(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)                            # the first call that moved, by name
    assert len(got) == len(want)


def test_golden_holds_every_case(golden):
    with open(GOLDEN) as f:
        assert len(json.load(f)["parent"]) == 40
    assert sorted(golden["seeds"]) == sorted(seed_name(*c) for c in SEED_CASES)
    assert sorted(golden["steps"]) == sorted(step_name(*c) for c in STEP_CASES)
    assert sorted(golden["summary_factor"]) == sorted(factor_name(*c) for c in FACTOR_CASES)
    assert sorted(golden["state"]) == sorted(OPTS)
    # the cases are what they are named for: a dynamic seed reads the scale word, a clip step the clip block
    for name, calls in golden["seeds"].items():
        assert [c[0] for c in calls if c[0].endswith("_dyn")] == ([calls[-1][0]] if " dynamic " in name else []), name
    for name, calls in golden["steps"].items():
        steps = [c[0] for c in calls if "_step" in c[0]]
        assert len(steps) == 2 and [c[1:] for c in calls if c[0] == "counters"] == [[1, 1], [2, 2]], name
        assert steps[0].endswith("_clip") == (" clip_" in name), name


@pytest.mark.parametrize("family,scale,loss_div", SEED_CASES)
def test_loss_seed_launches_what_the_parent_launched(golden, family, scale, loss_div):
    _same_calls(json.loads(json.dumps(run_loss_seed(family, scale, loss_div))), golden["seeds"][seed_name(family, scale, loss_div)])


@pytest.mark.parametrize("which,mode,grad_scale,ema", STEP_CASES)
def test_two_optimiser_steps_launch_what_the_parent_launched(golden, which, mode, grad_scale, ema):
    _same_calls(json.loads(json.dumps(run_steps(which, mode, grad_scale, ema))), golden["steps"][step_name(which, mode, grad_scale, ema)])


@pytest.mark.parametrize("mode,k", FACTOR_CASES)
def test_summary_factor_is_the_parents(golden, mode, k):
    assert json.loads(json.dumps(run_summary_factor(mode, k))) == golden["summary_factor"][factor_name(mode, k)]


@pytest.mark.parametrize("which", OPTS)
def test_state_round_trip_is_the_parents(golden, which):
    got = json.loads(json.dumps(run_state_round_trip(which)))
    assert got == golden["state"][which]
    assert got["saved"] == got["loaded"] and got["global_step"] == 7
