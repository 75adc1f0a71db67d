"""Host: the input-gradient route selector (layers.select_input_grad), the gradient buffer (Act.open_grad) and the handshake
records of graph.py.  No library, no device: the activations are real `Act`s around a shape, the kernel names come from a
fake `variant`, and nothing is launched."""
import pytest

from tensorflow_ocr_amd import layers, ops
from tensorflow_ocr_amd.graph import Act, BnCtx, Partial, TailCtx
from tensorflow_ocr_amd.layers import PwxOperand, select_input_grad

PERSIST, W4, OTHER = "conv_c64_persist_kernel<64>", "conv3x3_w4_kernel", "conv_igemm_kernel<128,32,2,1,1>"
SHAPE = (2, 8, 8, 64)


class _Data:
    def __init__(self, shape):
        self.shape = shape


def _act(**slots):
    a = Act(_Data(SHAPE))
    for k, v in slots.items():
        setattr(a, k, v)
    return a


def _lazy(moments=True, stored=False):
    y = ops.LazyFirstY(None, "x4", "w_first", SHAPE)
    y.moments = "moments" if moments else None
    y.t = "y" if stored else None
    return y


def _bn(y="y"):
    return BnCtx(y, "scale", "shift", "mean", "invstd", True)


TAIL = TailCtx("y3", "mean", "invstd", "out")
PWX = PwxOperand("dz", "y_above", ("A", "B", "C"), None)
PWX_RELU = PWX._replace(relu_shift="shift")
# the named parameters each caller passes (layers._conv_backward, conv_bn_raw.backward_from unfused / fused, _cat_backward)
CONV2D = dict(conv2d_routes=True)
UNFUSED = dict(tail=True, tail_1x1_only=True)
FUSED = dict(tail=True, bnred_unpended_only=True)
CAT = dict(plain_only=True)

# (what the row shows, Act slots, kernel size, variant, fused, last, the caller's parameters, route)
ROWS = [
    ("first contribution to a conv + BN output", dict(bn_ctx=_bn()), 3, OTHER, None, False, CONV2D, "bnred"),
    ("... an accumulating one", dict(bn_ctx=_bn(), grad="dx"), 3, OTHER, None, False, CONV2D, "plain"),
    ("... no producer context", dict(), 3, OTHER, None, False, CONV2D, "plain"),
    ("... the merge convolution never fuses", dict(bn_ctx=_bn()), 1, OTHER, None, False, CAT, "plain"),
    ("bias + ReLU producer, sole consumer", dict(bias_ctx=_bn(), sole_consumer=True), 3, OTHER, None, False, CONV2D, "bias_masked"),
    ("... sole_consumer off", dict(bias_ctx=_bn()), 3, OTHER, None, False, CONV2D, "plain"),
    ("... accumulating", dict(bias_ctx=_bn(), sole_consumer=True, grad="dx"), 3, OTHER, None, False, CONV2D, "plain"),
    ("... a caller without the conv2d routes", dict(bias_ctx=_bn(), sole_consumer=True), 3, OTHER, None, False, UNFUSED, "plain"),
    ("lazy conv1_1 y with moments, sole consumer", dict(bn_ctx=_bn(_lazy()), sole_consumer=True), 3, PERSIST, None, False, CONV2D,
     "first_sums"),
    ("... without moments", dict(bn_ctx=_bn(_lazy(moments=False)), sole_consumer=True), 3, PERSIST, None, False, CONV2D, "bnred_first"),
    ("... sole_consumer off", dict(bn_ctx=_bn(_lazy())), 3, PERSIST, None, False, CONV2D, "bnred_first"),
    ("... accumulating", dict(bn_ctx=_bn(_lazy()), sole_consumer=True, grad="dx"), 3, PERSIST, None, False, CONV2D, "plain"),
    ("... the library does not take the shape", dict(bn_ctx=_bn(_lazy()), sole_consumer=True), 3, PERSIST, None, False,
     dict(CONV2D, first_sums=False), "bnred_first"),
    ("... on another kernel", dict(bn_ctx=_bn(_lazy(moments=False))), 3, OTHER, None, False, CONV2D, "bnred"),
    ("... y stored after all", dict(bn_ctx=_bn(_lazy(stored=True)), sole_consumer=True), 3, PERSIST, None, False, CONV2D, "bnred"),
    ("... a caller without the conv2d routes", dict(bn_ctx=_bn(_lazy()), sole_consumer=True), 3, PERSIST, None, False, UNFUSED, "bnred"),
    ("last contribution to a bottleneck output, 1x1", dict(tail_ctx=TAIL), 1, OTHER, None, True, UNFUSED, "tail"),
    ("... 3x3, unfused", dict(tail_ctx=TAIL), 3, OTHER, None, True, UNFUSED, "plain"),
    ("... not the last", dict(tail_ctx=TAIL), 1, OTHER, None, False, UNFUSED, "plain"),
    ("... last without tail_ctx", dict(), 1, OTHER, None, True, UNFUSED, "plain"),
    ("... the caller's FUSE_TAIL off", dict(tail_ctx=TAIL), 1, OTHER, None, True, dict(UNFUSED, tail=False), "plain"),
    ("... a caller that builds no bottlenecks", dict(tail_ctx=TAIL), 1, OTHER, None, True, CONV2D, "plain"),
    ("... accumulating: still the tail", dict(tail_ctx=TAIL, grad="dx"), 1, OTHER, None, True, UNFUSED, "tail"),
    ("fused: last contribution", dict(tail_ctx=TAIL, grad="dx"), 1, OTHER, PWX_RELU, True, FUSED, "pwx_tail"),
    ("fused: the tail asks for no 1x1", dict(tail_ctx=TAIL), 3, OTHER, PWX, True, FUSED, "pwx_tail"),
    ("fused: last without tail_ctx", dict(grad="dx"), 1, OTHER, PWX, True, FUSED, "pwx_plain"),
    ("fused: first contribution to a conv + BN output", dict(bn_ctx=_bn()), 1, OTHER, PWX, False, FUSED, "pwx_bnred"),
    ("... relu_shift set", dict(bn_ctx=_bn()), 1, OTHER, PWX_RELU, False, FUSED, "pwx_plain"),
    ("... pending set", dict(bn_ctx=_bn(), pending=1), 1, OTHER, PWX, False, FUSED, "pwx_plain"),
    ("... pending set, unfused caller", dict(bn_ctx=_bn(), pending=1), 1, OTHER, None, False, UNFUSED, "bnred"),
    ("... accumulating", dict(bn_ctx=_bn(), grad="dx"), 1, OTHER, PWX, False, FUSED, "pwx_plain"),
]


def _select(slots, k, variant, fused, last, guards, h=8):
    x = _act(**slots)
    before = {s: getattr(x, s) for s in Act.__slots__}
    d = ops.conv_desc((2, h, 8, 64), 64, k, k)
    route = select_input_grad(x, d, fused=fused, last=last, variant=lambda: variant, **guards)
    assert {s: getattr(x, s) for s in Act.__slots__} == before, "the selector changed the activation"
    return route


@pytest.mark.parametrize("what,slots,k,variant,fused,last,guards,route", ROWS, ids=[r[0] for r in ROWS])
def test_selector_table(what, slots, k, variant, fused, last, guards, route):
    assert _select(slots, k, variant, fused, last, guards) == route


def test_w4_cutoff_is_the_conv2d_callers_alone(monkeypatch):
    bn = dict(bn_ctx=_bn())
    assert _select(bn, 3, W4, None, False, CONV2D) == "bnred"                    # the shipped cut-off is out of reach
    monkeypatch.setattr(layers, "FUSE_BN_W4_MAXHW", 8)
    assert _select(bn, 3, W4, None, False, CONV2D, h=8) == "plain"
    assert _select(bn, 3, W4, None, False, CONV2D, h=7) == "bnred"
    assert _select(bn, 3, OTHER, None, False, CONV2D, h=8) == "bnred"
    assert _select(bn, 3, W4, None, False, UNFUSED, h=8) == "bnred"


# (switch, value, a row's name, the route it falls back to)
SWITCHED = [
    ("FUSE_BN_REDUCE", False, "first contribution to a conv + BN output", "plain"),
    ("FUSE_BN_REDUCE", False, "fused: first contribution to a conv + BN output", "pwx_plain"),
    ("FUSE_BN_REDUCE", False, "lazy conv1_1 y with moments, sole consumer", "plain"),
    ("FUSE_BN_REDUCE", False, "last contribution to a bottleneck output, 1x1", "tail"),
    ("FIRST_WGRAD_SUMS", False, "lazy conv1_1 y with moments, sole consumer", "bnred_first"),
    ("FUSE_BIAS_RELU", False, "bias + ReLU producer, sole consumer", "plain"),
]


@pytest.mark.parametrize("switch,value,row,route", SWITCHED)
def test_switch_off_falls_back(monkeypatch, switch, value, row, route):
    _, slots, k, variant, fused, last, guards, _ = next(r for r in ROWS if r[0] == row)
    assert getattr(layers, switch) != value
    monkeypatch.setattr(layers, switch, value)
    assert _select(slots, k, variant, fused, last, guards) == route


# ------------------------------------------------------------------------------------------------ the gradient buffer
class _G:
    def __init__(self):
        self.made = []

    def empty(self, shape):
        self.made.append(shape)
        return "buffer %d" % len(self.made)


def test_open_grad_allocates_once_and_an_accumulating_call_drops_the_first_sums():
    g = _G()
    x = _act(tail_partial=Partial("t", 1), first_s1="s1", pending=2)
    assert x.open_grad(g) == ("buffer 1", False) and g.made == [SHAPE] and x.grad == "buffer 1"
    x.bn_partial, x.bias_partial = Partial("rows", 3), Partial("bias rows", 3)
    assert x.open_grad(g) == ("buffer 1", True) and g.made == [SHAPE]
    assert x.bn_partial is None and x.bias_partial is None
    assert (x.tail_partial, x.first_s1, x.pending) == (Partial("t", 1), "s1", 2)


def test_count_contribution_counts_the_owners_alone():
    owner = object()
    x = _act(pending=2, pending_owner=owner)
    assert not x.count_contribution(None) and not x.count_contribution(object()) and x.pending == 2
    assert not x.count_contribution(owner) and x.pending == 1
    assert x.count_contribution(owner) and x.pending == 0
    assert not _act().count_contribution(owner)


# ------------------------------------------------------------------------------------------------ the records
def test_records_stay_tuples():
    assert TailCtx("y", "mean", "invstd", "out").bits is None
    assert TailCtx(*("y", "mean", "invstd", "out", "bits")).bits == "bits"      # what ops does with a caller's plain tuple
    plain = ("y", "scale", "shift", "mean", "invstd", True)
    assert BnCtx(*plain) == plain and BnCtx(*plain).invstd == "invstd" and BnCtx(*plain)[0] == "y"
    lazy = _lazy()
    assert BnCtx(lazy, "scale", "shift", "mean", "invstd", True).first() == ("x4", "w_first", "scale", "shift", "mean", "invstd", True)


def test_of_bias_is_the_identity_batch_norm():
    class G:
        def const_vec(self, n, value):
            return (n, value)
    assert BnCtx.of_bias(G(), "a", 64) == ("a", (64, 1.0), (64, 0.0), (64, 0.0), (64, 1.0), True)


# ------------------------------------------------------------------------------------------------ the executor
LAUNCHES = ["conv2d", "conv2d_bnred", "conv2d_bnred_first", "conv2d_bnred_first_wgrad", "conv2d_bnred_tail",
            "conv2d_pw_bnbwd_bnred", "conv2d_pw_bnbwd_tail"]


@pytest.fixture
def launches(monkeypatch):
    """-> log of (wrapper, arguments after the descriptor, keywords, the descriptor's flags) with every ops entry faked."""
    log = []
    for name in LAUNCHES:
        monkeypatch.setattr(ops, name, lambda d, *a, _n=name, **kw: log.append((_n, a, kw, d.flags)))
    monkeypatch.setattr(ops, "conv2d_variant", lambda d: PERSIST)
    monkeypatch.setattr(ops, "conv2d_num_mtiles", lambda d: 5)
    monkeypatch.setattr(ops, "conv2d_bnred_first_wgrad_blocks", lambda d: 7)
    return log


class _GE(_G):
    def empty(self, shape, dtype=None):
        return "%s %s" % (super().empty(shape), shape)


GRAD, ROWS5 = "buffer 1 %s" % (SHAPE,), "buffer 2 (5, 2, 64)"


def _run(slots, k, guards, fused=None, owner=None):
    x = _act(**slots)
    layers.input_grad(_GE(), x, ops.conv_desc((2, 8, 8, 64), 64, k, k), "w_dg", "dy", owner=owner, fused=fused, **guards)
    return x


def test_executor_plain_first_and_accumulating(launches):
    x = _run({}, 3, CONV2D)
    assert launches == [("conv2d", ("dy", "w_dg", GRAD, None, None), {}, 0)] and x.grad == GRAD
    del launches[:]
    x = _run(dict(grad="dx", bn_ctx=_bn(), bn_partial=Partial("stale", 1)), 1, CAT)
    assert launches == [("conv2d", ("dy", "w_dg", "dx", None, None), {}, ops.CONV_ACCUM_F16)] and x.bn_partial is None


def test_executor_bnred_and_bias_masked(launches):
    x = _run(dict(bn_ctx=_bn()), 3, UNFUSED)
    assert launches == [("conv2d_bnred", ("dy", "w_dg", GRAD, ROWS5, _bn()), {"store_masked": False}, 0)]
    assert x.bn_partial == (ROWS5, 5) and x.bias_partial is None
    del launches[:]
    x = _run(dict(bias_ctx=_bn("a"), sole_consumer=True), 3, CONV2D)
    assert launches == [("conv2d_bnred", ("dy", "w_dg", GRAD, ROWS5, _bn("a")), {"store_masked": True}, 0)]
    assert x.bias_partial == (ROWS5, 5) and x.bn_partial is None


def test_executor_first_layer_routes(launches, monkeypatch):
    first = ("x4", "w_first", "scale", "shift", "mean", "invstd", True)
    x = _run(dict(bn_ctx=_bn(_lazy()), sole_consumer=True), 3, CONV2D)
    rows, s1 = "buffer 1 (5, 2, 64)", "buffer 2 (7, 32, 64)"
    assert launches == [("conv2d_bnred_first_wgrad", ("dy", "w_dg", rows, first, s1), {}, 0)]
    assert x.grad is None and x.bn_partial == (rows, 5) and x.first_s1 == s1
    del launches[:]
    monkeypatch.setattr(ops, "conv2d_bnred_first_wgrad_blocks", lambda d: -1)       # the library does not take the shape
    x = _run(dict(bn_ctx=_bn(_lazy()), sole_consumer=True), 3, CONV2D)
    assert launches == [("conv2d_bnred_first", ("dy", "w_dg", GRAD, ROWS5, first), {}, 0)]
    assert x.grad == GRAD and x.bn_partial == (ROWS5, 5) and x.first_s1 is None


def test_executor_tail_and_the_pwx_loader(launches):
    owner = object()
    counted = dict(tail_ctx=TAIL, pending=1, pending_owner=owner, sub_grad="sub", grad="dx")
    x = _run(counted, 1, UNFUSED, owner=owner)
    rows = "buffer 1 (5, 2, 64)"
    assert launches == [("conv2d_bnred_tail", ("dy", "w_dg", "dx", rows, TAIL, "sub"), {}, ops.CONV_ACCUM_F16)]
    assert x.tail_partial == (rows, 5) and x.sub_grad is None and x.pending == 0
    del launches[:]
    x = _run(counted, 1, FUSED, fused=PWX_RELU, owner=owner)
    assert launches == [("conv2d_pw_bnbwd_tail", ("dz", "y_above", ("A", "B", "C"), "shift", "dy", "w_dg", "dx", rows, TAIL, "sub"),
                         {}, ops.CONV_ACCUM_F16)]
    assert x.tail_partial == (rows, 5) and x.sub_grad is None
    del launches[:]
    x = _run(dict(counted, pending=2), 1, FUSED, fused=PWX_RELU, owner=owner)          # not the last: plain epilogue
    assert launches == [("conv2d_pw_bnbwd_tail", ("dz", "y_above", ("A", "B", "C"), "shift", "dy", "w_dg", "dx", None, None, None),
                         {}, ops.CONV_ACCUM_F16)]
    assert x.tail_partial is None and x.sub_grad == "sub" and x.pending == 1
    del launches[:]
    x = _run(dict(bn_ctx=_bn()), 1, FUSED, fused=PWX)
    assert launches == [("conv2d_pw_bnbwd_bnred", ("dz", "y_above", ("A", "B", "C"), "dy", "w_dg", GRAD, ROWS5, _bn()), {}, 0)]
    assert x.bn_partial == (ROWS5, 5)
