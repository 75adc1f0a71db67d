"""The fuse heads: the small f32 tensors behind the last quarter of every net's step.

The merged 1x1 fuse convolutions on the trunk's end points (`head_group`; per source `head_conv_bn` / `head_conv_bias`),
the adds and upsamples between them (`fuse`), the two predication convolutions on the fused 18-channel tensor
(`pointwise_pair`; per head `pointwise_bn` / `pointwise_bias`) and the sigmoid / RBOX heads on EAST's merge branch
(`sigmoid_heads`, `rbox_heads`).  As in layers.py each function runs its forward kernels immediately and records one
backward closure on the graph's tape; the variables keep slim's names, merged ones as `<a>+<b>/weights`
(checkpoint.internal_to_tf splits them back).
"""
import numpy as np
import torch

from . import layers_f32, ops
from .graph import F32, constant, variance_scaling, xavier_uniform
from .layers import BN_DECAY, BN_EPS, _bn_buffers, _bn_params, _bn_vars, _switch

BATCH_HEADS = _switch("OCR_BATCH_HEADS")    # one launch per kernel kind over the head sources
MERGE_HEADS = _switch("OCR_RESNET_MERGE_HEADS")   # F_score + geo_map: one pass over the feature


class SmallAct:
    """f32 [n,h,w,C] head tensor."""
    __slots__ = ("data", "grad")

    def __init__(self, data):
        self.data = data
        self.grad = None


class HeadSource:
    """One source of a batched head launch: a feature map with its merged fuse convolution (head_group), or one of the
    two predication heads on the fused tensor (pointwise_pair: no feature, no operand packs).  gamma .. mv and scale ..
    invstd exist under batch norm only, `bias` without it; part / T only while training batch norm; dz only inside the
    backward."""
    __slots__ = ("feat", "cin", "w_kc32", "w_ck32", "P", "C", "wv", "gamma", "beta", "mm", "mv", "bias", "z", "out",
                 "scale", "shift", "mean", "invstd", "part", "T", "dz")

    def __init__(self, P, C, wv, bn_vars, bias, z, feat=None, cin=None, packs=(None, None)):
        self.feat, self.cin = feat, cin
        self.w_kc32, self.w_ck32 = packs
        self.P, self.C, self.wv, self.bias, self.z = P, C, wv, bias, z
        self.gamma, self.beta, self.mm, self.mv = bn_vars or (None,) * 4
        self.out = SmallAct(z)      # grad of out = gradient w.r.t. relu(bn(z)) (bn) / z (bias)
        self.scale = self.shift = self.mean = self.invstd = None
        self.part = self.T = self.dz = None


def _data(v):
    return v.data if v is not None else None


def _grad(v):
    return v.grad if v is not None else None


def _merged_init(g, cin, couts, base=None):
    base = base or variance_scaling

    def init(shape):
        cols = [base(g.rng)((1, 1, cin, c)).reshape(cin, c) for c in couts]
        return np.concatenate(cols, axis=1)
    return init


def _head_vars(g, names, cin, couts, mode, initializer=None):
    """One merged parameter per head source, its columns mapping onto the reference variables `names`
    -> (weights [cin, sum(couts)], BN variables | None, biases | None)."""
    C = sum(couts)
    with g.variable_scope("+".join(names)):
        init = _merged_init(g, cin, couts, None if mode == "bn" else (initializer or xavier_uniform))
        wv = g.get_variable("weights", (cin, C), init, regularized=True)
        if mode == "bn":
            return wv, _bn_vars(g, C), None
        return wv, None, g.get_variable("biases", (C,), constant(0.0))


def _small_packs(g, wv, cin):
    """f16 operand layouts of a merged head weight, padded to 32 columns: forward [32][cin] and dgrad [cin][32]."""
    def mk(old):
        if old is None:
            old = (g.empty((32, cin)), g.empty((cin, 32)))
        ops.pack_weights_small(wv.data, old[0], old[1])
        return old
    return g.packed(wv, "small", mk)


def _small_stats(g, z, C):
    """Batch statistics of an f32 head tensor [..., C]: the `stats` of _bn_params."""
    P = z.numel() // C
    T = ops.sc_num_partials(P, C)
    part, stage = g.ws_small.two(T * 2 * C * 4, ops.bn_reduce_workspace(T, C))
    ops.sc_stats(z, C, part)
    return part, T, float(P), stage


def _pointwise_vars(g, scope, c, mode, initializer=None):
    """One predication convolution's (weights [1,1,c,c], BN variables | None, biases | None)."""
    with g.variable_scope(scope):
        init = variance_scaling(g.rng) if mode == "bn" else (initializer or xavier_uniform)(g.rng)
        wv = g.get_variable("weights", (1, 1, c, c), init, regularized=True)
        if mode == "bn":
            return wv, _bn_vars(g, c), None
        return wv, None, g.get_variable("biases", (c,), constant(0.0))


# ---------------------------------------------------------------------------- what the batched forms share
def _bn_alloc(g, s, T):
    """The batch-norm buffers of source `s`; T: the partial rows its forward kernel leaves while training, else None."""
    s.scale, s.shift, s.mean, s.invstd = _bn_buffers(g, s.C)
    if T is not None:
        s.T, s.part = T, g.empty((T, 2, s.C), F32)


def _bn_fill(srcs, is_training):
    """scale / shift / mean / invstd of every source: from the partial rows in ONE launch while training (moves the
    moving statistics too), scale / shift from the moving statistics otherwise."""
    if is_training:
        ops.bn_finalize_batch([(s.part, s.T, s.C, float(s.P), s.gamma.data, s.beta.data, s.mm.data, s.mv.data,
                                s.scale, s.shift, s.mean, s.invstd) for s in srcs], BN_EPS, BN_DECAY)
        return
    for s in srcs:
        ops.bn_inference_params(s.gamma.data, s.beta.data, s.mm.data, s.mv.data, BN_EPS, s.scale, s.shift)


def _bn_bwd_batch(g, srcs, relu, is_training):
    """s.dz of every source from the gradient of relu(bn(z)) in s.out.grad, dgamma / dbeta with it: ONE launch."""
    if not is_training:
        raise NotImplementedError("backward through inference-mode batch norm")
    items = []
    for s in srcs:
        s.dz = g.empty(s.z.shape, F32)
        T = ops.sc_num_partials(s.P, s.C)
        items.append((s.z, s.scale, s.shift, s.mean, s.invstd, s.out.grad, s.gamma.grad, s.beta.grad, s.dz,
                      g.empty((T, 2, s.C), F32), relu))
    ops.sc_bn_bwd_batch(items)


def _produces(srcs):
    """The variables whose gradients the sources' backward completes."""
    out = []
    for s in srcs:
        out += [s.wv] + ([s.bias] if s.bias is not None else [s.gamma, s.beta])
    return out


# ---------------------------------------------------------------------------- fuse convolutions
def _head_conv(g, feat, names, couts, mode, is_training=True, relu=True, initializer=None):
    """One source's merged fuse convolution, a launch per kernel: head_conv_bn (mode "bn") / head_conv_bias ("bias")."""
    n, h, w, cin = feat.shape
    C = sum(couts)
    ws = g.workspace()
    wv, bn_vars, bias = _head_vars(g, names, cin, couts, mode, initializer)
    w_kc32, w_ck32 = _small_packs(g, wv, cin)
    z = g.empty((n, h, w, C), F32)
    if g.precision == "f32":
        layers_f32.head_conv(g, feat, wv, C, z, bias)
    else:
        ops.conv1x1_small(feat.data, w_kc32, C, z, _data(bias))
    scale = shift = None
    if mode == "bn":
        gamma, beta = bn_vars[:2]
        scale, shift, mean, invstd = _bn_params(g, C, bn_vars, _small_stats(g, z, C) if is_training else None)
    out = SmallAct(z)   # grad of out = gradient w.r.t. relu(bn(z)) (bn) / z (bias)

    def backward():
        if out.grad is None:
            return
        if mode == "bn":
            dz = g.empty(z.shape, F32)
            ops.sc_bn_bwd(z, scale, shift, mean, invstd, out.grad, relu, gamma.grad, beta.grad, dz, ws)
        else:
            dz = out.grad
            ops.sc_colsum(dz, C, bias.grad, ws)
        ops.conv1x1_small_wgrad(feat.data, dz, C, wv.grad, ws)
        if feat.requires_grad:
            ops.conv1x1_small_dgrad(dz, w_ck32, C, *feat.open_grad(g))
        out.grad = None
    g.record(backward, (wv, gamma, beta) if mode == "bn" else (wv, bias))
    return out, scale, shift


def head_conv_bn(g, feat, names, couts, is_training=True, relu=True):
    """The BN'd 1x1 fuse convs that several heads apply to ONE feature map, evaluated in a single
    pass over the feature: slim.conv2d(feat, c, 1) for c in couts (nets/model_vgg_16.py:160-172).
    Returns (z, scale, shift): z = SmallAct of the raw conv output [n,h,w,sum(couts)] f32."""
    return _head_conv(g, feat, names, couts, "bn", is_training, relu)


def head_conv_bias(g, feat, names, couts, initializer=None):
    """PixelLinkNet's fuse convs on one feature map — slim.conv2d(feat, c, [1,1], activation_fn=None)
    with biases, no normaliser (nets/pixellink.py:58-67) — merged into one pass over the feature.
    Returns (z, None, None) in the triple form `fuse` consumes."""
    return _head_conv(g, feat, names, couts, "bias", initializer=initializer)


def head_group(g, feats, names_list, couts, *, mode="bn", is_training=True, relu=True, initializer=None):
    """The fuse convs of ALL head sources (nets/model_vgg_16.py:160-172: fc7, conv5_3, conv4_3, conv3_3; nets/pixellink.py:
    58-67; nets/model.py:129-141) with one launch per kernel kind over the sources instead of one per source: per feature map
    the same merged 1x1 convolution (+ batch-norm statistics | + biases) as head_conv_bn / head_conv_bias, same variables in
    the same order.  Returns the list of (z SmallAct, scale, shift) triples `fuse` consumes (scale = shift = None for
    mode="bias").  OCR_BATCH_HEADS=0 (or the f32 verification precision) runs the per-source forms."""
    if not BATCH_HEADS or g.precision == "f32" or len(feats) > 4:
        return [_head_conv(g, f, nm, couts, mode, is_training, relu, initializer) for f, nm in zip(feats, names_list)]
    C = sum(couts)
    ws = g.workspace()
    srcs = []
    for feat, names in zip(feats, names_list):
        n, h, w, cin = feat.shape
        wv, bn_vars, bias = _head_vars(g, names, cin, couts, mode, initializer)
        packs = _small_packs(g, wv, cin)
        s = HeadSource(n * h * w, C, wv, bn_vars, bias, g.empty((n, h, w, C), F32), feat, cin, packs)
        if mode == "bn":
            _bn_alloc(g, s, ops.conv1x1_small_batch_rows(s.P) if is_training else None)
        srcs.append(s)
    ops.conv1x1_small_batch([(s.feat.data, s.w_kc32, _data(s.bias), s.z, s.part) for s in srcs])
    if mode == "bn":
        _bn_fill(srcs, is_training)

    def backward():
        live = [s for s in srcs if s.out.grad is not None]
        if not live:
            return
        if mode == "bn":
            _bn_bwd_batch(g, live, relu, is_training)
        else:
            items = []
            for s in live:
                s.dz = s.out.grad
                T = ops.sc_num_partials(s.P, C)
                items.append((s.dz, s.bias.grad, g.empty((T + 1, 2, C), F32)))
            ops.sc_colsum_batch(items)
        # the batched MFMA kernel: 128-channel blocks, 32-bit buffer offsets (heads.hip: P * cin * 2 and P * C * 4 below
        # 2 GiB); anything else — a 256-channel map beyond 4.19 M pixels, say — keeps the per-map kernel, which has no limit
        def is_wide(s):
            return s.cin % 128 == 0 and s.P * s.cin * 2 < (1 << 31) and s.P * C * 4 < (1 << 31)
        wide = [s for s in live if is_wide(s)]
        if wide:
            ops.conv1x1_small_wgrad_batch([
                (s.feat.data, s.dz, s.wv.grad,
                 g.empty((ops.conv1x1_small_wgrad_batch_slab_bytes(s.P, s.cin),), torch.uint8)) for s in wide])
        for s in live:
            if not is_wide(s):
                ops.conv1x1_small_wgrad(s.feat.data, s.dz, C, s.wv.grad, ws)
        items = [(s.dz, s.w_ck32) + s.feat.open_grad(g) for s in live if s.feat.requires_grad]
        if items:
            ops.conv1x1_small_dgrad_batch(items)
        for s in live:
            s.out.grad = s.dz = None
    g.record(backward, _produces(srcs))
    return [(s.out, s.scale, s.shift) for s in srcs]


def fuse(g, shape, a=None, b=None, prev=None, relu=True):
    """out = relu(bn(a.z)) + relu(bn(b.z)) + unpool(prev)   (any subset) on f32 head tensors.
    a, b: (SmallAct z, scale, shift) triples from head_conv_bn; prev: SmallAct at half resolution."""
    out = SmallAct(g.empty(shape, F32))
    za, sa, ha = (a[0].data, a[1], a[2]) if a is not None else (None, None, None)
    zb, sb, hb = (b[0].data, b[1], b[2]) if b is not None else (None, None, None)
    ops.sc_fuse(out.data, za, sa, ha, zb, sb, hb, prev.data if prev is not None else None, relu)

    def backward():
        if out.grad is None:
            return
        # the add fans the same gradient out to every branch; the BN/ReLU part of a and b is
        # differentiated inside head_conv_bn's closure
        for br in (a, b):
            if br is not None:
                if br[0].grad is not None:
                    raise RuntimeError("head tensor used twice")
                br[0].grad = out.grad
        if prev is not None:
            dprev = g.empty(prev.data.shape, F32)
            ops.sc_unpool_bwd(out.grad, dprev)
            prev.grad = dprev
        out.grad = None
    g.record(backward)
    return out


# ---------------------------------------------------------------------------- predication convolutions
def _pointwise(g, x, xo, c, scope, mode, is_training=True, relu=True, initializer=None):
    """One predication convolution on the channel slice [xo, xo + c) of a head tensor, a launch per kernel:
    pointwise_bn (mode "bn") / pointwise_bias ("bias")."""
    n, h, w, C = x.data.shape
    ws = g.workspace()
    wv, bn_vars, bias = _pointwise_vars(g, scope, c, mode, initializer)
    z = g.empty((n, h, w, c), F32)
    ops.sc_pointwise_fwd(x.data, xo, c, wv.data, z, 0, c, _data(bias))
    if mode == "bn":
        gamma, beta = bn_vars[:2]
        scale, shift, mean, invstd = _bn_params(g, c, bn_vars, _small_stats(g, z, c) if is_training else None)
        out = SmallAct(g.empty((n, h, w, c), F32))
        ops.sc_fuse(out.data, z, scale, shift, relu=relu)
    else:
        out = SmallAct(z)

    def backward():
        if out.grad is None:
            return
        if mode == "bn":
            dz = g.empty(z.shape, F32)
            ops.sc_bn_bwd(z, scale, shift, mean, invstd, out.grad, relu, gamma.grad, beta.grad, dz, ws)
        else:
            dz = out.grad
        ops.sc_pointwise_wgrad(x.data, xo, c, dz, 0, c, wv.grad, _grad(bias), ws)
        if x.grad is None:
            x.grad = g.empty(x.data.shape, F32)
            ops.fill_(x.grad, 0.0)
        ops.sc_pointwise_dgrad(dz, 0, c, wv.data, x.grad, xo, c)
        out.grad = None
    g.record(backward, (wv, gamma, beta) if mode == "bn" else (wv, bias))
    return out


def pointwise_bn(g, x, xo, c, scope, is_training=True, relu=True):
    """Final predication conv on a channel slice of a head tensor:
    out = relu(bn(conv1x1(x[..., xo:xo+c], c)))   (pixel_cls / link_cls,
    nets/model_vgg_16.py:166,173).  Returns a contiguous SmallAct [n,h,w,c]."""
    return _pointwise(g, x, xo, c, scope, "bn", is_training, relu)


def pointwise_bias(g, x, xo, c, scope, initializer=None):
    """text_predication / link_predication: 1x1 conv with biases and no activation on a channel
    slice of the fused head tensor (nets/pixellink.py:61,67).  Returns contiguous logits."""
    return _pointwise(g, x, xo, c, scope, "bias", initializer=initializer)


def pointwise_pair(g, x, scopes, *, mode="bn", is_training=True, relu=True, initializer=None):
    """The two predication convolutions on the fused 18-channel head tensor — pixel (2 -> 2 on channels 0..1) and link
    (16 -> 16 on channels 2..17): `pointwise_bn` x 2 (nets/model_vgg_16.py:166,173: conv + BN + ReLU) or `pointwise_bias`
    x 2 (nets/pixellink.py:61,67, nets/model.py:139-141: conv + biases, linear) — as ONE pass over the tensor per
    direction, same variables in the same order.  Returns (pixel SmallAct [n,h,w,2], link SmallAct [n,h,w,16])."""
    n, h, w, C = x.data.shape
    if not BATCH_HEADS or g.precision == "f32" or C != 18:
        return tuple(_pointwise(g, x, xo, c, scope, mode, is_training, relu, initializer)
                     for xo, c, scope in ((0, 2, scopes[0]), (2, 16, scopes[1])))
    P = n * h * w
    ws = g.workspace()
    T = ops.sc_pointwise_pair_num_partials(P) if mode == "bn" and is_training else None
    hd = []
    for scope, c in zip(scopes, (2, 16)):
        wv, bn_vars, bias = _pointwise_vars(g, scope, c, mode, initializer)
        d = HeadSource(P, c, wv, bn_vars, bias, g.empty((n, h, w, c), F32))
        if mode == "bn":
            _bn_alloc(g, d, T)
            d.out = SmallAct(g.empty((n, h, w, c), F32))        # relu(bn(z)), written below
        hd.append(d)
    a, b = hd
    ops.sc_pointwise_pair_fwd(x.data, a.wv.data, _data(a.bias), b.wv.data, _data(b.bias), a.z, b.z, a.part, b.part)
    if mode == "bn":
        _bn_fill(hd, is_training)
        ops.sc_act_batch([(d.z, d.scale, d.shift, d.out.data) for d in hd], relu)

    def backward():
        if a.out.grad is None and b.out.grad is None:
            return
        for d in hd:
            if d.out.grad is None:                       # a head the loss did not read: its gradient is zero
                d.out.grad = g.empty(d.out.data.shape, F32)
                ops.fill_(d.out.grad, 0.0)
        if mode == "bn":
            _bn_bwd_batch(g, hd, relu, is_training)
        else:
            for d in hd:
                d.dz = d.out.grad
        if x.grad is not None:
            raise RuntimeError("the fused head tensor already carries a gradient (pointwise_pair writes all of it)")
        x.grad = g.empty(x.data.shape, F32)
        ops.sc_pointwise_pair_bwd(x.data, a.dz, b.dz, a.wv.data, b.wv.data, x.grad, a.wv.grad, _grad(a.bias),
                                  b.wv.grad, _grad(b.bias), ws)
        for d in hd:
            d.out.grad = d.dz = None
    g.record(backward, _produces(hd))
    return a.out, b.out


# ---------------------------------------------------------------------------- heads on EAST's merge branch
def sigmoid_head(g, feat, cout, scope):
    """slim.conv2d(feat, cout, 1, activation_fn=tf.nn.sigmoid, normalizer_fn=None) (model_vgg_16.py:129-131)."""
    z, _, _ = head_conv_bias(g, feat, (scope,), (cout,))
    out = SmallAct(g.empty(z.data.shape, F32))
    ops.sc_sigmoid(z.data, out.data)

    def backward():
        if out.grad is None:
            return
        z.grad = g.empty(z.data.shape, F32)
        ops.sc_sigmoid_bwd(out.data, out.grad, z.grad)
        out.grad = None
    g.record(backward)
    return out


def sigmoid_heads(g, feat, couts, scopes):
    """The two sigmoid heads on the merge branch's output (nets/model_vgg_16.py:129-131: F_score = conv1x1 -> 1,
    geo_map = conv1x1 -> 8, both sigmoid, biases, no normaliser) as ONE merged 1x1 convolution over the feature
    (head_conv_bias: variable `<scope0>+<scope1>/weights` [cin, 1+8], split back into the reference's two by
    checkpoint.internal_to_tf) — one pass over the 105 MB feature for the forward, the weight gradient and the input
    gradient instead of two each.  Returns the two activation handles."""
    if g.precision == "f32" or not MERGE_HEADS:
        return tuple(sigmoid_head(g, feat, c, s) for c, s in zip(couts, scopes))
    z, _, _ = head_conv_bias(g, feat, tuple(scopes), tuple(couts))
    n, h, w, _ = z.data.shape
    o0 = SmallAct(g.empty((n, h, w, couts[0]), F32))
    o1 = SmallAct(g.empty((n, h, w, couts[1]), F32))
    ops.sc_sigmoid_split(z.data, couts[0], o0.data, o1.data)

    def backward():
        if o0.grad is None and o1.grad is None:
            return
        z.grad = g.empty(z.data.shape, F32)
        ops.sc_sigmoid_split_bwd(o0.data, o0.grad, o1.data, o1.grad, z.grad)
        o0.grad = o1.grad = None
    g.record(backward)
    return o0, o1


def rbox_heads(g, feat, scopes, text_scale):
    """EAST's RBOX heads on the merge branch's output (reference nets/model.py:76-80): F_score = sigmoid(conv1x1 -> 1),
    four distances = sigmoid(conv1x1 -> 4) * text_scale, angle = (sigmoid(conv1x1 -> 1) - 0.5) * pi/2, as ONE merged 1x1
    convolution (head_conv_bias: variable `<s0>+<s1>+<s2>/weights` [cin, 1+4+1], split back into the reference's
    three by checkpoint.internal_to_tf) and one f32 activation kernel (ops.rbox_head_fwd).  Returns the handles
    (F_score [n,h,w,1], F_geometry [n,h,w,5]).  With the f32 inference precision or OCR_RESNET_MERGE_HEADS=0: one
    convolution per head, the same activation kernel on their concatenation."""
    couts = (1, 4, 1)
    if g.precision == "f32" or not MERGE_HEADS:
        if g.keepalive is not None:
            # the columns are gathered / scattered by torch copies, which a recorded step plan does not replay
            raise NotImplementedError("rbox_heads with OCR_RESNET_MERGE_HEADS=0 cannot run inside a recorded step")
        zs = [head_conv_bias(g, feat, (s,), (c,))[0] for s, c in zip(scopes, couts)]
        z = SmallAct(torch.cat([t.data for t in zs], dim=-1))
    else:
        zs = None
        z, _, _ = head_conv_bias(g, feat, tuple(scopes), couts)
    n, h, w, _ = z.data.shape
    o0 = SmallAct(g.empty((n, h, w, 1), F32))
    o1 = SmallAct(g.empty((n, h, w, 5), F32))
    ops.rbox_head_fwd(z.data, float(text_scale), o0.data, o1.data)

    def backward():
        if o0.grad is None and o1.grad is None:
            return
        z.grad = g.empty(z.data.shape, F32)
        ops.rbox_head_bwd(o0.data, o0.grad, o1.data, o1.grad, float(text_scale), z.grad)
        if zs is not None:
            o = 0
            for t, c in zip(zs, couts):
                t.grad = z.grad[..., o:o + c].contiguous()
                o += c
        o0.grad = o1.grad = None
    g.record(backward)
    return o0, o1
