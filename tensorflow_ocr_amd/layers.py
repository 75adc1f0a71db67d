"""slim-style layers (conv2d [+batch_norm] [+relu] [+max_pool2d]) driving the HIP kernels; the fuse heads on top of
them are in head_layers.py.

Each function runs the forward kernels immediately and records ONE backward closure on the
graph's tape.  Variable names follow tf.contrib.slim so checkpoints/state-dicts line up with
the reference: `<scope>/weights`, `<scope>/biases`,
`<scope>/BatchNorm/{gamma,beta,moving_mean,moving_variance}`.
"""
import functools
import os
from typing import NamedTuple

import torch

from . import ops
from .graph import Act, BnCtx, F16, F32, Partial, PoolGrad, constant, variance_scaling
from ._lib import CONV_ACCUM_F16, CONV_BIAS, CONV_RELU, CONV_STATS

BN_DECAY = 0.997
BN_EPS = 1e-5


def _switch(name, default=True):
    """A host-side switch: `name` in the environment ("1" / "0"), read once at import."""
    return os.environ.get(name, "1" if default else "0") == "1"


def _switch_int(name, default):
    return int(os.environ.get(name, str(default)))


FUSE_BN_REDUCE = _switch("OCR_FUSE_BN")   # BN-backward reduction inside the consumer's input-gradient kernel
FUSE_BIAS_POOL = _switch("OCR_FUSE_BIAS_POOL")   # bias nets: conv1_2's bias + ReLU + pool in the conv epilogue
FUSE_BIAS_RELU = _switch("OCR_FUSE_BIAS_RELU")   # bias nets: ReLU mask + bias gradient in the consumer's dgrad epilogue
FUSE_BN_W4_MAXHW = _switch_int("OCR_FUSE_BN_W4_MAXHW", 1000000)
FUSE_BN_POOL_REDUCE = _switch("OCR_FUSE_BN_POOL_REDUCE")    # measurement switch
FIRST_RECOMPUTE = _switch("OCR_FIRST_RECOMPUTE")            # measurement switch (forward: 439 -> 318 us)
FIRST_DROP_Y = _switch("OCR_FIRST_DROP_Y")                  # conv1_1's y is never stored (ops.LazyFirstY)
FIRST_MOMENTS = _switch("OCR_FIRST_MOMENTS")                # ... and its statistics come from the image's moments
# conv1_1's weight gradient recomputing y even when y IS stored: bit-identical, but no faster by itself (413 vs 402 us at
# 32 x 512^2: with one stream instead of two the kernel is bound by its per-tile LDS work, not by HBM).  With
# FIRST_DROP_Y (y never stored) the recomputing form is what runs regardless of this switch.
FIRST_WGRAD_RECOMPUTE = _switch("OCR_FIRST_WGRAD_RECOMPUTE", False)
GUEST_REDUCE = _switch("OCR_GUEST_REDUCE")            # end-point layers' BN-backward reduction as a guest pass
FUSE_FIRST_WGRAD = _switch("OCR_FUSE_FIRST_WGRAD")    # measurement switch
# conv1_1's weight gradient from SUMS (csrc/conv_first.hip: first_wgrad_sums_kernel): conv1_2's input-gradient launch
# leaves S1 = V^T dz instead of the 1 GiB gradient, dW = A .* S1 + B .* (M W) + C .* m
FIRST_WGRAD_SUMS = _switch("OCR_FIRST_WGRAD_SUMS")


def _bn_vars(g, C):
    with g.variable_scope("BatchNorm"):
        gamma = g.get_variable("gamma", (C,), constant(1.0))
        beta = g.get_variable("beta", (C,), constant(0.0))
        mm = g.get_variable("moving_mean", (C,), constant(0.0), trainable=False)
        mv = g.get_variable("moving_variance", (C,), constant(1.0), trainable=False)
    return gamma, beta, mm, mv


def _bn_buffers(g, C):
    """scale, shift, mean, invstd of one batch norm (f32 [C] each)."""
    return g.empty((C,), F32), g.empty((C,), F32), g.empty((C,), F32), g.empty((C,), F32)


def _bn_params(g, C, bn_vars, stats):
    """scale, shift, mean, invstd: from the batch's partial sums while training (stats = (part, T, count, stage); moves
    the moving statistics too), from the moving statistics otherwise (stats = None)."""
    gamma, beta, mm, mv = bn_vars
    scale, shift, mean, invstd = _bn_buffers(g, C)
    if stats is not None:
        part, T, count, stage = stats
        ops.bn_finalize(part, T, C, count, gamma.data, beta.data, BN_EPS, BN_DECAY, mm.data, mv.data,
                        scale, shift, mean, invstd, stage)
    else:
        ops.bn_inference_params(gamma.data, beta.data, mm.data, mv.data, BN_EPS, scale, shift)
    return scale, shift, mean, invstd


def _coef(g, c):
    """The batch-norm backward's apply coefficients (A, B, C): dy = A * dz + B * y + C per channel."""
    return g.empty((c,), F32), g.empty((c,), F32), g.empty((c,), F32)


def _bn_bwd_coef(g, bn, partial, T, count, pre=False):
    """dgamma / dbeta and the apply coefficients from sums already reduced to `partial` rows; bn = (scale, mean, invstd,
    gamma, beta); pre: tagged as the front of a guest apply pass."""
    scale, mean, invstd, gamma, beta = bn
    c = scale.numel()
    coef = _coef(g, c)
    fn = ops.bn_bwd_coefficients_pre if pre else ops.bn_bwd_coefficients
    fn(partial, T, c, count, scale, mean, invstd, gamma.grad, beta.grad, coef, g.workspace())
    return coef


def _packs(g, w, first):
    """f16 operand layouts of a conv weight: forward [tap][cout][cin] and dgrad [tap][cin][cout]."""
    kh, kw, cin, cout = w.shape
    if first:
        def mk(old):
            t = old if old is not None else g.empty((3, cout, 16))
            ops.pack_weights_first(w.data, t)
            return t
        return g.packed(w, "first", mk), None

    def mk(old):
        if old is None:
            old = (g.empty((kh * kw, cout, cin)), g.empty((kh * kw, cin, cout)))
        ops.pack_weights(w.data, old[0], old[1])
        return old
    return g.packed(w, "kc_ck", mk)


def conv2d(g, x, cout, k, scope, *, stride=1, rate=1, normalizer="bn", relu=True, pool=0,
           keep_full=True, is_training=True, bn_training=None, first=False, weight_decay=True,
           initializer=None):
    """slim.conv2d(+batch_norm)(+ReLU), optionally fused with the following 2x2/2 max-pool.

    x: Act f16 [n,h,w,cin] (for `first`: the [n,h,w,4] prepared image).
    normalizer: "bn" (no bias, slim drops it) or None (bias).
    Returns (full, pooled) Acts; `full` is None when keep_full=False and pool>0.
    Reference: nets/vgg.py:14-39 under resnet_arg_scope (nets/model_vgg_16.py:144) or the
    PixelLink bias scope (nets/pixellink.py:41-48).
    """
    if g.precision == "f32":
        from . import layers_f32
        return layers_f32.conv2d(g, x, cout, k, scope, stride=stride, rate=rate, normalizer=normalizer,
                                 relu=relu, pool=pool, keep_full=keep_full, is_training=is_training,
                                 bn_training=bn_training, first=first, weight_decay=weight_decay,
                                 initializer=initializer)
    # what the two layers share: variables, operand packs, descriptor, partial-row count and the raw output
    n, h, w, cin_x = x.shape
    cin = 3 if first else cin_x
    bn_training = is_training if bn_training is None else bn_training
    with g.variable_scope(scope):
        init = initializer or variance_scaling(g.rng)
        wv = g.get_variable("weights", (k, k, cin, cout), init, regularized=weight_decay)
        if normalizer == "bn":
            bn_vars = _bn_vars(g, cout)
        else:
            bias = g.get_variable("biases", (cout,), constant(0.0))
    g.workspace()
    packs = _packs(g, wv, first)
    if first:
        d = None
        oh, ow = h, w
        mt = ops.conv2d_first_num_mtiles(n, h, w)
    else:
        d = ops.conv_desc((n, h, w, cin), cout, k, k, stride, rate)
        oh, ow = d.oh, d.ow
        mt = ops.conv2d_num_mtiles(d)
    # conv1_1 under training-mode batch norm: y is never stored — the statistics pass writes nothing, the activation and
    # the two readers of y in the backward pass (conv1_2's fused BN-backward sums, conv1_1's own weight gradient)
    # evaluate the 3-channel convolution again; a consumer that cannot asks the LazyFirstY for the tensor
    drop_y = (first and normalizer == "bn" and not pool and cout == 64 and FIRST_RECOMPUTE and FIRST_DROP_Y
              and bn_training and FUSE_FIRST_WGRAD)
    shape = (n, oh, ow, cout)
    y = ops.LazyFirstY(g.empty, x.data, packs[0], shape) if drop_y else g.empty(shape)
    if normalizer == "bn":
        return _conv2d_bn(g, x, scope, wv, bn_vars, packs, d, mt, y, shape, relu, pool, keep_full, bn_training, first)
    return _conv2d_bias(g, x, scope, wv, bias, packs, d, y, shape, relu, pool, keep_full, is_training, first)


def _conv2d_bn(g, x, scope, wv, bn_vars, packs, d, mt, y, shape, relu, pool, keep_full, train_stats, first):
    """conv2d's batch-norm layer: statistics in the convolution's epilogue, normalise + ReLU (+ pool) in one pass."""
    gamma, beta = bn_vars[:2]
    w_fwd, w_dg = packs
    n, oh, ow, cout = shape
    count = float(n) * oh * ow
    ws = g.workspace()
    drop_y = isinstance(y, ops.LazyFirstY)
    flags = CONV_STATS if train_stats else 0
    part, stage = _stats_rows(g, mt, cout)
    mt_fin = mt
    if first and drop_y and train_stats and FIRST_MOMENTS:
        # the statistics from the image's second moments (csrc/conv_first.hip: first_moments_kernel): no pass over the
        # 64-channel output at all; one partial row
        if FIRST_WGRAD_SUMS:
            y.moments = g.empty((32 * 32,), torch.float64)      # kept for the backward (ops.conv2d_first_wgrad_sums)
        ops.conv2d_first_moments(x.data, w_fwd, part, cout, ws, moments=y.moments)
        mt_fin = 1
    elif first:
        ops.conv2d_first(x.data, w_fwd, None if drop_y else y, flags, None, part if train_stats else None, cout=cout)
    else:
        d.flags = flags
        ops.conv2d(d, x.data, w_fwd, y, None, part if train_stats else None)
    scale, shift, mean, invstd = _bn_params(g, cout, bn_vars, (part, mt_fin, count, stage) if train_stats else None)
    bn = (scale, mean, invstd, gamma, beta)
    even = oh % 2 == 0 and ow % 2 == 0
    full = pooled = None
    argmax = y_pool = argmax_full = None
    if pool:
        pooled = g.empty((n, (oh + 1) // 2, (ow + 1) // 2, cout))
        if keep_full:
            full = g.empty(shape)
            if train_stats and relu and ops.guest_apply_ok(shape) and even:
                # an end point that is also pooled (conv3_3 / conv4_3): keep the first-max positions, so that the
                # backward's apply pass can run as a guest (ops.bn_relu_poolfull_bwd_apply_affine) without
                # re-deriving them
                argmax_full = g.empty(pooled.shape, torch.uint8)
                ops.bn_relu_pool_idx(y, scale, shift, relu, full, pooled, argmax_full, None)
            else:
                ops.bn_relu(y, scale, shift, relu, 2, full, pooled)
        else:
            # the pool is the only consumer: keep the first-max position so that the backward routes
            # the pooled gradient without re-deriving the four candidates' activations
            argmax = g.empty(pooled.shape, torch.uint8)
            # ... and, while training, the conv output AT that position: dz is zero everywhere else, so the conv
            # that consumes the pooled activation can sum this layer's BN-backward terms over the pooled
            # positions in its input-gradient epilogue (a_pool.bn_ctx below) and the reduction pass over y goes
            y_pool = g.empty(pooled.shape) if (train_stats and FUSE_BN_POOL_REDUCE) else None
            ops.bn_relu_pool_idx(y, scale, shift, relu, None, pooled, argmax, y_pool)
    else:
        full = g.empty(shape)
        if first and FIRST_RECOMPUTE:
            # conv1_1: evaluating the 3-channel convolution again costs 67 MB of reads, the element-wise pass 1 GiB
            ops.conv2d_first_bn_relu(x.data, w_fwd, scale, shift, relu, full)
        else:
            ops.bn_relu(y.tensor() if drop_y else y, scale, shift, relu, 0, full, None)
    a_full = Act(full, name=scope) if full is not None else None
    a_pool = Act(pooled, name=scope + "/pool") if pooled is not None else None
    if not pool and train_stats:
        # lets the consumer conv's input-gradient kernel do this layer's BN-backward reduction
        a_full.bn_ctx = BnCtx(y, scale, shift, mean, invstd, relu)
    if pool and argmax is not None and y_pool is not None:
        a_pool.bn_ctx = BnCtx(y_pool, scale, shift, mean, invstd, relu)

    def first_from_sums():
        # conv1_1 whose sole consumer left the sums instead of the gradient (input_grad): dgamma / dbeta and the
        # apply coefficients from the partial rows, then dW = A .* S1 + B .* (M W) + C .* m — no pass over a
        # 64-channel tensor at all
        coef = _bn_bwd_coef(g, bn, *a_full.bn_partial, count)
        ops.conv2d_first_wgrad_sums(a_full.first_s1, y.moments, w_fwd, coef, wv.grad)
        a_full.bn_partial = None
        a_full.first_s1 = None

    def first_wgrad_applies(da_full):
        # conv1_1: no input gradient, so the weight gradient is the only reader of dy — it applies the BN
        # backward while staging its tiles and dy is never written (ocr_conv2d_first_wgrad_bn_f16)
        coef = _bn_bwd_coef(g, bn, *a_full.bn_partial, count)
        lazy = drop_y
        if lazy and y.t is not None:
            lazy, y_t = False, y.t                # somebody had it evaluated: read it
        else:
            y_t = None if lazy else y
        ops.conv2d_first_wgrad_bn(x.data, da_full, y_t, shift, coef, relu, wv.grad, ws,
                                  w_first=w_fwd if (lazy or FIRST_WGRAD_RECOMPUTE) else None)
        a_full.bn_partial = None
        a_full.grad = None

    def backward():
        if not train_stats:
            raise NotImplementedError("backward through inference-mode batch norm")
        da_full = a_full.grad if a_full is not None else None
        da_pool = a_pool.grad if a_pool is not None else None
        if first and a_full is not None and a_full.first_s1 is not None:
            return first_from_sums()                          # conv1_1
        if da_full is None and da_pool is None:
            return
        if pool and da_pool is None:
            da_pool = g.empty(a_pool.data.shape)
            ops.fill_(da_pool, 0.0)
        if not pool and da_full is None:
            return
        if first and not pool and a_full.bn_partial is not None and FUSE_FIRST_WGRAD:
            return first_wgrad_applies(da_full)               # conv1_1 with FIRST_WGRAD_SUMS off
        y_b = y.tensor() if drop_y else y                     # (the unfused routes below read y)
        dy = g.empty(y_b.shape)
        guest_ok = ops.guest_apply_ok(y_b.shape)
        if not pool and a_full.bn_partial is not None:
            # the sole consumer's input-gradient kernel summed this layer's terms (conv2_1 ... conv5_2, fc6)
            part_f, T_f = a_full.bn_partial
            if guest_ok:
                # the apply pass as a GUEST (csrc/guest_bn.hip): dgamma / dbeta / coefficients first, then one slim
                # launch that the recorded step runs beside the weight gradient of the layer above
                coef = _bn_bwd_coef(g, bn, part_f, T_f, count, pre=True)
                ops.bn_relu_bwd_apply_affine(y_b, da_full, scale, shift, coef[1], coef[2], relu, dy)
            else:
                ops.bn_relu_bwd_apply(y_b, scale, shift, mean, invstd, da_full, relu, part_f, T_f,
                                      gamma.grad, beta.grad, dy, ws)
            a_full.bn_partial = None
        elif pool and argmax is not None and da_full is None and a_pool.bn_partial is not None:
            # ... summed them over the pooled positions (conv1_2, conv2_2: the pool is the only reader)
            part_p, T_p = a_pool.bn_partial
            if guest_ok and even:
                coef = _bn_bwd_coef(g, bn, part_p, T_p, count, pre=True)
                ops.bn_relu_pool_bwd_idx_apply_affine(y_b, argmax, da_pool, coef, relu, dy)
            else:
                ops.bn_relu_pool_bwd_idx_apply(y_b, scale, mean, invstd, argmax, da_pool, relu, part_p, T_p,
                                               gamma.grad, beta.grad, dy, ws)
            a_pool.bn_partial = None
        elif pool and argmax is not None and da_full is None:
            # the same layers with nobody having summed (FUSE_BN_REDUCE / FUSE_BN_POOL_REDUCE off): one pass, routed by index
            ops.bn_relu_pool_bwd_idx(y_b, scale, mean, invstd, a_pool.data, argmax, da_pool, relu,
                                     gamma.grad, beta.grad, dy, ws)
        elif (not pool or argmax_full is not None) and da_full is not None and guest_ok:
            # no consumer summed this layer's terms (several contributed to its gradient: an end point of the fuse
            # heads — conv3_3, conv4_3, conv5_3, fc7): the reduction pass stays, its finalize emits the coefficients,
            # the apply pass is a guest
            if GUEST_REDUCE and (relu or not pool):
                # ... as a guest as well (beside weight gradients still held back), its rows folded on the main stream
                part_e, T_e = ops.bn_relu_bwd_reduce_rows(y_b, da_full, scale, shift, mean, invstd, relu, g.empty,
                                                          da_pool=da_pool if pool else None,
                                                          argmax=argmax_full if pool else None)
                coef = _bn_bwd_coef(g, bn, part_e, T_e, count, pre=True)
            else:
                coef = _coef(g, cout)
                ops.bn_relu_bwd_reduce(y_b, scale, shift, mean, invstd, da_full, relu, gamma.grad, beta.grad, coef, ws,
                                       da_pool=da_pool if pool else None)
            if pool:
                ops.bn_relu_poolfull_bwd_apply_affine(y_b, da_full, da_pool, argmax_full, scale, shift, coef, relu, dy)
            else:
                ops.bn_relu_bwd_apply_affine(y_b, da_full, scale, shift, coef[1], coef[2], relu, dy)
        else:
            # everything else (shapes the guest passes do not take, a pooled end point without its index): the plain pass
            ops.bn_relu_bwd(y_b, scale, shift, mean, invstd, da_full, da_pool, relu, 2 if pool else 0,
                            gamma.grad, beta.grad, dy, ws)
        _conv_backward(g, x, wv, w_dg, d, dy, first)
        if a_full is not None:
            a_full.grad = None
        if a_pool is not None:
            a_pool.grad = None
    g.record(backward, (wv, gamma, beta))
    return a_full, a_pool


def _conv2d_bias(g, x, scope, wv, bias, packs, d, y, shape, relu, pool, keep_full, is_training, first):
    """conv2d's bias (+ReLU) layer: PixelLinkNet's VGG (nets/pixellink.py:41-48)."""
    w_fwd, w_dg = packs
    n, oh, ow, cout = shape
    ws = g.workspace()
    flags = CONV_BIAS | (CONV_RELU if relu else 0)
    if (pool == 2 and relu and not keep_full and not first and FUSE_BIAS_POOL
            and ops.conv2d_variant(d) == "conv_c64_persist_kernel<64>"):
        # conv1_2 (64 -> 64 at full resolution) followed by its pool, the full-resolution activation wanted by nobody:
        # bias + ReLU + 2x2 max-pool inside the convolution's epilogue, only the pooled activation (+ first-max
        # positions while training) is written — 1/4 of the bytes and no pooling pass
        ph, pw_ = (oh + 1) // 2, (ow + 1) // 2
        pooled = g.empty((n, ph, pw_, cout))
        argmax = g.empty((n, ph, pw_, cout), torch.uint8) if is_training else None
        d.flags = flags
        ops.conv2d_relu_pool(d, x.data, w_fwd, bias.data, pooled, argmax)
        a_pool = Act(pooled, name=scope + "/pool")

        def backward_pool():
            if a_pool.grad is None:
                return
            if argmax is None:
                # an is_training=False build is forward-only here as it is under batch norm: the first-max positions
                # the routing needs were not kept, and the full-resolution activation was never written
                raise NotImplementedError("backward through a conv + ReLU + pool built with is_training=False "
                                          "(the first-max positions are kept only while training)")
            # ReLU mask and bias gradient on the pooled tensors (a window maximum is positive iff the element its
            # gradient is routed to is), then the routed gradient IS dz of the convolution
            dzp = g.empty(pooled.shape)
            ops.bias_relu_bwd(pooled, a_pool.grad, True, dzp, bias.grad, ws)
            dz = g.empty(shape)
            ops.maxpool_bwd(None, dzp, 2, 2, (0, 0), dz, False, argmax=argmax, in_shape=shape)
            _conv_backward(g, x, wv, w_dg, d, dz, first)
            a_pool.grad = None
        g.record(backward_pool, (wv, bias))
        return None, a_pool
    if first:
        ops.conv2d_first(x.data, w_fwd, y, flags, bias.data, None)
    else:
        d.flags = flags
        ops.conv2d(d, x.data, w_fwd, y, bias.data, None)
    a_full = Act(y, name=scope)
    if relu and is_training:
        a_full.bias_ctx = BnCtx.of_bias(g, y, cout)

    def backward_bias():
        if a_full.grad is None:
            return
        if a_full.bias_done:
            dz = a_full.grad                       # masked and summed on the POOLED tensors (max_pool2d below)
            a_full.bias_done = False
        elif a_full.bias_partial is not None:
            # a_full.grad IS dz already (masked by the consumer's input-gradient kernel); its partial rows sum to dbias
            part_f, T_f = a_full.bias_partial
            ops.bn_bwd_sums(part_f, T_f, cout, bias.grad, g.ws_small.get(cout * 4)[:cout * 4].view(F32), ws)
            dz = a_full.grad
            a_full.bias_partial = None
        else:
            dz = g.empty(y.shape)
            ops.bias_relu_bwd(y, a_full.grad, relu, dz, bias.grad, ws)
        _conv_backward(g, x, wv, w_dg, d, dz, first)
        a_full.grad = None
    g.record(backward_bias, (wv, bias))
    a_pool = max_pool2d(g, a_full, 2, 2, scope=scope + "/pool", bias_relu=bias if (relu and is_training) else None) if pool else None
    return a_full, a_pool


def _wgrad_desc(d):
    """The weight gradient's descriptor of the forward convolution `d`: same geometry, no flags."""
    return ops.ConvDesc(d.n, d.h, d.w, d.cin, d.oh, d.ow, d.cout, d.kh, d.kw, d.stride, d.dilation,
                        d.pad_top, d.pad_left, 0, 0)


def _dgrad_desc(d, flags):
    """dx = conv(dy, W^T flipped) of the stride-1 convolution `d`: input = dy [n,oh,ow,cout], output = [n,h,w,cin]."""
    pt = d.dilation * (d.kh - 1) - d.pad_top
    pl = d.dilation * (d.kw - 1) - d.pad_left
    return ops.ConvDesc(d.n, d.oh, d.ow, d.cout, d.h, d.w, d.cin, d.kh, d.kw, 1, d.dilation, pt, pl, 1, flags)


def _partial_rows(g, dg):
    """(partial, T): the [T, 2, channels] f32 rows a fused input-gradient epilogue leaves its sums in."""
    T = ops.conv2d_num_mtiles(dg)
    return g.empty((T, 2, dg.cout), F32), T


def _stats_rows(g, T, c):
    """(part, stage) in the small arena: the [T, 2, c] f32 rows a forward launch leaves its statistics in, and the
    staging ops.bn_finalize folds them through."""
    return g.ws_small.two(T * 2 * c * 4, ops.bn_reduce_workspace(T, c))


def _conv_backward(g, x, wv, w_dg, d, dy, first):
    """Weight gradient (always) and input gradient (when the input needs one)."""
    ws = g.workspace()
    if first:
        ops.conv2d_first_wgrad(x.data, dy, wv.grad, ws)
        return
    dd = _wgrad_desc(d)
    if ops.GUEST_BN and x.requires_grad:
        # input gradient FIRST: the layer below can then start its backward while this layer's weight gradient runs —
        # its batch-norm apply pass is a guest beside it (csrc/guest_bn.hip; the recorded step pairs the two)
        input_grad(g, x, d, w_dg, dy, conv2d_routes=True)
        ops.conv2d_wgrad(dd, x.data, dy, wv.grad, g.ws_wgrad, alloc=lambda nb: g.empty((nb,), torch.uint8))
        return
    ops.conv2d_wgrad(dd, x.data, dy, wv.grad, g.ws_wgrad)
    if x.requires_grad:
        input_grad(g, x, d, w_dg, dy, conv2d_routes=True)


class PwxOperand(NamedTuple):
    """input_grad's `fused`: dy is still EMPTY — it is the batch-norm backward apply A*dz + B*y + C (coef = (A, B, C)), masked
    by the ReLU of that batch norm when relu_shift (its shift) is given, which the 1x1 input-gradient convolution computes
    while loading its operand (conv_pwx_kernel) and writes into dy for the weight gradient."""
    dz: object
    y: object
    coef: tuple
    relu_shift: object


def select_input_grad(x, d, *, fused, last, variant, plain_only=False, conv2d_routes=False, tail=False,
                      tail_1x1_only=False, bnred_unpended_only=False, first_sums=True):
    """Which launch the backward of convolution `d` (its FORWARD descriptor, stride 1) issues for the gradient of its input
    x: the epilogue, behind "pwx_" when `fused` (a PwxOperand) asks for the operand-transforming loader.  Pure: it reads x,
    the switches and — through variant(), the kernel the library runs for this launch — nothing else.

      first_sums   x is conv1_1's activation and nobody stored conv1_1's y: the launch leaves the sums conv1_1's weight
                   gradient is finished from INSTEAD of the gradient (that gradient has no other reader)
      bias_masked  x = relu(conv + bias): the gradient is stored past the ReLU, beside the bias gradient's sums
      tail         the LAST contribution (`last`) to a bottleneck output: the gradient is stored past the output's ReLU,
                   beside the BN-backward sums of the unit's last conv
      bnred_first  x = relu?(bn(y)): the BN-backward sums of that layer, conv1_1's y recomputed in the epilogue ...
      bnred        ... or read
      plain        the gradient and nothing else
    Every fused epilogue but `tail` describes the whole gradient only while it is the FIRST contribution.

    The callers differ, and each difference has a name here:
      plain_only           the merge convolutions (_cat_backward) never fuse
      conv2d_routes        layers.conv2d alone knows first_sums, bias_masked, bnred_first — all for an x the net marked
                           sole_consumer or that is conv1_1's — and the FUSE_BN_W4_MAXHW cut-off
      tail                 the caller's FUSE_TAIL: resnet_layers alone builds bottlenecks
      tail_1x1_only        its unfused launch takes the tail route for a 1x1 convolution only (a fused one is 1x1 anyway)
      bnred_unpended_only  its fused launch leaves an x that counts contributions (x.pending) to the tail route
      first_sums           False: the library has answered that it does not take this shape (input_grad)"""
    pwx = "pwx_" if fused is not None else ""
    if plain_only:
        return pwx + "plain"
    first = x.grad is None
    by = x.bn_ctx.y if x.bn_ctx is not None else None
    lazy_first = isinstance(by, ops.LazyFirstY) and by.t is None and d.cin == 64      # conv1_1's y, stored by nobody
    if conv2d_routes and first and x.sole_consumer:
        if first_sums and FIRST_WGRAD_SUMS and FUSE_BN_REDUCE and lazy_first and by.moments is not None:
            return pwx + "first_sums"
        if x.bias_ctx is not None and FUSE_BIAS_RELU:
            return pwx + "bias_masked"
    if tail and last and x.tail_ctx is not None and (d.kh == 1 or not tail_1x1_only):
        return pwx + "tail"
    if not (x.bn_ctx is not None and first and FUSE_BN_REDUCE):
        return pwx + "plain"
    if fused is not None and fused.relu_shift is not None:
        return pwx + "plain"        # (ocr_conv2d_pw_bnbwd_bnred_f16 has no ReLU mask on load)
    if bnred_unpended_only and x.pending is not None:
        return pwx + "plain"
    if conv2d_routes and d.h >= FUSE_BN_W4_MAXHW and variant() == "conv3x3_w4_kernel":
        return pwx + "plain"        # (measurement switch: the one-wave-per-SIMD kernel cannot overlap its epilogue with anything)
    if conv2d_routes and lazy_first and variant() == "conv_c64_persist_kernel<64>":
        return pwx + "bnred_first"
    return pwx + "bnred"


# the Act slot in which each fused epilogue leaves its Partial for the producer's backward
_PARTIAL_SLOT = {"first_sums": "bn_partial", "bnred_first": "bn_partial", "bnred": "bn_partial",
                 "bias_masked": "bias_partial", "tail": "tail_partial"}


def input_grad(g, x, d, w_dg, dy, *, owner=None, fused=None, **guards):
    """The input-gradient launch of the convolution with forward descriptor `d` and input-gradient pack w_dg, into x's
    gradient: the route select_input_grad names (guards: its named parameters), its partial rows and what it leaves
    on x.  owner: the bottleneck on whose behalf x's contributions are counted; fused: a PwxOperand."""
    if d.stride != 1:
        raise NotImplementedError("strided dgrad")
    dg = _dgrad_desc(d, 0)
    select = functools.partial(select_input_grad, x, d, fused=fused, last=x.count_contribution(owner),
                               variant=lambda: ops.conv2d_variant(dg), **guards)
    route = select()
    if route == "first_sums":
        blocks = ops.conv2d_bnred_first_wgrad_blocks(dg)
        if blocks <= 0:
            route = select(first_sums=False)
    if route != "first_sums":
        dx, accumulating = x.open_grad(g)
        dg.flags = CONV_ACCUM_F16 if accumulating else 0
    epilogue = route[4:] if fused is not None else route
    rows = None
    if epilogue != "plain":
        part = Partial(*_partial_rows(g, dg))
        setattr(x, _PARTIAL_SLOT[epilogue], part)
        rows = part.rows
    is_tail = epilogue == "tail"
    if fused is not None and epilogue == "bnred":
        ops.conv2d_pw_bnbwd_bnred(dg, fused.dz, fused.y, fused.coef, dy, w_dg, dx, rows, x.bn_ctx)
    elif fused is not None:
        ops.conv2d_pw_bnbwd_tail(dg, fused.dz, fused.y, fused.coef, fused.relu_shift, dy, w_dg, dx, rows,
                                 x.tail_ctx if is_tail else None, x.sub_grad if is_tail else None)
    elif epilogue == "first_sums":
        x.first_s1 = g.empty((blocks, 32, 64), F32)
        ops.conv2d_bnred_first_wgrad(dg, dy, w_dg, rows, x.bn_ctx.first(), x.first_s1)
    elif epilogue == "bnred_first":
        ops.conv2d_bnred_first(dg, dy, w_dg, dx, rows, x.bn_ctx.first())
    elif epilogue in ("bnred", "bias_masked"):
        masked = epilogue == "bias_masked"
        ops.conv2d_bnred(dg, dy, w_dg, dx, rows, x.bias_ctx if masked else x.bn_ctx, store_masked=masked)
    elif is_tail:
        ops.conv2d_bnred_tail(dg, dy, w_dg, dx, rows, x.tail_ctx, x.sub_grad)
    else:
        ops.conv2d(dg, dy, w_dg, dx, None, None)
    if is_tail:
        x.sub_grad = None


def max_pool2d(g, x, k, stride, scope="pool", bias_relu=None):
    """slim.max_pool2d(padding='SAME') as a standalone op (pool5 3x3/1, ResNet pool1, subsample).
    bias_relu: x = relu(conv + bias) and this is that layer's own pool (`bias_relu` = its bias variable): when the pool
    is the first to contribute to x's gradient, the ReLU mask and the bias gradient are taken on the POOLED tensors
    (the window maximum is positive iff the element the gradient is routed to is) and the routed gradient IS dz — the
    layer's full-resolution bias_relu_bwd pass disappears (PixelLink conv1_2 / conv2_2: 3 GiB and 1.5 GiB per step)."""
    if g.precision == "f32":
        from . import layers_f32
        return layers_f32.max_pool2d(g, x, k, stride, scope)
    n, h, w, c = x.shape
    oh, pt = ops.same_pad(h, k, stride)
    ow, pl = ops.same_pad(w, k, stride)
    y = g.empty((n, oh, ow, c))
    # index of the first maximum per window (TF gradient routing), kept for the backward pass
    argmax = g.empty((n, oh, ow, c), torch.uint8) if x.requires_grad else None
    fwd = x.bn_fwd
    if x.deferred is not None and fwd is not None:
        # x = relu(bn(y)) that nobody has computed yet (resnet_layers.root_block): the pool evaluates it per window
        # element from the raw conv output and x stays unwritten unless somebody else asks for x.data
        ops.bn_relu_maxpool(fwd.y, fwd.scale, fwd.shift, fwd.relu, k, stride, (pt, pl), y, argmax)
    else:
        ops.maxpool(x.data, k, stride, (pt, pl), y, argmax)
    out = Act(y, name=scope)

    def backward():
        if out.grad is None or not x.requires_grad:
            return
        if bias_relu is not None and x.grad is None and argmax is not None and FUSE_BIAS_RELU:
            dzp = g.empty(out.shape)
            ops.bias_relu_bwd(out.data, out.grad, True, dzp, bias_relu.grad, g.workspace())
            x.grad = g.empty(x.shape)
            ops.maxpool_bwd(x._data, dzp, k, stride, (pt, pl), x.grad, False, argmax=argmax, in_shape=x.shape)
            x.bias_done = True
            out.grad = None
            return
        if x.takes_pool_grad and x.grad is None and x.pool_grad is None and argmax is not None:
            # the producer gathers this gradient while it loads (resnet_layers.root_block): nothing is written here
            x.pool_grad = PoolGrad(out.grad, argmax, k, stride, (pt, pl))
            out.grad = None
            return
        dx, acc = x.open_grad(g)
        # (with the forward's index tensor the backward never reads x: do not force a deferred x into existence)
        ops.maxpool_bwd(x._data if argmax is not None else x.data, out.grad, k, stride, (pt, pl), dx, acc,
                        argmax=argmax, in_shape=x.shape)
        out.grad = None
    g.record(backward)
    return out


def prep_images(g, images, means=(123.68, 116.78, 103.94), div=1.0):
    """mean_image_subtraction (nets/model.py:18-31) + f16 cast into the [n,h,w,4] layout; `div`
    folds the PixelLink pipeline's `(x - 120) / 60` into the same pass."""
    if images.shape[-1] != len(means):
        raise ValueError("len(means) must match the number of channels")
    if g.precision == "f32":
        from . import layers_f32
        if div != 1.0:
            raise NotImplementedError("input normalisation is folded into the f16 path only")
        return layers_f32.prep_images(g, images, means)
    n, h, w, _ = images.shape
    x4 = g.empty((n, h, w, 4))
    ops.prep_images(images, x4, means, div)
    return Act(x4, requires_grad=False, name="images")
