"""Wrappers over the C ABI (include/ocr_hip.h).

Every function takes torch CUDA tensors purely as device-memory handles, passes raw
pointers + the current HIP stream through ctypes, and returns nothing new except
tensors it was asked to allocate.  There is no torch compute and no CPU fallback
here: without libocr_hip.so every call raises `_lib.OcrHipError`.

The wrappers of the training step and the inference forward (everything above `softmax_pairs`, the optimiser block
and the f32 / f16x2 block) check nothing: layer code that allocates every buffer itself calls them once, at record
time, and the replay never comes back here.  The decode, NMS, label, resize, evaluation, multi-scale, map-fusion, grid
and summary wrappers are called by tools, the feeder thread and users with tensors of their own, so each states its
operands once, as rows of `_operands`, which refuses a wrong shape, dtype, layout or device before a pointer is taken.
"""
import ctypes
import os
from ctypes import byref, c_double, c_float, c_int, c_int64, c_size_t

import torch

from . import _lib as L, step_plan
from . import graph as G      # (the handshake records only, at call time: graph imports this module)
from ._lib import ConvDesc, CONV_ACCUM_F16, CONV_BIAS, CONV_RELU, CONV_STATS, ptr

F16, F32 = (torch.bfloat16 if L.STORAGE == "bf16" else torch.float16), torch.float32


def _st():
    return L.stream_ptr()


def same_pad(size, k, stride, dilation=1):
    """TF 'SAME' padding for one spatial dim -> (out, pad_before)."""
    k_eff = (k - 1) * dilation + 1
    out = -(-size // stride)
    total = max((out - 1) * stride + k_eff - size, 0)
    return out, total // 2


class Workspace:
    """Stream-ordered scratch arena shared by all kernels of one tower."""

    def __init__(self, device, nbytes=64 << 20):
        self.device = device
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.retired = []

    def get(self, nbytes):
        if nbytes > self.buf.numel():
            # a recorded step plan or a captured HIP graph may hold raw pointers into the old arena:
            # it stays allocated (never handed back to the caching allocator) for the tower's lifetime
            self.retired.append(self.buf)
            self.buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=self.device)
        return self.buf

    def two(self, a_bytes, b_bytes):
        """Two disjoint 256-byte aligned regions."""
        a_al = (a_bytes + 255) // 256 * 256
        buf = self.get(a_al + b_bytes)
        return buf[:a_al], buf[a_al:a_al + b_bytes]


# ----------------------------------------------------------------------------- conv
def conv_desc(x_shape, cout, kh, kw, stride=1, dilation=1, pad=None, out_hw=None, flags=0,
              flip=0):
    n, h, w, cin = x_shape
    if pad is None:
        oh, pt = same_pad(h, kh, stride, dilation)
        ow, pl = same_pad(w, kw, stride, dilation)
    else:
        pt, pl = pad
        oh, ow = out_hw
    return ConvDesc(n, h, w, cin, oh, ow, cout, kh, kw, stride, dilation, pt, pl, flip, flags)


def conv2d_num_mtiles(d):
    return L.call_int("ocr_conv2d_num_mtiles", byref(d))


# When bench.py sets KERNEL_TIMING to a list, every implicit-GEMM conv launch is bracketed by
# HIP events on the launch stream and logged as (variant, flops, start_event, stop_event).
KERNEL_TIMING = None


_VARIANTS = {}


def conv2d_variant(d):
    """Which conv_igemm_kernel<BN,CK,WCO,M16,TH> instantiation the library launches for `d`."""
    key = (d.n, d.h, d.w, d.cin, d.cout, d.kh, d.kw, d.stride, d.dilation)
    v = _VARIANTS.get(key)
    if v is None:
        buf = ctypes.create_string_buffer(96)
        L.call_int("ocr_conv2d_variant", byref(d), buf, c_size_t(96))
        v = _VARIANTS[key] = buf.value.decode()
    return v


def _conv_call(fn, d, *args, phase, pwx=False, timed=False):
    """One conv entry point `fn(d, *args, stream)` with its tag (kernel instantiation, FLOP, phase) for the recorder:
    phase "fwd" launches run with nothing beside them, "dgrad" launches share the GPU with the side-stream weight
    gradients.  pwx: the operand-transforming 1x1 entries run conv_pwx_kernel where ocr_conv2d_variant names
    conv_pw_kernel.  timed: bracketed by HIP events when KERNEL_TIMING is a list."""
    tag = None
    if timed or L.RECORDER is not None:
        v = conv2d_variant(d)
        if pwx:
            v = v.replace("conv_pw_kernel", "conv_pwx_kernel")
        tag = step_plan.kernel_tag(v, 2.0 * d.n * d.oh * d.ow * d.cout * d.cin * d.kh * d.kw, phase)
    events = None
    if timed and KERNEL_TIMING is not None:
        events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        events[0].record()
    L.call(fn, byref(d), *args, _st())
    if events is not None:
        events[1].record()
        KERNEL_TIMING.append(tag + events)
    if L.RECORDER is not None:
        L.RECORDER.tag_last(tag)


def conv2d(d, x, w_kc, y, bias=None, stats=None):
    _conv_call("ocr_conv2d_f16", d, ptr(x), ptr(w_kc), ptr(bias), ptr(y), ptr(stats),
               phase="dgrad" if d.flip_taps else "fwd", timed=True)


def conv2d_relu_pool(d, x, w_kc, bias, pooled, argmax=None):
    """conv3x3 + bias + ReLU + 2x2/2 max-pool in one kernel (64 -> 64 channels): pooled output (+ first-max positions) only."""
    _conv_call("ocr_conv2d_relu_pool_f16", d, ptr(x), ptr(w_kc), ptr(bias), ptr(pooled), ptr(argmax), phase="fwd", timed=True)


def conv2d_bnred(d, x, w_kc, y, partial, bn_ctx, store_masked=False):
    """Input-gradient conv fused with the BN-backward reduction of the layer below.  store_masked: y receives the
    gradient PAST that layer's ReLU (bias nets: graph.BnCtx.of_bias).  bn_ctx: a graph.BnCtx, or its six fields."""
    c = G.BnCtx(*bn_ctx)
    # (a consumer that cannot recompute conv1_1's y evaluates and stores it now)
    by = c.y.tensor() if isinstance(c.y, LazyFirstY) else c.y
    _conv_call("ocr_conv2d_bnred_f16", d, ptr(x), ptr(w_kc), ptr(y), ptr(partial), ptr(by), ptr(c.scale), ptr(c.shift),
               ptr(c.mean), ptr(c.invstd), c_int(int(c.relu)), c_int(int(store_masked)), phase="dgrad")


class LazyFirstY:
    """conv1_1's raw output y, which the batch-norm training step no longer stores (the statistics pass writes nothing,
    the activation and both readers of y in the backward pass evaluate the 3-channel convolution again): `tensor()`
    evaluates and stores it for a consumer that cannot."""

    def __init__(self, alloc, x4, w_first, shape):
        self.alloc, self.x4, self.w_first, self.shape = alloc, x4, w_first, shape
        self.t = None
        self.moments = None       # f64 [32*32]: the image's patch moments, when the statistics came from them (kept for the backward)

    def tensor(self):
        if self.t is None:
            self.t = self.alloc(self.shape)
            conv2d_first(self.x4, self.w_first, self.t)
        return self.t


def conv2d_bnred_first(d, x, w_kc, y, partial, first_ctx):
    """conv2d_bnred for the consumer of conv1_1's activation with conv1_1's y recomputed from the image instead of read:
    first_ctx = graph.BnCtx.first(): (x4, w_first, scale, shift, mean, invstd, relu)."""
    x4, wf, sc, sh, mu, istd, relu = first_ctx
    _conv_call("ocr_conv2d_bnred_first_f16", d, ptr(x), ptr(w_kc), ptr(y), ptr(partial), ptr(x4), ptr(wf), ptr(sc), ptr(sh),
               ptr(mu), ptr(istd), c_int(int(relu)), phase="dgrad")


def conv2d_bnred_first_wgrad_blocks(d):
    """Number of S1 blocks conv2d_bnred_first_wgrad leaves (one per workgroup); -1 where that launch is unsupported."""
    return int(L._fn("ocr_conv2d_bnred_first_wgrad_blocks", ctypes.c_int)(byref(d)))


def conv2d_bnred_first_wgrad(d, x, w_kc, partial, first_ctx, s1):
    """conv2d_bnred_first that does not store the gradient: `s1` [blocks][32][64] f32 receives the sums conv1_1's weight
    gradient is finished from (conv2d_first_wgrad_sums)."""
    x4, wf, sc, sh, mu, istd, relu = first_ctx
    _conv_call("ocr_conv2d_bnred_first_wgrad_f16", d, ptr(x), ptr(w_kc), ptr(partial), ptr(x4), ptr(wf), ptr(sc), ptr(sh),
               ptr(mu), ptr(istd), c_int(int(relu)), ptr(s1), phase="dgrad")


def conv2d_first_wgrad_sums(s1, moments, w_first, coef, dw):
    """dW of conv1_1 = A .* S1 + B .* (M W) + C .* m (csrc/conv_first.hip: first_wgrad_sums_kernel)."""
    a, b, c = coef
    L.call("ocr_conv2d_first_wgrad_sums_f32", ptr(s1), c_int(s1.shape[0]), ptr(moments), ptr(w_first),
           c_int(dw.shape[-1]), ptr(a), ptr(b), ptr(c), ptr(dw), _st())


def conv2d_bnred_tail(d, x, w_kc, y, partial, tail_ctx, sub_grad=None):
    """Input-gradient conv that completes the gradient of a bottleneck output: stores the gradient past the
    output ReLU and emits the BN-backward sums of the unit's last conv; `sub_grad`: gradient of the output's
    stride-2 subsample, added at the even positions (include/ocr_hip.h).  tail_ctx: a graph.TailCtx, or its fields;
    with `bits` (the output's ReLU mask, one byte per 8 channels) the kernel reads them instead of `out`."""
    t = G.TailCtx(*tail_ctx)
    _conv_call("ocr_conv2d_bnred_tail_f16", d, ptr(x), ptr(w_kc), ptr(y), ptr(partial), ptr(t.y), ptr(t.mean), ptr(t.invstd),
               ptr(t.out), ptr(t.bits), ptr(sub_grad), phase="dgrad")


def conv2d_pw_bnaddrelu(d, prev_y, prev_scale, prev_shift, shortcut, sc_scale, sc_shift, x_out, bits, w_kc, y, stats):
    """1x1 conv whose input x = relu(bn(prev_y) + shortcut) is computed while it is loaded and written to x_out (+ bits)."""
    _conv_call("ocr_conv2d_pw_bnaddrelu_f16", d, ptr(prev_y), ptr(prev_scale), ptr(prev_shift), ptr(shortcut),
               ptr(sc_scale), ptr(sc_shift), ptr(x_out), ptr(bits), ptr(w_kc), ptr(y), ptr(stats), phase="fwd", pwx=True)


def conv2d_pw_bnrelu(d, prev_y, prev_scale, prev_shift, x_out, w_kc, y, stats):
    """1x1 conv whose input x = relu(bn(prev_y)) is computed while it is loaded and written to x_out."""
    _conv_call("ocr_conv2d_pw_bnrelu_f16", d, ptr(prev_y), ptr(prev_scale), ptr(prev_shift), ptr(x_out), ptr(w_kc), ptr(y),
               ptr(stats), phase="fwd", pwx=True)


def conv2d_pw_bnbwd_bnred(d, dz, y_above, coef, dy_out, w_kc, dx, partial, bn_ctx):
    """1x1 input-gradient conv whose operand dy = A*dz + B*y_above + C is computed while it is loaded and written to
    dy_out; fused BN-backward reduction of the layer below as in conv2d_bnred."""
    bn = G.BnCtx(*bn_ctx)
    by = bn.y.tensor() if isinstance(bn.y, LazyFirstY) else bn.y
    a, b, c = coef
    _conv_call("ocr_conv2d_pw_bnbwd_bnred_f16", d, ptr(dz), ptr(y_above), ptr(a), ptr(b), ptr(c), ptr(dy_out), ptr(w_kc),
               ptr(dx), ptr(partial), ptr(by), ptr(bn.scale), ptr(bn.shift), ptr(bn.mean), ptr(bn.invstd),
               c_int(int(bn.relu)), phase="dgrad", pwx=True)


def conv2d_pw_bnbwd_tail(d, dz, y_above, coef, relu_shift, dy_out, w_kc, dx, partial=None, tail_ctx=None, sub_grad=None):
    """conv2d_pw_bnbwd_bnred's loader (+ the ReLU mask of the BN above when relu_shift is given) in front of the plain /
    accumulating (d.flags) / bottleneck-tail epilogue (tail_ctx, sub_grad as conv2d_bnred_tail)."""
    a, b, c = coef
    t = G.TailCtx(*tail_ctx) if tail_ctx is not None else G.TailCtx(None, None, None, None)
    _conv_call("ocr_conv2d_pw_bnbwd_tail_f16", d, ptr(dz), ptr(y_above), ptr(a), ptr(b), ptr(c), ptr(relu_shift), ptr(dy_out),
               ptr(w_kc), ptr(dx), ptr(partial), ptr(t.y), ptr(t.mean), ptr(t.invstd), ptr(t.out), ptr(t.bits), ptr(sub_grad),
               phase="dgrad", pwx=True)


def bn_bwd_sums(partial, T, c, out0, out1, ws):
    """Column sums of fused-reduction partial rows [T][2][c] (kind 0 -> out0, kind 1 -> out1)."""
    stage = ws.get(bn_reduce_workspace(T, c))
    L.call("ocr_bn_bwd_sums", ptr(partial), c_int(T), c_int(c), ptr(out0), ptr(out1), ptr(stage),
           c_size_t(stage.numel()), _st())


def bn_bwd_coefficients(partial, T, c, count, scale, save_mean, save_invstd, dgamma, dbeta, coef, ws):
    stage = ws.get(bn_reduce_workspace(T, c))
    a, b, cc = coef
    L.call("ocr_bn_bwd_coefficients", ptr(partial), c_int(T), c_int(c), c_double(count), ptr(scale), ptr(save_mean),
           ptr(save_invstd), ptr(dgamma), ptr(dbeta), ptr(a), ptr(b), ptr(cc), ptr(stage), c_size_t(stage.numel()), _st())


def bn_relu_bwd_apply(y, scale, shift, save_mean, save_invstd, da_full, relu, partial, T, dgamma, dbeta, dy, ws):
    n, h, w, c = y.shape
    stage = ws.get(bn_reduce_workspace(T, c))
    L.call("ocr_bn_relu_bwd_apply_f16", ptr(y), ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd),
           ptr(da_full), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(partial), c_int(T),
           ptr(dgamma), ptr(dbeta), ptr(dy), ptr(stage), c_size_t(stage.numel()), _st())


# --- guest forms (csrc/guest_bn.hip): <= 56 registers per lane, one launch, placed beside a resident weight-gradient
# workgroup; the recorded step runs them on a second stream (train.TrainStep: tags "pre" / "guest") -------------------
GUEST_BN = os.environ.get("OCR_GUEST_BN", "1") == "1"


def guest_apply_ok(shape):
    """The guest kernels address through 32-bit buffer offsets: tensors < 2 GiB, power-of-two channel chunks."""
    n, h, w, c = shape
    q = c // 4
    return GUEST_BN and c % 8 == 0 and q <= 256 and (q & (q - 1)) == 0 and n * h * w * c * 2 < (1 << 31)


def bn_bwd_coefficients_pre(partial, T, c, count, scale, save_mean, save_invstd, dgamma, dbeta, coef, ws):
    """ocr_bn_bwd_coefficients in front of a guest apply pass: tagged so that the recorded step issues it BEFORE the
    weight gradient the guest runs beside (its finalize workgroups need 72 registers: queued behind a resident
    weight-gradient grid they would hold the guest back for that grid's whole launch)."""
    bn_bwd_coefficients(partial, T, c, count, scale, save_mean, save_invstd, dgamma, dbeta, coef, ws)
    if L.RECORDER is not None:
        L.RECORDER.tag_last(step_plan.pre_tag())


def bn_relu_bwd_apply_affine(y, da, scale, shift, coef_b, coef_c, relu, dy):
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_bwd_apply_affine_f16", ptr(y), ptr(da), ptr(scale), ptr(shift), ptr(coef_b), ptr(coef_c),
           c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(dy), c_int(0), _st())
    if L.RECORDER is not None:
        L.RECORDER.tag_last(step_plan.guest_tag(6.0 * n * h * w * c))           # bytes: y + da read, dy written


def bn_relu_pool_bwd_idx_apply_affine(y, argmax, da_pool, coef, relu, dy):
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_pool_bwd_idx_apply_affine_f16", ptr(y), ptr(argmax), ptr(da_pool), ptr(coef[0]), ptr(coef[1]),
           ptr(coef[2]), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(dy), c_int(0), _st())
    if L.RECORDER is not None:
        L.RECORDER.tag_last(step_plan.guest_tag(4.75 * n * h * w * c))          # y read + dy written + the pooled gradient and index


def conv2d_wgrad_variant(d):
    """What the weight gradient of `d` launches (ocr_conv2d_wgrad_variant): a dict with `kernel` (the slab kernel's
    instantiation), `slabs`, `grid`, `xcd` (ints) and `reduce` (the slab sum's instantiation).  Raises OcrHipError with
    the status ocr_conv2d_wgrad_f16 would give where no kernel family takes the shape."""
    buf = ctypes.create_string_buffer(128)
    L.call_int("ocr_conv2d_wgrad_variant", byref(d), buf, c_size_t(128))
    kernel, *fields = buf.value.decode().split(" ")
    v = dict(f.split("=", 1) for f in fields)
    return {"kernel": kernel, "slabs": int(v["slabs"]), "grid": int(v["grid"]), "xcd": int(v["xcd"]), "reduce": v["reduce"]}


def conv2d_wgrad(d, x, dy, dw, ws, alloc=None):
    """alloc (callable: nbytes -> uint8 tensor; layers pass Graph.empty while OCR_GUEST_BN is on): the slabs get a
    buffer of their own and the call is issued as its two halves — slab kernel ["side", FLOP], slab sum ["reduce"] —
    so that the recorded step can run the first as the host of a guest pass and the second behind the join
    (train.schedule_guests).  Same numbers either way."""
    nbytes = L.call_size("ocr_conv2d_wgrad_workspace", byref(d))
    flops = 2.0 * d.n * d.oh * d.ow * d.cout * d.cin * d.kh * d.kw
    if alloc is not None and GUEST_BN:
        buf = alloc(nbytes)
        L.call("ocr_conv2d_wgrad_slabs_f16", byref(d), ptr(x), ptr(dy), ptr(buf), c_size_t(nbytes), _st())
        if L.RECORDER is not None:
            # a host only if a guest's 56 registers per lane fit beside it (a kernel that fills the file would
            # time-slice with the guest); otherwise it stays where it was recorded
            room = L.call_int("ocr_conv2d_wgrad_guest_room", byref(d))
            L.RECORDER.tag_last(step_plan.side_tag(flops if room >= 56 else None))
        L.call("ocr_conv2d_wgrad_reduce_f32", byref(d), ptr(buf), ptr(dw), _st())
        if L.RECORDER is not None:
            L.RECORDER.tag_last(step_plan.reduce_tag())
        return
    buf = ws.get(nbytes)
    L.call("ocr_conv2d_wgrad_f16", byref(d), ptr(x), ptr(dy), ptr(dw), ptr(buf), c_size_t(nbytes), _st())
    if L.RECORDER is not None:
        # (the one-call form shares the tower's slab workspace with the next weight gradient: it stays where it was
        # recorded — train.schedule_guests holds back only the split form above)
        L.RECORDER.tag_last(step_plan.side_tag())


def space_to_depth(x, xs):
    n, h, w, c = x.shape
    L.call("ocr_space_to_depth_f16", ptr(x), c_int(n), c_int(h), c_int(w), c_int(c), ptr(xs), _st())


def depth_to_space(xs, x, accumulate):
    n, h, w, c = x.shape
    L.call("ocr_depth_to_space_f16", ptr(xs), c_int(n), c_int(h), c_int(w), c_int(c), ptr(x), c_int(int(accumulate)), _st())


def weights_s2d(w33, w22):
    _, _, cin, cout = w33.shape
    L.call("ocr_weights_s2d_f32", ptr(w33), c_int(cin), c_int(cout), ptr(w22), _st())


def weights_s2d_grad(dw22, dw33):
    _, _, cin, cout = dw33.shape
    L.call("ocr_weights_s2d_grad_f32", ptr(dw22), c_int(cin), c_int(cout), ptr(dw33), _st())
    if L.RECORDER is not None:
        L.RECORDER.tag_last(step_plan.side_tag())      # reads what the weight-gradient launch before it wrote: same stream


def conv2d_first_num_mtiles(n, h, w):
    return L.call_int("ocr_conv2d_first_num_mtiles", c_int(n), c_int(h), c_int(w))


def conv2d_first(x4, w_first, y, flags=0, bias=None, stats=None, cout=None):
    """y = None with CONV_STATS: a statistics-only launch (pass `cout`)."""
    n, h, w, _ = x4.shape
    cout = y.shape[-1] if y is not None else cout
    L.call("ocr_conv2d_first_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(w_first),
           ptr(bias), c_int(flags), ptr(y), ptr(stats), _st())


def conv2d_first_moments(x4, w_first, row, cout, ws, moments=None):
    """conv1_1's batch-norm statistics (sum y, sum y^2 per channel -> row [1][2][cout] f32, any byte buffer) from the
    image's second moments; `moments` (f64 [32][32]) keeps them for conv2d_first_wgrad_sums."""
    n, h, w, _ = x4.shape
    nbytes = L.call_size("ocr_conv2d_first_moments_workspace")
    buf = ws.get(nbytes)
    L.call("ocr_conv2d_first_moments_keep_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(w_first),
           ptr(row), ptr(moments), ptr(buf), c_size_t(nbytes), _st())


def conv2d_first_wgrad(x4, dy, dw, ws):
    n, h, w, _ = x4.shape
    cout = dy.shape[-1]
    nbytes = L.call_size("ocr_conv2d_first_wgrad_workspace", c_int(n), c_int(h), c_int(w), c_int(cout))
    buf = ws.get(nbytes)
    L.call("ocr_conv2d_first_wgrad_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(dy),
           ptr(dw), ptr(buf), c_size_t(nbytes), _st())


def conv2d_first_wgrad_bn(x4, da, y, shift, coef, relu, dw, ws, w_first=None):
    """conv1_1's weight gradient with its BN-backward apply computed on load (coef: bn_bwd_coefficients); with
    `w_first` y is recomputed from the image instead of read."""
    n, h, w, _ = x4.shape
    cout = da.shape[-1]
    nbytes = L.call_size("ocr_conv2d_first_wgrad_workspace", c_int(n), c_int(h), c_int(w), c_int(cout))
    buf = ws.get(nbytes)
    a, b, c = coef
    L.call("ocr_conv2d_first_wgrad_bn_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(da),
           ptr(None if w_first is not None else y), ptr(w_first), ptr(shift), ptr(a), ptr(b), ptr(c), c_int(int(relu)),
           ptr(dw), ptr(buf), c_size_t(nbytes), _st())


def conv2d_first_bn_relu(x4, w_first, scale, shift, relu, a):
    """conv1_1's activation relu(bn(conv(x))) with the convolution evaluated again (second pass; the statistics exist)."""
    n, h, w, _ = x4.shape
    L.call("ocr_conv2d_first_bn_relu_f16", c_int(n), c_int(h), c_int(w), c_int(a.shape[-1]), ptr(x4), ptr(w_first),
           ptr(scale), ptr(shift), c_int(int(relu)), ptr(a), _st())


def conv2d_stem_num_mtiles(n, h, w):
    return L.call_int("ocr_conv2d_stem_num_mtiles", c_int(n), c_int(h), c_int(w))


def conv2d_stem(x4, w_stem, y, flags=0, bias=None, stats=None):
    n, h, w, _ = x4.shape
    L.call("ocr_conv2d_stem_f16", c_int(n), c_int(h), c_int(w), c_int(y.shape[-1]), ptr(x4), ptr(w_stem),
           ptr(bias), c_int(flags), ptr(y), ptr(stats), _st())


def conv2d_stem_wgrad(x4, dy, dw, ws):
    n, h, w, _ = x4.shape
    cout = dy.shape[-1]
    nbytes = L.call_size("ocr_conv2d_stem_wgrad_workspace", c_int(n), c_int(h), c_int(w), c_int(cout))
    buf = ws.get(nbytes)
    L.call("ocr_conv2d_stem_wgrad_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(dy), ptr(dw),
           ptr(buf), c_size_t(nbytes), _st())


def conv2d_stem_wgrad_bn(x4, da, y, shift, coef, relu, dw, ws):
    """The root convolution's weight gradient with its BN-backward apply computed on load (coef: bn_relu_bwd_reduce)."""
    n, h, w, _ = x4.shape
    cout = da.shape[-1]
    nbytes = L.call_size("ocr_conv2d_stem_wgrad_workspace", c_int(n), c_int(h), c_int(w), c_int(cout))
    buf = ws.get(nbytes)
    a, b, c = coef
    L.call("ocr_conv2d_stem_wgrad_bn_f16", c_int(n), c_int(h), c_int(w), c_int(cout), ptr(x4), ptr(da), ptr(y),
           ptr(shift), ptr(a), ptr(b), ptr(c), c_int(int(relu)), ptr(dw), ptr(buf), c_size_t(nbytes), _st())


def bn_relu_bwd_reduce(y, scale, shift, save_mean, save_invstd, da_full, relu, dgamma, dbeta, coef, ws, da_pool=None):
    """Reduction + finalize of the BN backward, the apply step returned as coefficients (dy = A*dz + B*y + C).
    da_pool: the gradient of the layer's 2x2/2 max-pool, routed to each window's first maximum."""
    n, h, w, c = y.shape
    T = bn_bwd_num_partials(y.shape, 2 if da_pool is not None else 0)
    part, stage = ws.two(T * 2 * c * 4, bn_reduce_workspace(T, c))
    a, b, cc = coef
    L.call("ocr_bn_relu_bwd_reduce_f16", ptr(y), ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd), ptr(da_full),
           ptr(da_pool), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(dgamma), ptr(dbeta), ptr(a), ptr(b),
           ptr(cc), ptr(part), ptr(stage), c_size_t(stage.numel()), _st())


def bn_relu_bwd_reduce_rows(y, da_full, scale, shift, save_mean, save_invstd, relu, alloc, da_pool=None, argmax=None):
    """Guest reduction pass of an end-point layer's BN backward (csrc/guest_bn.hip): returns (partial rows, T) for
    bn_bwd_coefficients_pre.  alloc: shape, dtype -> tensor (the rows outlive the call: the recorded step runs the
    finalize later)."""
    n, h, w, c = y.shape
    pooled = int(da_pool is not None)
    T = L.call_int("ocr_bn_relu_bwd_reduce_rows_count", c_int(n), c_int(h), c_int(w), c_int(c), c_int(pooled), c_int(0))
    part = alloc((T, 2, c), torch.float32)
    L.call("ocr_bn_relu_bwd_reduce_rows_f16", ptr(y), ptr(da_full), ptr(da_pool), ptr(argmax), ptr(scale), ptr(shift),
           ptr(save_mean), ptr(save_invstd), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(part), c_int(0),
           _st())
    if L.RECORDER is not None:
        # (its grid is one workgroup per CU wherever it runs: the row count must not depend on the placement)
        L.RECORDER.tag_last(step_plan.guest_tag((4.0 if not pooled else 4.75) * n * h * w * c, as_is=True))
    return part, T


def bn_relu_poolfull_bwd_apply_affine(y, da_full, da_pool, argmax, scale, shift, coef, relu, dy):
    """Guest apply pass of a pooled end-point layer (csrc/guest_bn.hip): dz = (da_full + routed da_pool) * ReLU mask."""
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_poolfull_bwd_apply_affine_f16", ptr(y), ptr(da_full), ptr(da_pool), ptr(argmax), ptr(scale), ptr(shift),
           ptr(coef[1]), ptr(coef[2]), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(dy), c_int(0), _st())
    if L.RECORDER is not None:
        L.RECORDER.tag_last(step_plan.guest_tag(6.75 * n * h * w * c))          # y + da_full read, dy written, pooled gradient + index


def bn_relu_bwd_reduce_pooled(y, scale, shift, save_mean, save_invstd, pooled, relu, da_out, dgamma, dbeta, coef, ws):
    """bn_relu_bwd_reduce with the max-pool backward that produces the activation gradient folded in.
    pooled: a graph.PoolGrad (grad [n,oh,ow,c], argmax u8, k, stride, (pad_top, pad_left)); da_out (nullable): the gathered
    gradient."""
    n, h, w, c = y.shape
    dap, argmax, k, stride, (pt, pl) = pooled
    T = bn_bwd_num_partials(y.shape, 0)
    part, stage = ws.two(T * 2 * c * 4, bn_reduce_workspace(T, c))
    a, b, cc = coef
    L.call("ocr_bn_relu_bwd_reduce_pooled_f16", ptr(y), ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd), ptr(dap),
           ptr(argmax), c_int(n), c_int(h), c_int(w), c_int(c), c_int(k), c_int(stride), c_int(pt), c_int(pl),
           c_int(dap.shape[1]), c_int(dap.shape[2]), c_int(int(relu)), ptr(da_out), ptr(dgamma), ptr(dbeta), ptr(a), ptr(b),
           ptr(cc), ptr(part), ptr(stage), c_size_t(stage.numel()), _st())


def pack_weights_stem(w_hwio, w_stem):
    L.call("ocr_pack_weights_stem_f16", ptr(w_hwio), c_int(w_hwio.shape[-1]), ptr(w_stem), _st())


def pack_weights_first(w_hwio, w_first):
    L.call("ocr_pack_weights_first_f16", ptr(w_hwio), c_int(w_hwio.shape[-1]), ptr(w_first), _st())


def pack_weights(w_hwio, w_kc=None, w_ck=None):
    kh, kw, cin, cout = w_hwio.shape
    L.call("ocr_pack_weights_f16", ptr(w_hwio), c_int(kh * kw), c_int(cin), c_int(cout), ptr(w_kc),
           ptr(w_ck), _st())


class PackBatch:
    """Device table for ocr_pack_weights_batch_f16: built once for a list of (w_hwio f32, w_kc, w_ck[, ld_ck]) tensors
    (ld_ck = 32: a fuse head's [32][cin] / [cin][32] zero-padded pair; w then is the [cin][C] master)."""

    def __init__(self, entries, device):
        n = len(entries)
        vp = ctypes.c_void_p * n
        ci = ctypes.c_int * n
        ent = [(e + (0,))[:4] for e in entries]
        shp = [tuple(w.shape) if w.dim() == 4 else (1, 1) + tuple(w.shape) for w, _, _, _ in ent]
        ws = vp(*[w.data_ptr() for w, _, _, _ in ent])
        kc = vp(*[(a.data_ptr() if a is not None else None) for _, a, _, _ in ent])
        ck = vp(*[(b.data_ptr() if b is not None else None) for _, _, b, _ in ent])
        taps = ci(*[s[0] * s[1] for s in shp])
        cin = ci(*[s[2] for s in shp])
        cout = ci(*[s[3] for s in shp])
        ld = ci(*[l for _, _, _, l in ent])
        nbytes = L.call_size("ocr_pack_weights_batch_table_bytes", c_int(n))
        host = torch.empty(nbytes, dtype=torch.uint8)
        grid = ctypes.c_int(0)
        L.call("ocr_pack_weights_batch_table", c_int(n), ws, taps, cin, cout, kc, ck, ld, ctypes.c_void_p(host.data_ptr()),
               ctypes.byref(grid))
        self.table = host.to(device)
        self.n, self.grid = n, grid.value
        self.keep = entries                      # the tensors the table points at

    def run(self):
        L.call("ocr_pack_weights_batch_f16", ptr(self.table), c_int(self.n), c_int(self.grid), _st())


def pack_weights_small(w, w_kc32, w_ck32):
    cin, cout = w.shape
    L.call("ocr_pack_weights_small_f16", ptr(w), c_int(cin), c_int(cout), ptr(w_kc32), ptr(w_ck32), _st())


# ------------------------------------------------------------------- image / BN / pool
def prep_images(images_f32, out_f16x4, means=(123.68, 116.78, 103.94), div=1.0):
    npix = images_f32.numel() // 3
    L.call("ocr_prep_images_norm_f16", ptr(images_f32), c_int64(npix), c_float(means[0]),
           c_float(means[1]), c_float(means[2]), c_float(div), ptr(out_f16x4), _st())


def sum_squares(x, scale, out, ws):
    """out[0] = scale * sum(x^2) (f64 accumulation, fixed order)."""
    n = x.numel()
    nbytes = L.call_size("ocr_sum_squares_workspace", c_int64(n))
    buf = ws.get(nbytes)
    L.call("ocr_sum_squares_f32", ptr(x), c_int64(n), c_float(scale), ptr(out), ptr(buf), c_size_t(nbytes), _st())


def bn_finalize(partial, T, C, count, gamma, beta, eps, decay, moving_mean, moving_var, scale, shift,
                save_mean, save_invstd, ws):
    nbytes = L.call_size("ocr_bn_reduce_workspace", c_int(T), c_int(C))
    buf = ws
    L.call("ocr_bn_finalize", ptr(partial), c_int(T), c_int(C), c_double(count), ptr(gamma), ptr(beta),
           c_float(eps), c_float(decay), ptr(moving_mean), ptr(moving_var), ptr(scale), ptr(shift),
           ptr(save_mean), ptr(save_invstd), ptr(buf), c_size_t(buf.numel() * buf.element_size()), _st())
    return nbytes


def bn_reduce_workspace(T, C):
    return L.call_size("ocr_bn_reduce_workspace", c_int(T), c_int(C))


def bn_inference_params(gamma, beta, mm, mv, eps, scale, shift):
    L.call("ocr_bn_inference_params", ptr(gamma), ptr(beta), ptr(mm), ptr(mv), c_float(eps),
           c_int(mm.numel()), ptr(scale), ptr(shift), _st())


def bn_relu(y, scale, shift, relu, pool, a_full=None, a_pool=None):
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_f16", ptr(y), ptr(scale), ptr(shift), c_int(n), c_int(h), c_int(w), c_int(c),
           c_int(int(relu)), c_int(pool), ptr(a_full), ptr(a_pool), _st())


def bn_relu_pool_idx(y, scale, shift, relu, a_full, a_pool, argmax, y_pool=None):
    """bn+ReLU+2x2 max-pool that also stores the first-max position (uint8 [n,oh,ow,c]) and, with `y_pool`, the conv
    output AT that position (the BN-backward operand of the pooled positions: bn_relu_pool_bwd_idx_apply)."""
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_pool_idx_f16", ptr(y), ptr(scale), ptr(shift), c_int(n), c_int(h), c_int(w), c_int(c),
           c_int(int(relu)), ptr(a_full), ptr(a_pool), ptr(argmax), ptr(y_pool), _st())


def bn_relu_pool_bwd_idx_apply(y, scale, save_mean, save_invstd, argmax, da_pool, relu, partial, T, dgamma, dbeta, dy, ws):
    """bn_relu_pool_bwd_idx without its reduction pass: `partial` [T][2][c] from the input-gradient kernel that wrote
    da_pool (conv2d_bnred with bn_y = y_pool)."""
    n, h, w, c = y.shape
    stage = ws.get(bn_reduce_workspace(T, c))
    L.call("ocr_bn_relu_pool_bwd_idx_apply_f16", ptr(y), ptr(scale), ptr(save_mean), ptr(save_invstd), ptr(argmax),
           ptr(da_pool), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(partial), c_int(T), ptr(dgamma),
           ptr(dbeta), ptr(dy), ptr(stage), c_size_t(stage.numel()), _st())


def bn_relu_pool_bwd_idx(y, scale, save_mean, save_invstd, a_pool, argmax, da_pool, relu, dgamma, dbeta, dy, ws):
    n, h, w, c = y.shape
    T = bn_bwd_num_partials(y.shape, 2)
    part, stage = ws.two(T * 2 * c * 4, bn_reduce_workspace(T, c))
    L.call("ocr_bn_relu_pool_bwd_idx_f16", ptr(y), ptr(scale), ptr(save_mean), ptr(save_invstd), ptr(a_pool),
           ptr(argmax), ptr(da_pool), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)), ptr(dgamma),
           ptr(dbeta), ptr(dy), ptr(part), ptr(stage), c_size_t(stage.numel()), _st())


def bn_bwd_num_partials(shape, pool):
    n, h, w, c = shape
    return L.call_int("ocr_bn_bwd_num_partials", c_int(n), c_int(h), c_int(w), c_int(c), c_int(pool))


def bn_relu_bwd(y, scale, shift, save_mean, save_invstd, da_full, da_pool, relu, pool, dgamma, dbeta,
                dy, ws):
    n, h, w, c = y.shape
    T = bn_bwd_num_partials(y.shape, pool)
    part, stage = ws.two(T * 2 * c * 4, bn_reduce_workspace(T, c))
    L.call("ocr_bn_relu_bwd_f16", ptr(y), ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd),
           ptr(da_full), ptr(da_pool), c_int(n), c_int(h), c_int(w), c_int(c), c_int(int(relu)),
           c_int(pool), ptr(dgamma), ptr(dbeta), ptr(dy), ptr(part), ptr(stage),
           c_size_t(stage.numel()), _st())


def channel_stats_num_partials(npix, c):
    return L.call_int("ocr_channel_stats_num_partials", c_int64(npix), c_int(c))


def channel_stats(x, partial):
    c = x.shape[-1]
    L.call("ocr_channel_stats_f16", ptr(x), c_int64(x.numel() // c), c_int(c), ptr(partial), _st())


def bn_add_relu(y, scale, shift, shortcut, out, sc_scale=None, sc_shift=None, bits=None):
    """out = relu(bn(y) + shortcut); sc_scale/sc_shift: the shortcut's own (projection) batch norm applied on the fly;
    bits: optional ReLU-mask bytes (one per 8 channels)."""
    c = y.shape[-1]
    L.call("ocr_bn_add_relu_f16", ptr(y), ptr(scale), ptr(shift), ptr(shortcut), ptr(sc_scale), ptr(sc_shift),
           c_int64(y.numel() // c), c_int(c), ptr(out), ptr(bits), _st())


def relu_bwd(out, dout, dz):
    L.call("ocr_relu_bwd_f16", ptr(out), ptr(dout), c_int64(out.numel()), ptr(dz), _st())


def add_inplace(a, b):
    L.call("ocr_add_inplace_f16", ptr(a), ptr(b), c_int64(a.numel()), _st())


def unpool_f16(x, y):
    n, lh, lw, c = x.shape
    L.call("ocr_unpool_f16", ptr(x), c_int(n), c_int(lh), c_int(lw), c_int(c), ptr(y), _st())


def unpool_bwd_f16(dy, dx, accumulate):
    n, lh, lw, c = dx.shape
    L.call("ocr_unpool_bwd_f16", ptr(dy), c_int(n), c_int(lh), c_int(lw), c_int(c), ptr(dx),
           c_int(int(accumulate)), _st())


def sc_sigmoid_split(z, c0, out0, out1):
    C = z.shape[-1]
    L.call("ocr_sc_sigmoid_split", ptr(z), c_int(z.numel() // C), c_int(C), c_int(c0), ptr(out0), ptr(out1), _st())


def sc_sigmoid_split_bwd(out0, dout0, out1, dout1, dz):
    C = dz.shape[-1]
    L.call("ocr_sc_sigmoid_split_bwd", ptr(out0), ptr(dout0), ptr(out1), ptr(dout1), c_int(dz.numel() // C), c_int(C),
           c_int(out0.shape[-1]), ptr(dz), _st())


def unpool_add_stats(t_low, y, partial):
    """y += unpool(t_low) in place; partial (nullable): [channel_stats_num_partials(y pixels, c)][2][c] f32."""
    n, lh, lw, c = t_low.shape
    L.call("ocr_unpool_add_stats_f16", ptr(t_low), c_int(n), c_int(lh), c_int(lw), c_int(c), ptr(y), ptr(partial), _st())


def sc_sigmoid(z, out):
    L.call("ocr_sc_sigmoid", ptr(z), c_int64(z.numel()), ptr(out), _st())


def sc_sigmoid_bwd(out, dout, dz):
    L.call("ocr_sc_sigmoid_bwd", ptr(out), ptr(dout), c_int64(out.numel()), ptr(dz), _st())


def bias_relu_bwd(a, da, relu, dz, dbias, ws):
    c = a.shape[-1]
    npix = a.numel() // c
    T = L.call_int("ocr_bias_relu_bwd_num_partials", c_int64(npix), c_int(c))
    buf = ws.get(T * c * 4)
    L.call("ocr_bias_relu_bwd_f16", ptr(a), ptr(da), c_int64(npix), c_int(c), c_int(int(relu)), ptr(dz),
           ptr(dbias), ptr(buf), _st())


def sc_colsum(x, C, out, ws):
    P = x.numel() // C
    T = sc_num_partials(P, C)
    buf = ws.get((T + 1) * 2 * C * 4)
    L.call("ocr_sc_colsum", ptr(x), c_int(P), c_int(C), ptr(out), ptr(buf), _st())


def maxpool(x, k, stride, pad, y, argmax=None):
    n, h, w, c = x.shape
    _, oh, ow, _ = y.shape
    L.call("ocr_maxpool_f16", ptr(x), c_int(n), c_int(h), c_int(w), c_int(c), c_int(k), c_int(stride),
           c_int(pad[0]), c_int(pad[1]), c_int(oh), c_int(ow), ptr(y), ptr(argmax), _st())


def bn_relu_maxpool(bn_y, scale, shift, relu, k, stride, pad, y, argmax=None):
    """max-pool over relu(bn(bn_y)) computed on the fly from the raw conv output."""
    n, h, w, c = bn_y.shape
    _, oh, ow, _ = y.shape
    L.call("ocr_bn_relu_maxpool_f16", ptr(bn_y), ptr(scale), ptr(shift), c_int(int(relu)), c_int(n), c_int(h), c_int(w),
           c_int(c), c_int(k), c_int(stride), c_int(pad[0]), c_int(pad[1]), c_int(oh), c_int(ow), ptr(y), ptr(argmax), _st())


def maxpool_bwd(x, dy, k, stride, pad, dx, accumulate, argmax=None, in_shape=None):
    """Either `x` (arg-max re-derived) or the forward pass's `argmax` index tensor."""
    n, h, w, c = in_shape if in_shape is not None else x.shape
    _, oh, ow, _ = dy.shape
    L.call("ocr_maxpool_bwd_f16", ptr(None if argmax is not None else x), ptr(argmax), ptr(dy), c_int(n),
           c_int(h), c_int(w), c_int(c), c_int(k), c_int(stride), c_int(pad[0]), c_int(pad[1]), c_int(oh),
           c_int(ow), ptr(dx), c_int(int(accumulate)), _st())


# ------------------------------------------------------------------------------ heads
def conv1x1_small(x, w_kc32, cout, out, bias=None):
    P = x.numel() // x.shape[-1]
    L.call("ocr_conv1x1_small_f16", ptr(x), ptr(w_kc32), ptr(bias), c_int(P), c_int(x.shape[-1]),
           c_int(cout), ptr(out), _st())


def conv1x1_small_dgrad(dz, w_ck32, cout, dx, accumulate, grad_scale=1.0):
    P = dx.numel() // dx.shape[-1]
    L.call("ocr_conv1x1_small_dgrad_f16", ptr(dz), ptr(w_ck32), c_int(P), c_int(dx.shape[-1]),
           c_int(cout), c_float(grad_scale), ptr(dx), c_int(int(accumulate)), _st())


def conv1x1_small_wgrad(x, dz, cout, dw, ws):
    cin = x.shape[-1]
    P = x.numel() // cin
    nbytes = L.call_size("ocr_conv1x1_small_wgrad_workspace", c_int(P), c_int(cin), c_int(cout))
    buf = ws.get(nbytes)
    L.call("ocr_conv1x1_small_wgrad_f16", ptr(x), ptr(dz), c_int(P), c_int(cin), c_int(cout), ptr(dw),
           ptr(buf), c_size_t(nbytes), _st())


def sc_num_partials(P, C):
    return L.call_int("ocr_sc_num_partials", c_int(P), c_int(C))


def sc_stats(x, C, partial):
    P = x.numel() // C
    L.call("ocr_sc_stats", ptr(x), c_int(P), c_int(C), ptr(partial), _st())


def sc_fuse(out, za=None, sa=None, ha=None, zb=None, sb=None, hb=None, prev=None, relu=True):
    n, h, w, C = out.shape
    L.call("ocr_sc_fuse", ptr(za), ptr(sa), ptr(ha), ptr(zb), ptr(sb), ptr(hb), ptr(prev), c_int(n),
           c_int(h), c_int(w), c_int(C), c_int(int(relu)), ptr(out), _st())


def sc_unpool_bwd(dout, dprev):
    n, lh, lw, C = dprev.shape
    L.call("ocr_sc_unpool_bwd", ptr(dout), c_int(n), c_int(lh), c_int(lw), c_int(C), ptr(dprev), _st())


def sc_bn_bwd(z, scale, shift, save_mean, save_invstd, dout, relu, dgamma, dbeta, dz, ws):
    C = z.shape[-1]
    P = z.numel() // C
    T = sc_num_partials(P, C)
    buf = ws.get((T + 1) * 2 * C * 4)
    L.call("ocr_sc_bn_bwd", ptr(z), ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd), ptr(dout),
           c_int(P), c_int(C), c_int(int(relu)), ptr(dgamma), ptr(dbeta), ptr(dz), ptr(buf), _st())


def sc_pointwise_fwd(x, xo, cin, w, out, oo, cout, bias=None):
    ldx, ldo = x.shape[-1], out.shape[-1]
    P = x.numel() // ldx
    L.call("ocr_sc_pointwise_fwd", ptr(x), c_int(ldx), c_int(xo), c_int(cin), ptr(w), ptr(bias), c_int(P),
           ptr(out), c_int(ldo), c_int(oo), c_int(cout), _st())


def sc_pointwise_dgrad(dout, oo, cout, w, dx, xo, cin):
    ldx, ldo = dx.shape[-1], dout.shape[-1]
    P = dx.numel() // ldx
    L.call("ocr_sc_pointwise_dgrad", ptr(dout), c_int(ldo), c_int(oo), c_int(cout), ptr(w), c_int(P),
           ptr(dx), c_int(ldx), c_int(xo), c_int(cin), _st())


def sc_pointwise_wgrad(x, xo, cin, dout, oo, cout, dw, db, ws):
    ldx, ldo = x.shape[-1], dout.shape[-1]
    P = x.numel() // ldx
    nbytes = L.call_size("ocr_sc_pointwise_wgrad_workspace", c_int(cin), c_int(cout))
    buf = ws.get(nbytes)
    L.call("ocr_sc_pointwise_wgrad", ptr(x), c_int(ldx), c_int(xo), c_int(cin), ptr(dout), c_int(ldo),
           c_int(oo), c_int(cout), c_int(P), ptr(dw), ptr(db), ptr(buf), c_size_t(nbytes), _st())


# ------------------------------------------------------------------------------- loss
def dice_loss_fwd(yt_pixel, yp_pixel, yt_link, yp_link, mask, sums27, loss10, ws):
    P = mask.numel()
    pc = yp_pixel.numel() // P
    G = yp_link.numel() // (8 * P)
    nbytes = L.call_size("ocr_dice_workspace", c_int(P))
    buf = ws.get(nbytes)
    L.call("ocr_dice_loss_fwd", ptr(yt_pixel), ptr(yp_pixel), c_int(pc), ptr(yt_link), ptr(yp_link),
           c_int(G), ptr(mask), c_int(P), ptr(sums27), ptr(loss10), ptr(buf), c_size_t(nbytes), _st())


def dice_loss_bwd(yt_pixel, yt_link, mask, sums27, grad_scale, d_pixel, d_link):
    P = mask.numel()
    pc = d_pixel.numel() // P
    G = d_link.numel() // (8 * P)
    L.call("ocr_dice_loss_bwd", ptr(yt_pixel), c_int(pc), ptr(yt_link), c_int(G), ptr(mask), c_int(P),
           ptr(sums27), c_float(grad_scale), ptr(d_pixel), ptr(d_link), _st())


def dice_loss_bwd_dyn(yt_pixel, yt_link, mask, sums27, grad_scale, loss_scale, d_pixel, d_link):
    """dice_loss_bwd with the seed grad_scale * loss_scale[0], `loss_scale` a DEVICE f32 (LossScaleState.scale_ptr)."""
    P = mask.numel()
    pc = d_pixel.numel() // P
    G = d_link.numel() // (8 * P)
    L.call("ocr_dice_loss_bwd_dyn", ptr(yt_pixel), c_int(pc), ptr(yt_link), c_int(G), ptr(mask), c_int(P),
           ptr(sums27), c_float(grad_scale), ptr(loss_scale), ptr(d_pixel), ptr(d_link), _st())


def softmax_loss_fwd(desc, pixel_logits, link_logits, pixel_labels, link_labels, thr, sums34, loss10, ws):
    nbytes = L.call_size("ocr_softmax_loss_workspace", byref(desc))
    buf = ws.get(nbytes)
    L.call("ocr_softmax_loss_fwd", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(thr), ptr(sums34), ptr(loss10), ptr(buf), c_size_t(nbytes), _st())


def softmax_loss_selected(desc, pixel_logits, pixel_labels, thr, mask_u8):
    L.call("ocr_softmax_loss_selected", byref(desc), ptr(pixel_logits), ptr(pixel_labels), ptr(thr), ptr(mask_u8), _st())


def softmax_loss_bwd(desc, pixel_logits, link_logits, pixel_labels, link_labels, thr, sums34, grad_scale,
                     d_pixel, d_link):
    L.call("ocr_softmax_loss_bwd", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(thr), ptr(sums34), c_float(grad_scale), ptr(d_pixel), ptr(d_link), _st())


def softmax_loss_bwd_dyn(desc, pixel_logits, link_logits, pixel_labels, link_labels, thr, sums34, grad_scale, loss_scale,
                         d_pixel, d_link):
    L.call("ocr_softmax_loss_bwd_dyn", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(thr), ptr(sums34), c_float(grad_scale), ptr(loss_scale), ptr(d_pixel), ptr(d_link), _st())


def _balanced_check(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights):
    px = desc.n * desc.hw
    if pixel_logits.numel() != 2 * px or pixel_labels.numel() != px or pixel_weights.numel() != px or \
            (link_logits is not None and (link_logits.numel() != 16 * px or link_labels.numel() != 8 * px)):
        raise ValueError("balanced loss: tensors do not match n * hw = %d" % px)


def balanced_loss_fwd(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights, thr, sums34, loss10, ws):
    """PixelLink's instance-balanced loss (include/ocr_hip.h: ocr_balanced_loss_fwd); pixel_weights f32 [n, hw]."""
    _balanced_check(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights)
    nbytes = L.call_size("ocr_balanced_loss_workspace", byref(desc))
    buf = ws.get(nbytes)
    L.call("ocr_balanced_loss_fwd", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(pixel_weights), ptr(thr), ptr(sums34), ptr(loss10), ptr(buf), c_size_t(nbytes), _st())


def balanced_loss_selected(desc, pixel_logits, pixel_labels, pixel_weights, thr, mask_u8):
    _balanced_check(desc, pixel_logits, None, pixel_labels, None, pixel_weights)
    L.call("ocr_balanced_loss_selected", byref(desc), ptr(pixel_logits), ptr(pixel_labels), ptr(pixel_weights), ptr(thr),
           ptr(mask_u8), _st())


def balanced_loss_bwd(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights, thr, sums34, grad_scale,
                      d_pixel, d_link):
    _balanced_check(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights)
    L.call("ocr_balanced_loss_bwd", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(pixel_weights), ptr(thr), ptr(sums34), c_float(grad_scale), ptr(d_pixel), ptr(d_link),
           _st())


def balanced_loss_bwd_dyn(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights, thr, sums34,
                          grad_scale, loss_scale, d_pixel, d_link):
    """balanced_loss_bwd with the seed grad_scale * loss_scale[0], `loss_scale` a DEVICE f32 (LossScaleState.scale_ptr)."""
    _balanced_check(desc, pixel_logits, link_logits, pixel_labels, link_labels, pixel_weights)
    L.call("ocr_balanced_loss_bwd_dyn", byref(desc), ptr(pixel_logits), ptr(link_logits), ptr(pixel_labels),
           ptr(link_labels), ptr(pixel_weights), ptr(thr), ptr(sums34), c_float(grad_scale), ptr(loss_scale),
           ptr(d_pixel), ptr(d_link), _st())


# ------------------------------------------------------------------ heads, batched (one launch per kernel kind)
def _struct(name, fields):
    return type(name, (ctypes.Structure,), {"_fields_": fields})


_VP, _I32 = ctypes.c_void_p, ctypes.c_int32
HeadConvItem = _struct("HeadConvItem", [("x", _VP), ("w_kc32", _VP), ("bias", _VP), ("out", _VP), ("stats_partial", _VP),
                                        ("P", _I32), ("cin", _I32), ("cout", _I32)])
HeadDgradItem = _struct("HeadDgradItem", [("dz", _VP), ("w_ck32", _VP), ("dx", _VP), ("P", _I32), ("cin", _I32),
                                          ("cout", _I32), ("accumulate", _I32)])
HeadWgradItem = _struct("HeadWgradItem", [("x", _VP), ("dz", _VP), ("dw", _VP), ("slab", _VP), ("P", _I32), ("cin", _I32),
                                          ("cout", _I32)])
BnFinalizeItem = _struct("BnFinalizeItem", [("partial", _VP), ("T", _I32), ("C", _I32), ("count", c_double), ("gamma", _VP),
                                            ("beta", _VP), ("moving_mean", _VP), ("moving_var", _VP), ("scale", _VP),
                                            ("shift", _VP), ("save_mean", _VP), ("save_invstd", _VP)])
ScBnBwdItem = _struct("ScBnBwdItem", [("z", _VP), ("scale", _VP), ("shift", _VP), ("save_mean", _VP), ("save_invstd", _VP),
                                      ("dout", _VP), ("dgamma", _VP), ("dbeta", _VP), ("dz", _VP), ("partial", _VP),
                                      ("P", _I32), ("C", _I32), ("relu", _I32)])
ScColsumItem = _struct("ScColsumItem", [("x", _VP), ("out", _VP), ("partial", _VP), ("P", _I32), ("C", _I32)])
ScActItem = _struct("ScActItem", [("z", _VP), ("scale", _VP), ("shift", _VP), ("out", _VP), ("total", c_int64), ("C", _I32)])


def _dp(t):
    return t.data_ptr() if t is not None else None


def _arr(cls, rows):
    return (cls * len(rows))(*[cls(*r) for r in rows])


def conv1x1_small_batch_rows(P):
    return L.call_int("ocr_conv1x1_small_batch_rows", c_int(P))


def conv1x1_small_batch(items):
    """items: [(x f16 [P,cin], w_kc32, bias | None, out f32 [P,cout], stats_partial | None)]"""
    rows = [(_dp(x), _dp(w), _dp(b), _dp(o), _dp(sp), x.numel() // x.shape[-1], x.shape[-1], o.shape[-1])
            for x, w, b, o, sp in items]
    L.call("ocr_conv1x1_small_batch_f16", _arr(HeadConvItem, rows), c_int(len(rows)), _st())


def conv1x1_small_dgrad_batch(items, grad_scale=1.0):
    """items: [(dz f32 [P,cout], w_ck32, dx f16 [P,cin], accumulate)]"""
    rows = [(_dp(dz), _dp(w), _dp(dx), dx.numel() // dx.shape[-1], dx.shape[-1], dz.shape[-1], int(acc))
            for dz, w, dx, acc in items]
    L.call("ocr_conv1x1_small_dgrad_batch_f16", _arr(HeadDgradItem, rows), c_int(len(rows)), c_float(grad_scale), _st())


def conv1x1_small_wgrad_batch_slab_bytes(P, cin):
    return L.call_size("ocr_conv1x1_small_wgrad_batch_slab_bytes", c_int(P), c_int(cin))


def conv1x1_small_wgrad_batch(items):
    """items: [(x f16 [P,cin], dz f32 [P,cout], dw f32 [cin,cout], slab)]"""
    rows = [(_dp(x), _dp(dz), _dp(dw), _dp(slab), x.numel() // x.shape[-1], x.shape[-1], dz.shape[-1])
            for x, dz, dw, slab in items]
    L.call("ocr_conv1x1_small_wgrad_batch_f16", _arr(HeadWgradItem, rows), c_int(len(rows)), _st())


def bn_finalize_batch(items, eps, decay):
    """items: [(partial, T, C, count, gamma, beta, moving_mean, moving_var, scale, shift, save_mean, save_invstd)]"""
    rows = [(_dp(p), T, C, float(cnt), _dp(ga), _dp(be), _dp(mm), _dp(mv), _dp(sc), _dp(sh), _dp(mu), _dp(istd))
            for p, T, C, cnt, ga, be, mm, mv, sc, sh, mu, istd in items]
    L.call("ocr_bn_finalize_batch", _arr(BnFinalizeItem, rows), c_int(len(rows)), c_float(eps), c_float(decay), _st())


def sc_bn_bwd_batch(items):
    """items: [(z, scale, shift, save_mean, save_invstd, dout, dgamma, dbeta, dz, partial, relu)] on [P][C] f32 tensors"""
    rows = [(_dp(z), _dp(sc), _dp(sh), _dp(mu), _dp(istd), _dp(do), _dp(dg), _dp(db), _dp(dz), _dp(part),
             z.numel() // z.shape[-1], z.shape[-1], int(relu))
            for z, sc, sh, mu, istd, do, dg, db, dz, part, relu in items]
    L.call("ocr_sc_bn_bwd_batch", _arr(ScBnBwdItem, rows), c_int(len(rows)), _st())


def sc_colsum_batch(items):
    """items: [(x f32 [P,C], out f32 [C], partial)]"""
    rows = [(_dp(x), _dp(o), _dp(part), x.numel() // x.shape[-1], x.shape[-1]) for x, o, part in items]
    L.call("ocr_sc_colsum_batch", _arr(ScColsumItem, rows), c_int(len(rows)), _st())


def sc_act_batch(items, relu):
    """items: [(z, scale, shift, out)]"""
    rows = [(_dp(z), _dp(sc), _dp(sh), _dp(o), z.numel(), z.shape[-1]) for z, sc, sh, o in items]
    L.call("ocr_sc_act_batch", _arr(ScActItem, rows), c_int(len(rows)), c_int(int(relu)), _st())


def sc_pointwise_pair_num_partials(P):
    return L.call_int("ocr_sc_pointwise_pair_num_partials", c_int(P))


def sc_pointwise_pair_fwd(x18, w_px, b_px, w_lk, b_lk, z_px, z_lk, part_px=None, part_lk=None):
    P = x18.numel() // 18
    L.call("ocr_sc_pointwise_pair_fwd", ptr(x18), ptr(w_px), ptr(b_px), ptr(w_lk), ptr(b_lk), c_int(P), ptr(z_px),
           ptr(z_lk), ptr(part_px), ptr(part_lk), _st())


def sc_pointwise_pair_bwd(x18, dz_px, dz_lk, w_px, w_lk, dx18, dw_px, db_px, dw_lk, db_lk, ws):
    P = x18.numel() // 18
    nbytes = L.call_size("ocr_sc_pointwise_pair_bwd_workspace")
    buf = ws.get(nbytes)
    L.call("ocr_sc_pointwise_pair_bwd", ptr(x18), ptr(dz_px), ptr(dz_lk), ptr(w_px), ptr(w_lk), c_int(P), ptr(dx18),
           ptr(dw_px), ptr(db_px), ptr(dw_lk), ptr(db_lk), ptr(buf), c_size_t(nbytes), _st())


def label_masks(labels, label_rule, pos_u8, neg_u8):
    L.call("ocr_label_masks", ptr(labels), c_int64(labels.numel()), c_int(label_rule), ptr(pos_u8), ptr(neg_u8), _st())


def ohnm_select(scores, pos_u8, neg_u8, n_pos_i32, n, hw, neg_ratio, selected_neg, selected):
    L.call("ocr_ohnm_select", ptr(scores), ptr(pos_u8), ptr(neg_u8), ptr(n_pos_i32), c_int(n), c_int(hw),
           c_float(neg_ratio), ptr(selected_neg), ptr(selected), _st())


def link_ce_fwd(gt, gt_stride, pred, pred_stride, w_pixel, count, sums4, loss1, ws):
    nbytes = L.call_size("ocr_link_ce_workspace", c_int64(count))
    buf = ws.get(nbytes)
    L.call("ocr_link_ce_fwd", ptr(gt), c_int(gt_stride), ptr(pred), c_int(pred_stride), ptr(w_pixel), c_int64(count),
           ptr(sums4), ptr(loss1), ptr(buf), c_size_t(nbytes), _st())


def link_ce_bwd(gt, gt_stride, pred, pred_stride, w_pixel, count, sums4, grad_scale, d_pred, d_stride):
    L.call("ocr_link_ce_bwd", ptr(gt), c_int(gt_stride), ptr(pred), c_int(pred_stride), ptr(w_pixel), c_int64(count),
           ptr(sums4), c_float(grad_scale), ptr(d_pred), c_int(d_stride), _st())


def link_ce_bwd_dyn(gt, gt_stride, pred, pred_stride, w_pixel, count, sums4, grad_scale, loss_scale, d_pred, d_stride):
    L.call("ocr_link_ce_bwd_dyn", ptr(gt), c_int(gt_stride), ptr(pred), c_int(pred_stride), ptr(w_pixel), c_int64(count),
           ptr(sums4), c_float(grad_scale), ptr(loss_scale), ptr(d_pred), c_int(d_stride), _st())


# ----------------------------------------------------------------------------- operand checks
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64
OPTIONAL = True
_DTYPE_WORDS = {F32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", I32: "int32", I64: "int64", U8: "uint8", F64: "float64"}


def _dims(what, name, t, rank=None):
    """The shape of operand `name`, which wrapper `what` reads free sizes from: a tensor (of `rank` dimensions), or refused."""
    shape = getattr(t, "shape", None)
    if shape is None or (rank is not None and len(shape) != rank):
        raise ValueError("%s: tensors do not match (%s is %s, wants %s)" % (
            what, name, None if shape is None else tuple(shape), "a tensor" if rank is None else "%d dimensions" % rank))
    return shape


def _operands(what, sizes, *rows):
    """The operand statement of wrapper `what`, enforced.  `sizes` names its free sizes; a row is (name, tensor, dtype,
    shape[, OPTIONAL]): shape a tuple of ints, an int (that many elements, any shape) or None (any), dtype None for a
    byte buffer of any element type, OPTIONAL for an operand that may be None.  Metadata only, nothing launches or
    synchronises.  Raises ValueError as three passes would, so that a call with several faults reports a shape before
    a dtype before a layout: every shape; every dtype; then contiguity and the device, which is the first operand's."""
    first = dtype_fault = layout_fault = None
    for row in rows:
        t, shape = row[1], row[3]
        if t is None and len(row) == 5:
            continue
        if t is None or (shape is not None and (t.numel() if type(shape) is int else t.shape) != shape):
            raise ValueError("%s: tensors do not match %s (%s is %s, wants %s)" % (
                what, sizes, row[0], None if t is None else tuple(t.shape), "%d elements" % shape if type(shape) is int else shape))
        if first is None:
            first, device = row[0], t.device
        if row[2] is not None and t.dtype != row[2] and dtype_fault is None:
            dtype_fault = "%s: %s is %s, wants %s" % (what, row[0], _DTYPE_WORDS.get(t.dtype, t.dtype), _DTYPE_WORDS[row[2]])
        if layout_fault is None:
            if not t.is_contiguous():
                layout_fault = "%s: contiguous tensors only (%s)" % (what, row[0])
            elif t.device != device:
                layout_fault = "%s: tensors on one device only (%s is on %s, %s on %s)" % (what, first, device, row[0], t.device)
    if dtype_fault or layout_fault:
        raise ValueError(dtype_fault or layout_fault)


def _workspace(ws, size_entry, *args):
    """(pointer, byte count) of the scratch that `size_entry(*args)` asks of the arena `ws`: an entry's two workspace arguments"""
    nbytes = L.call_size(size_entry, *args)
    return ptr(ws.get(nbytes)), c_size_t(nbytes)


# ----------------------------------------------------------------------------- decode
def softmax_pairs(logits, probs):
    pairs = _dims("softmax_pairs", "logits", logits).numel() // 2
    _operands("softmax_pairs", "pairs", ("logits", logits, F32, 2 * pairs), ("probs", probs, F32, 2 * pairs))
    L.call("ocr_softmax_pairs", ptr(logits), c_int64(pairs), ptr(probs), _st())


def link_softmax_stack(link_logits, out):
    m = _dims("link_softmax_stack", "link_logits", link_logits).numel() // 16
    _operands("link_softmax_stack", "m", ("link_logits", link_logits, F32, 16 * m), ("out", out, F32, 16 * m))
    L.call("ocr_link_softmax_stack", ptr(link_logits), c_int64(m), ptr(out), _st())


def pixel_detect(score_map, link_scores, n, h, w, score_thresh, link_thresh, mask):
    _operands("pixel_detect", "n, h, w",
              ("score_map", score_map, F32, n * h * w), ("link_scores", link_scores, F32, 16 * n * h * w), ("mask", mask, U8, h * w))
    L.call("ocr_pixel_detect", ptr(score_map), ptr(link_scores), c_int(n), c_int(h), c_int(w),
           c_float(score_thresh), c_float(link_thresh), ptr(mask), _st())


def _link_cc_rows(pixel_score, link_score, stride, n, h, w):
    # link_score by element count: the callers pass [8,n,h,w,2] read at stride 2, offset 1, or [8,n,h,w] at stride 1
    return ("pixel_score", pixel_score, F32, n * h * w), ("link_score", link_score, F32, 8 * n * h * w * stride)


def link_cc(pixel_score, link_score, stride, offset, n, h, w, pixel_thresh, link_thresh, min_size, labels,
            ncomp, comps, ws):
    max_comps = _dims("link_cc", "comps", comps, 3)[1]
    _operands("link_cc", "n, h, w, stride, max_comps", *_link_cc_rows(pixel_score, link_score, stride, n, h, w),
              ("labels", labels, I32, n * h * w), ("ncomp", ncomp, I32, n), ("comps", comps, I32, (n, max_comps, 2)))
    L.call("ocr_link_cc", ptr(pixel_score), ptr(link_score), c_int(stride), c_int(offset), c_int(n), c_int(h),
           c_int(w), c_float(pixel_thresh), c_float(link_thresh), c_int(min_size), ptr(labels), ptr(ncomp),
           ptr(comps), c_int(max_comps), *_workspace(ws, "ocr_link_cc_workspace", c_int(n), c_int(h), c_int(w)), _st())


def link_cc_directed(pixel_score, link_score, stride, offset, n, h, w, pixel_thresh, link_thresh, min_size,
                     union_labels, union_ncomp, labels, ncomp, comps, ws, seed_order=None):
    """The reference's directed-DFS grouping, refining ocr_link_cc's components (include/ocr_hip.h).
    seed_order: int32 [n, h*w] device tensor from `py27_dict_order` (None: ascending pixel index)."""
    max_comps = _dims("link_cc_directed", "comps", comps, 3)[1]
    _operands("link_cc_directed", "n, h, w, stride, max_comps", *_link_cc_rows(pixel_score, link_score, stride, n, h, w),
              ("union_labels", union_labels, I32, n * h * w), ("union_ncomp", union_ncomp, I32, n),
              ("seed_order", seed_order, I32, n * h * w, OPTIONAL), ("labels", labels, I32, n * h * w), ("ncomp", ncomp, I32, n),
              ("comps", comps, I32, (n, max_comps, 2)))
    L.call("ocr_link_cc_directed", ptr(pixel_score), ptr(link_score), c_int(stride), c_int(offset), c_int(n),
           c_int(h), c_int(w), c_float(pixel_thresh), c_float(link_thresh), c_int(min_size), ptr(union_labels),
           ptr(union_ncomp), ptr(seed_order), ptr(labels), ptr(ncomp), ptr(comps), c_int(max_comps),
           *_workspace(ws, "ocr_link_cc_directed_workspace", c_int(n), c_int(h), c_int(w)), _st())


def py27_dict_order(pixel_score_host, pixel_thresh):
    """HOST routine: pixel scores f32 [n,h,w] CPU tensor -> int32 [n, h*w] CPU tensor, per image the keys of the script's
    Python-2 dict in `graph.keys()` order, -1 padded (ocr_py27_dict_order)."""
    t = pixel_score_host
    assert t.dtype == torch.float32 and not t.is_cuda and t.is_contiguous()
    n, h, w = t.shape
    out = torch.empty((n, h * w), dtype=torch.int32)
    fn = L._fn("ocr_py27_dict_order", c_int)
    for b in range(n):
        rc = fn(ctypes.c_void_p(t[b].data_ptr()), c_float(pixel_thresh), c_int(h), c_int(w), ctypes.c_void_p(out[b].data_ptr()))
        if rc < 0:
            L.check(rc, "ocr_py27_dict_order")
    return out


def lanms(boxes, counts, iou_thresh, merged, n_merged, keep_idx, n_keep, ws):
    n, max_k, _ = _dims("lanms", "boxes", boxes, 3)
    _operands("lanms", "n, max_k",
              ("boxes", boxes, F32, (n, max_k, 9)), ("counts", counts, I32, n), ("merged", merged, F32, (n, max_k, 9)),
              ("n_merged", n_merged, I32, n), ("keep_idx", keep_idx, I32, (n, max_k)), ("n_keep", n_keep, I32, n))
    L.call("ocr_lanms", ptr(boxes), ptr(counts), c_int(n), c_int(max_k), c_float(iou_thresh), ptr(merged), ptr(n_merged),
           ptr(keep_idx), ptr(n_keep), *_workspace(ws, "ocr_lanms_workspace", c_int(n), c_int(max_k)), _st())


# ------------------------------------------------------------------------------- EAST RBOX geometry (csrc/rbox.hip)
def rbox_head_fwd(z, text_scale, score, geo):
    """z [..., 6] f32 -> score [..., 1], geo [..., 5] (four distances * text_scale, angle in (-pi/4, pi/4))."""
    P = score.numel()
    if z.numel() != 6 * P or geo.numel() != 5 * P:
        raise ValueError("rbox_head_fwd: z, score, geo must hold 6, 1, 5 values per pixel")
    L.call("ocr_rbox_head_fwd", ptr(z), c_int(P), c_float(text_scale), ptr(score), ptr(geo), _st())


def rbox_head_bwd(score, dscore, geo, dgeo, text_scale, dz):
    """dz [..., 6] from the stored outputs; dscore / dgeo may be None (zeros)."""
    P = score.numel()
    if dz.numel() != 6 * P or geo.numel() != 5 * P or (dscore is not None and dscore.numel() != P) or \
            (dgeo is not None and dgeo.numel() != 5 * P):
        raise ValueError("rbox_head_bwd: dz, score, geo must hold 6, 1, 5 values per pixel, the gradients as their outputs")
    L.call("ocr_rbox_head_bwd", ptr(score), ptr(dscore), ptr(geo), ptr(dgeo), c_int(P), c_float(text_scale), ptr(dz), _st())


def _rbox_loss_pixels(mask, per_pixel):
    P = mask.numel()
    for t, c in per_pixel:
        if t.numel() != c * P:
            raise ValueError("rbox loss: every map must cover the mask's %d pixels" % P)
    return P


def rbox_loss_fwd(yt_cls, yp_cls, yt_geo, yp_geo, mask, sums5, out4, ws):
    P = _rbox_loss_pixels(mask, ((yt_cls, 1), (yp_cls, 1), (yt_geo, 5), (yp_geo, 5)))
    nbytes = L.call_size("ocr_rbox_loss_workspace", c_int(P))
    buf = ws.get(nbytes)
    L.call("ocr_rbox_loss_fwd", ptr(yt_cls), ptr(yp_cls), ptr(yt_geo), ptr(yp_geo), ptr(mask), c_int(P), ptr(sums5),
           ptr(out4), ptr(buf), c_size_t(nbytes), _st())


def rbox_loss_bwd(yt_cls, yt_geo, yp_geo, mask, sums5, grad_scale, d_cls, d_geo):
    P = _rbox_loss_pixels(mask, ((yt_cls, 1), (yt_geo, 5), (yp_geo, 5), (d_cls, 1), (d_geo, 5)))
    L.call("ocr_rbox_loss_bwd", ptr(yt_cls), ptr(yt_geo), ptr(yp_geo), ptr(mask), c_int(P), ptr(sums5),
           c_float(grad_scale), ptr(d_cls), ptr(d_geo), _st())


def rbox_loss_bwd_dyn(yt_cls, yt_geo, yp_geo, mask, sums5, grad_scale, loss_scale, d_cls, d_geo):
    """rbox_loss_bwd with the seed grad_scale * loss_scale[0], `loss_scale` a DEVICE f32 (LossScaleState.scale_ptr)."""
    P = _rbox_loss_pixels(mask, ((yt_cls, 1), (yt_geo, 5), (yp_geo, 5), (d_cls, 1), (d_geo, 5)))
    L.call("ocr_rbox_loss_bwd_dyn", ptr(yt_cls), ptr(yt_geo), ptr(yp_geo), ptr(mask), c_int(P), ptr(sums5),
           c_float(grad_scale), ptr(loss_scale), ptr(d_cls), ptr(d_geo), _st())


def rbox_decode(score, geo, n, h, w, score_thresh, scale, boxes, counts, total, ws):
    """score [n,h,w], geo [n,h,w,5] -> boxes [n,max_k,9] in raster order, counts / total int32 [n]."""
    max_k = _dims("rbox_decode", "boxes", boxes, 3)[1]
    _operands("rbox_decode", "n, h, w, max_k",
              ("score", score, F32, n * h * w), ("geo", geo, F32, 5 * n * h * w), ("boxes", boxes, F32, (n, max_k, 9)),
              ("counts", counts, I32, n), ("total", total, I32, n))
    L.call("ocr_rbox_decode", ptr(score), ptr(geo), c_int(n), c_int(h), c_int(w), c_float(score_thresh), c_float(scale),
           c_int(max_k), ptr(boxes), ptr(counts), ptr(total),
           *_workspace(ws, "ocr_rbox_decode_workspace", c_int(n), c_int(h), c_int(w)), _st())


def quad_mean_score(quads, score, inv_scale, mean):
    """quads f32 [k,8] (image px), score f32 [h,w] -> mean f32 [k]: the score's mean over the fillPoly raster of each quad's
    vertices floor(trunc(coord) * inv_scale); 0 for an empty raster."""
    k = _dims("quad_mean_score", "quads", quads, 2)[0]
    h, w = _dims("quad_mean_score", "score", score, 2)
    _operands("quad_mean_score", "k, h, w", ("quads", quads, F32, (k, 8)), ("score", score, F32, (h, w)), ("mean", mean, F32, k))
    L.call("ocr_quad_mean_score", ptr(quads), c_int(k), ptr(score), c_int(h), c_int(w), c_float(inv_scale), ptr(mean), _st())


def _hull_rows(n, max_comps, hull_n, hull_head, calipers):
    return (("hull_n", hull_n, I32, (n, max_comps)), ("hull_head", hull_head, I32, (n, max_comps, 4)),
            ("calipers", calipers, F32, (n, max_comps, 6)))


def min_area_rects(labels, ncomp, max_comps, scale_x, scale_y, hull_n, hull_head, calipers, ws):
    n, h, w = _dims("min_area_rects", "labels", labels, 3)
    _operands("min_area_rects", "n, h, w, max_comps", ("labels", labels, I32, (n, h, w)), ("ncomp", ncomp, I32, n),
              *_hull_rows(n, max_comps, hull_n, hull_head, calipers))
    L.call("ocr_min_area_rects", ptr(labels), ptr(ncomp), c_int(n), c_int(h), c_int(w), c_int(max_comps),
           c_double(scale_x), c_double(scale_y), ptr(hull_n), ptr(hull_head), ptr(calipers),
           *_workspace(ws, "ocr_min_area_rects_workspace", c_int(n), c_int(h), c_int(w), c_int(max_comps)), _st())


def mask_cc(mask, value, connectivity, labels, ncomp, comps, ws):
    n, h, w = _dims("mask_cc", "mask", mask, 3)
    max_comps = _dims("mask_cc", "comps", comps, 3)[1]
    _operands("mask_cc", "n, h, w, max_comps", ("mask", mask, U8, (n, h, w)), ("labels", labels, I32, n * h * w),
              ("ncomp", ncomp, I32, n), ("comps", comps, I32, (n, max_comps, 2)))
    L.call("ocr_mask_cc", ptr(mask), c_int(value), c_int(connectivity), c_int(n), c_int(h), c_int(w), ptr(labels),
           ptr(ncomp), ptr(comps), c_int(max_comps), *_workspace(ws, "ocr_link_cc_workspace", c_int(n), c_int(h), c_int(w)), _st())


def hole_border_rects(mask, zlabels, nregions, max_regions, scale_x, scale_y, hull_n, hull_head, calipers, ws):
    n, h, w = _dims("hole_border_rects", "mask", mask, 3)
    _operands("hole_border_rects", "n, h, w, max_regions", ("mask", mask, U8, (n, h, w)), ("zlabels", zlabels, I32, n * h * w),
              ("nregions", nregions, I32, n), *_hull_rows(n, max_regions, hull_n, hull_head, calipers))
    L.call("ocr_hole_border_rects", ptr(mask), ptr(zlabels), ptr(nregions), c_int(n), c_int(h), c_int(w),
           c_int(max_regions), c_double(scale_x), c_double(scale_y), ptr(hull_n), ptr(hull_head), ptr(calipers),
           *_workspace(ws, "ocr_hole_border_rects_workspace", c_int(n), c_int(h), c_int(w), c_int(max_regions)), _st())


def east_pixel_detect(score, link16, h, w, score_thresh, link_thresh, mask, first_second):
    _operands("east_pixel_detect", "h, w", ("score", score, F32, h * w), ("link16", link16, F32, 16 * h * w),
              ("mask", mask, U8, h * w), ("first_second", first_second, I32, (2, 8)))
    L.call("ocr_east_pixel_detect", ptr(score), ptr(link16), c_int(h), c_int(w), c_float(score_thresh),
           c_float(link_thresh), ptr(mask), ptr(first_second), _st())


def contour_parents(labels, zlabels, comps, ncomp, zcomps, nregions, parent_c, parent_z):
    """The two `mask_cc` labellings of one mask [h,w] and their first ncomp / nregions comps rows -> parent_c int32
    [>= ncomp], parent_z int32 [>= nregions] (include/ocr_hip.h: ocr_contour_parents)."""
    h, w = _dims("contour_parents", "labels", labels)[-2:]
    _operands("contour_parents", "h, w", ("labels", labels, I32, h * w), ("zlabels", zlabels, I32, h * w),
              ("comps", comps, I32, None), ("zcomps", zcomps, I32, None), ("parent_c", parent_c, I32, None),
              ("parent_z", parent_z, I32, None))
    if comps.numel() < 2 * ncomp or zcomps.numel() < 2 * nregions or parent_c.numel() < ncomp or parent_z.numel() < nregions:
        raise ValueError("contour_parents: comps / zcomps / parent_c / parent_z hold fewer than ncomp = %d / nregions = %d rows"
                         % (ncomp, nregions))
    L.call("ocr_contour_parents", ptr(labels), ptr(zlabels), ptr(comps), c_int(ncomp), ptr(zcomps), c_int(nregions),
           c_int(h), c_int(w), ptr(parent_c), ptr(parent_z), _st())


def zero_pixels(mask, idx):
    """mask uint8 (any shape), idx int32: up to 256 flat indices into it."""
    _operands("zero_pixels", "count", ("mask", mask, U8, None), ("idx", idx, I32, None))
    L.call("ocr_zero_pixels_u8", ptr(mask), ptr(idx), c_int(idx.numel()), _st())


# ----------------------------------------------------------------------------- labels
def poly_cover(polys, counts, ignore, h, w, cover):
    n, P, V, _ = _dims("poly_cover", "polys", polys, 4)
    _operands("poly_cover", "n, max_polys, verts, h, w", ("polys", polys, I32, (n, P, V, 2)), ("counts", counts, I32, n),
              ("ignore", ignore, U8, (n, P)), ("cover", cover, I32, n * h * w))
    L.call("ocr_poly_cover", ptr(polys), ptr(counts), ptr(ignore), c_int(n), c_int(P), c_int(V), c_int(h),
           c_int(w), ptr(cover), _st())


def icdar_labels(cover, step, score, geo, mask):
    n, h, w = _dims("icdar_labels", "cover", cover, 3)
    cells = n * -(-h // max(step, 1)) * -(-w // max(step, 1))
    _operands("icdar_labels", "n, h, w, step", ("cover", cover, I32, (n, h, w)), ("score", score, F32, cells),
              ("geo", geo, F32, 8 * cells), ("mask", mask, F32, cells))
    L.call("ocr_icdar_labels", ptr(cover), c_int(n), c_int(h), c_int(w), c_int(step), ptr(score), ptr(geo),
           ptr(mask), _st())


def rbox_labels(cover_score, cover_full, rects, step, score, geo, mask):
    """Two cover maps int32 [n,h,w] (shrunk / full polygons) + rects f32 [n,P,5,3] -> score f32 [n,oh,ow,1], geo f32
    [n,oh,ow,5], mask f32 [n,oh,ow,1] at every step-th pixel."""
    n, h, w = _dims("rbox_labels", "cover_score", cover_score, 3)
    P = _dims("rbox_labels", "rects", rects, 4)[1]
    cells = n * -(-h // max(step, 1)) * -(-w // max(step, 1))
    _operands("rbox_labels", "n, h, w, step, max_polys",
              ("cover_score", cover_score, I32, (n, h, w)), ("cover_full", cover_full, I32, (n, h, w)),
              ("rects", rects, F32, (n, P, 5, 3)), ("score", score, F32, cells), ("geo", geo, F32, 5 * cells),
              ("mask", mask, F32, cells))
    L.call("ocr_icdar_rbox_labels", ptr(cover_score), ptr(cover_full), ptr(rects), c_int(n), c_int(P), c_int(h), c_int(w),
           c_int(step), ptr(score), ptr(geo), ptr(mask), _st())


def pixellink_labels(cover, new_h, new_w, score, link):
    n, h, w = _dims("pixellink_labels", "cover", cover, 3)
    _operands("pixellink_labels", "n, h, w, new_h, new_w", ("cover", cover, I32, (n, h, w)),
              ("score", score, F32, n * new_h * new_w), ("link", link, F32, 8 * n * new_h * new_w))
    L.call("ocr_pixellink_labels", ptr(cover), c_int(n), c_int(h), c_int(w), c_int(new_h), c_int(new_w),
           ptr(score), ptr(link), _st())


def pixellink_instance_weights(cover, ignore, new_h, new_w, area, weight):
    """Instance-balanced weight map of the label cells (include/ocr_hip.h: ocr_pixellink_instance_weights): cover int32
    [n,h,w] (ocr_poly_cover), ignore uint8 [n,P] -> area int32 [n,P] (cells owned per polygon), weight f32 [n,new_h,new_w]."""
    n, h, w = _dims("pixellink_instance_weights", "cover", cover, 3)
    P = _dims("pixellink_instance_weights", "ignore", ignore, 2)[1]
    _operands("pixellink_instance_weights", "n, max_polys, new_h, new_w",
              ("cover", cover, I32, (n, h, w)), ("ignore", ignore, U8, (n, P)), ("area", area, I32, (n, P)),
              ("weight", weight, F32, n * new_h * new_w))
    L.call("ocr_pixellink_instance_weights", ptr(cover), ptr(ignore), c_int(n), c_int(P), c_int(h), c_int(w),
           c_int(new_h), c_int(new_w), ptr(area), ptr(weight), _st())


def resize_linear_u8(src_u8, dst_f32):
    H, W, cn = _dims("resize_linear_u8", "src_u8", src_u8, 3)
    dh, dw, _ = _dims("resize_linear_u8", "dst_f32", dst_f32, 3)
    _operands("resize_linear_u8", "H, W, cn, dh, dw", ("src_u8", src_u8, U8, (H, W, cn)), ("dst_f32", dst_f32, F32, (dh, dw, cn)))
    L.call("ocr_resize_linear_u8", ptr(src_u8), c_int(H), c_int(W), c_int(cn), ptr(dst_f32), c_int(dh),
           c_int(dw), _st())


def augment_u8_batch(slab, desc, n, S, dst):
    """One launch for a batch (include/ocr_hip.h: ocr_augment_u8_batch): slab uint8 [bytes] holding the n source images,
    desc uint8 [>= n * sizeof(ocr_augment_desc)] (datasets/augment.py: DESC_DTYPE), dst f32 [n,S,S,3]; all on the device."""
    _operands("augment_u8_batch", "n, S", ("slab", slab, U8, None), ("desc", desc, U8, None), ("dst", dst, F32, (n, S, S, 3)))
    if desc.numel() < 112 * n:
        raise ValueError("augment_u8_batch: desc holds %d bytes, fewer than %d records of 112" % (desc.numel(), n))
    L.call("ocr_augment_u8_batch", ptr(slab), ptr(desc), c_int(n), c_int(S), ptr(dst), _st())


def resize_cubic_f32(src_f32, dst_f32, pre_scale=1.0, post_scale=1.0):
    """src f32 [planes,h,w] -> dst f32 [planes,dh,dw] (cv2.resize INTER_CUBIC per plane)."""
    planes, h, w = _dims("resize_cubic_f32", "src_f32", src_f32, 3)
    _, dh, dw = _dims("resize_cubic_f32", "dst_f32", dst_f32, 3)
    _operands("resize_cubic_f32", "planes, h, w, dh, dw",
              ("src_f32", src_f32, F32, (planes, h, w)), ("dst_f32", dst_f32, F32, (planes, dh, dw)))
    L.call("ocr_resize_cubic_f32", ptr(src_f32), c_int(planes), c_int(h), c_int(w), ptr(dst_f32), c_int(dh),
           c_int(dw), c_float(pre_scale), c_float(post_scale), _st())


def quad_iou(dets, gts, mask_h, mask_w, inter, uni):
    nd, V, _ = _dims("quad_iou", "dets", dets, 3)
    ng = _dims("quad_iou", "gts", gts, 3)[0]
    _operands("quad_iou", "nd, ng, verts", ("dets", dets, I32, (nd, V, 2)), ("gts", gts, I32, (ng, V, 2)),
              ("inter", inter, I32, (nd, ng)), ("uni", uni, I32, (nd, ng)))
    L.call("ocr_quad_iou", ptr(dets), c_int(nd), ptr(gts), c_int(ng), c_int(V), c_int(mask_h), c_int(mask_w),
           ptr(inter), ptr(uni), _st())


# ------------------------------------------------------------------ held-out evaluation on the device (csrc/eval_match.hip)
EVAL_MAX_D, EVAL_MAX_G = 1024, 254      # the most detections / ground truths per image the matcher takes


def _lanms_rows(merged, keep_idx, n_keep, n, max_k):
    """ocr_lanms's output layout, which the collect, pool and box entries read or write"""
    return ("merged", merged, F32, (n, max_k, 9)), ("keep_idx", keep_idx, I32, (n, max_k)), ("n_keep", n_keep, I32, n)


def _quad_rows(dets, nd, gts, ng, n, max_d, max_g):
    """the detection and ground-truth lists of both matchers"""
    return (("dets", dets, I32, (n, max_d, 4, 2)), ("nd", nd, I32, n), ("gts", gts, I32, (n, max_g, 4, 2)), ("ng", ng, I32, n))


def eval_collect(merged, keep_idx, n_keep, passed, inv_ratio, dets, det_score, nd, nd_total):
    """LANMS output (merged f32 [n,max_k,9], keep_idx int32 [n,max_k], n_keep int32 [n]; passed uint8 [n,max_k] or None) ->
    dets int32 [n,max_d,4,2] (kept quads / the resize ratios inv_ratio f32 [n,2] = (ratio_w, ratio_h), truncated), det_score
    f32 [n,max_d], in descending score order; nd = min(nd_total, max_d), nd_total int32 [n] (include/ocr_hip.h)."""
    n, max_k, _ = _dims("eval_collect", "merged", merged, 3)
    max_d = _dims("eval_collect", "dets", dets, 4)[1]
    _operands("eval_collect", "n, max_k, max_d", *_lanms_rows(merged, keep_idx, n_keep, n, max_k),
              ("passed", passed, U8, (n, max_k), OPTIONAL), ("inv_ratio", inv_ratio, F32, (n, 2)), ("dets", dets, I32, (n, max_d, 4, 2)),
              ("det_score", det_score, F32, (n, max_d)), ("nd", nd, I32, n), ("nd_total", nd_total, I32, n))
    L.call("ocr_eval_collect", ptr(merged), ptr(keep_idx), ptr(n_keep), ptr(passed), ptr(inv_ratio), c_int(n), c_int(max_k),
           c_int(max_d), ptr(dets), ptr(det_score), ptr(nd), ptr(nd_total), _st())


def eval_match_batch(dets, nd, gts, ng, gignored, threshold, mask_h, mask_w, tp, fp, record, ws):
    """bboxes_matching of n images in one call: dets int32 [n,max_d,4,2] / nd int32 [n] in matching order, gts int32
    [n,max_g,4,2] / ng int32 [n], gignored uint8 [n,max_g] -> tp, fp uint8 [n,max_d]; record int64 [4] is added to."""
    n, max_d = _dims("eval_match_batch", "dets", dets, 4)[:2]
    max_g = _dims("eval_match_batch", "gts", gts, 4)[1]
    _operands("eval_match_batch", "n, max_d, max_g", *_quad_rows(dets, nd, gts, ng, n, max_d, max_g),
              ("gignored", gignored, U8, (n, max_g)), ("tp", tp, U8, (n, max_d)), ("fp", fp, U8, (n, max_d)), ("record", record, I64, 4))
    L.call("ocr_eval_match_batch", ptr(dets), ptr(nd), ptr(gts), ptr(ng), ptr(gignored), c_int(n), c_int(max_d), c_int(max_g),
           c_float(threshold), c_int(mask_h), c_int(mask_w), ptr(tp), ptr(fp), ptr(record),
           *_workspace(ws, "ocr_eval_match_workspace", c_int(n), c_int(max_d), c_int(max_g)), _st())


def eval_ic15_match_batch(dets, nd, gts, ng, gdontcare, iou_thr, area_prec_thr, det_match, gt_match, record, ws, inter=None):
    """The ICDAR-2015 matching of n images in one call (include/ocr_eval_ic15.h): dets int32 [n,max_d,4,2] / nd int32 [n] in
    ocr_eval_collect's order, gts int32 [n,max_g,4,2] / ng int32 [n], gdontcare uint8 [n,max_g] -> det_match int32 [n,max_d]
    (gt index, -1 unmatched, -2 don't-care), gt_match int32 [n,max_g] (det index, -1, -2); record int64 [4] is added to;
    inter: optional float64 [n,max_g,max_d], the pair intersection areas."""
    n, max_d = _dims("eval_ic15_match_batch", "dets", dets, 4)[:2]
    max_g = _dims("eval_ic15_match_batch", "gts", gts, 4)[1]
    _operands("eval_ic15_match_batch", "n, max_d, max_g", *_quad_rows(dets, nd, gts, ng, n, max_d, max_g),
              ("gdontcare", gdontcare, U8, (n, max_g)), ("det_match", det_match, I32, (n, max_d)),
              ("gt_match", gt_match, I32, (n, max_g)), ("record", record, I64, 4), ("inter", inter, F64, (n, max_g, max_d), OPTIONAL))
    L.call("ocr_eval_ic15_match_batch", ptr(dets), ptr(nd), ptr(gts), ptr(ng), ptr(gdontcare), c_int(n), c_int(max_d),
           c_int(max_g), c_double(iou_thr), c_double(area_prec_thr), ptr(det_match), ptr(gt_match), ptr(inter), ptr(record),
           *_workspace(ws, "ocr_eval_ic15_workspace", c_int(n), c_int(max_d), c_int(max_g)), _st())


def eval_record_init(record):
    _operands("eval_record_init", "its four counters", ("record", record, I64, 4))
    L.call("ocr_eval_record_init", ptr(record), _st())


# ------------------------------------------------------------------ score-threshold sweep and AP (csrc/eval_curve.hip)
EVAL_MAX_T = 64                         # the most thresholds one sweep takes


def _pool_rows(pool_score, pool_cum, pool_nd, n, max_d):
    """rows of the AP pool"""
    return ("pool_score", pool_score, F32, (n, max_d)), ("pool_cum", pool_cum, I32, (n, max_d, 2)), ("pool_nd", pool_nd, I32, n)


def _curve_rows(what, det_score, nd, ng, thresholds, curve, unsorted, pool, n, max_d):
    """the operands the two curve entries share -> (T, their rows, the three pool tensors or None)"""
    T = _dims(what, "thresholds", thresholds, 1)[0]
    rows = (("det_score", det_score, F32, (n, max_d)), ("nd", nd, I32, n), ("ng", ng, I32, n), ("thresholds", thresholds, F32, (T,)),
            ("curve", curve, I64, (T, 4)), ("unsorted", unsorted, I32, 1))
    if pool is None:
        return T, rows, (None, None, None)
    return T, rows + _pool_rows(*pool, n, max_d), pool


def eval_curve_init(curve, unsorted, ap=None):
    """zeroes curve int64 [T,4], the order flag int32 [1] and, when given, ap float64 [1] (include/ocr_eval_curve.h)"""
    T = _dims("eval_curve_init", "curve", curve, 2)[0]
    _operands("eval_curve_init", "T", ("curve", curve, I64, (T, 4)), ("unsorted", unsorted, I32, 1), ("ap", ap, F64, 1, OPTIONAL))
    L.call("ocr_eval_curve_init", ptr(curve), c_int(T), ptr(unsorted), ptr(ap), _st())


def eval_curve_batch(tp, fp, det_score, nd, ng, gignored, thresholds, curve, unsorted, pool=None):
    """The counters of T score thresholds from the raster matcher's outputs (include/ocr_eval_curve.h): tp, fp uint8
    [n,max_d], det_score f32 [n,max_d], nd, ng int32 [n], gignored uint8 [n,max_g], thresholds f32 [T] -> curve int64 [T,4]
    is added to, unsorted int32 [1] OR-ed into; pool: None or (pool_score f32 [n,max_d], pool_cum int32 [n,max_d,2],
    pool_nd int32 [n]), these images' rows of the AP pool."""
    n, max_d = _dims("eval_curve_batch", "tp", tp, 2)
    max_g = _dims("eval_curve_batch", "gignored", gignored, 2)[1]
    T, rows, pool = _curve_rows("eval_curve_batch", det_score, nd, ng, thresholds, curve, unsorted, pool, n, max_d)
    _operands("eval_curve_batch", "n, max_d, max_g, T", ("tp", tp, U8, (n, max_d)), ("fp", fp, U8, (n, max_d)),
              ("gignored", gignored, U8, (n, max_g)), *rows)
    L.call("ocr_eval_curve_batch", ptr(tp), ptr(fp), ptr(det_score), ptr(nd), ptr(ng), ptr(gignored), ptr(thresholds), c_int(n),
           c_int(max_d), c_int(max_g), c_int(T), ptr(curve), ptr(unsorted), ptr(pool[0]), ptr(pool[1]), ptr(pool[2]), _st())


def eval_ic15_curve_batch(det_match, gt_match, det_score, nd, ng, thresholds, curve, unsorted, pool=None):
    """`eval_curve_batch` from the ICDAR-2015 matcher's outputs: det_match int32 [n,max_d], gt_match int32 [n,max_g]."""
    n, max_d = _dims("eval_ic15_curve_batch", "det_match", det_match, 2)
    max_g = _dims("eval_ic15_curve_batch", "gt_match", gt_match, 2)[1]
    T, rows, pool = _curve_rows("eval_ic15_curve_batch", det_score, nd, ng, thresholds, curve, unsorted, pool, n, max_d)
    _operands("eval_ic15_curve_batch", "n, max_d, max_g, T", ("det_match", det_match, I32, (n, max_d)),
              ("gt_match", gt_match, I32, (n, max_g)), *rows)
    L.call("ocr_eval_ic15_curve_batch", ptr(det_match), ptr(gt_match), ptr(det_score), ptr(nd), ptr(ng), ptr(thresholds),
           c_int(n), c_int(max_d), c_int(max_g), c_int(T), ptr(curve), ptr(unsorted), ptr(pool[0]), ptr(pool[1]), ptr(pool[2]), _st())


def eval_ap(pool_score, pool_cum, pool_nd, record, ap, ws):
    """Average precision over the pool of a pass (include/ocr_eval_curve.h: ocr_eval_ap): pool_score f32 [n_img,max_d],
    pool_cum int32 [n_img,max_d,2], pool_nd int32 [n_img], record int64 [4] (slot 0 = G, read on the device) -> ap
    float64 [1]."""
    n_img, max_d = _dims("eval_ap", "pool_score", pool_score, 2)
    _operands("eval_ap", "n_img, max_d", *_pool_rows(pool_score, pool_cum, pool_nd, n_img, max_d), ("record", record, I64, 4),
              ("ap", ap, F64, 1))
    L.call("ocr_eval_ap", ptr(pool_score), ptr(pool_cum), ptr(pool_nd), c_int(n_img), c_int(max_d), ptr(record), ptr(ap),
           *_workspace(ws, "ocr_eval_ap_workspace", c_int(n_img), c_int(max_d)), _st())


# ------------------------------------------------------------------ multi-scale pooling and fusion (csrc/multiscale.hip)
FUSE_MAX_POOL = 4096                    # the most pooled quads per image ocr_quad_fuse takes
FUSE_MODES = {'nms': 0, 'vote': 1}


def ms_pool_append(merged, keep_idx, n_keep, passed, mean, ratio, scale_id, pool, pool_scale, pool_count, pool_total,
                   pool_nonfinite):
    """One scale's LANMS output (merged f32 [n,max_k,9], keep_idx int32 [n,max_k], n_keep int32 [n]; passed uint8 [n,max_k] or
    None, per keep slot; mean f32 [n,max_k], the pooled score of each keep slot; ratio f32 [n,2] = (ratio_w, ratio_h)) is
    appended in keep order to pool f32 [n,max_pool,9] / pool_scale int32 [n,max_pool] after pool_count int32 [n]; pool_total
    keeps the true count, pool_nonfinite the dropped non-finite rows (include/ocr_multiscale.h: ocr_ms_pool_append)."""
    n, max_k, _ = _dims("ms_pool_append", "merged", merged, 3)
    max_pool = _dims("ms_pool_append", "pool", pool, 3)[1]
    _operands("ms_pool_append", "n, max_k, max_pool", *_lanms_rows(merged, keep_idx, n_keep, n, max_k),
              ("passed", passed, U8, (n, max_k), OPTIONAL), ("mean", mean, F32, (n, max_k)), ("ratio", ratio, F32, (n, 2)),
              ("pool", pool, F32, (n, max_pool, 9)), ("pool_scale", pool_scale, I32, (n, max_pool)), ("pool_count", pool_count, I32, n),
              ("pool_total", pool_total, I32, n), ("pool_nonfinite", pool_nonfinite, I32, n))
    L.call("ocr_ms_pool_append", ptr(merged), ptr(keep_idx), ptr(n_keep), ptr(passed), ptr(mean), ptr(ratio), c_int(scale_id),
           c_int(n), c_int(max_k), c_int(max_pool), ptr(pool), ptr(pool_scale), ptr(pool_count), ptr(pool_total),
           ptr(pool_nonfinite), _st())


def quad_fuse(pool, pool_count, iou_thresh, mode, fused, keep_idx, n_keep, owner, ws):
    """Score-ordered NMS over each image's pooled list (include/ocr_multiscale.h: ocr_quad_fuse): pool f32 [n,max_pool,9],
    pool_count int32 [n], mode 'nms' / 'vote' (or 0 / 1) -> fused f32 [n,max_pool,9], keep_idx int32 [n,max_pool], n_keep int32
    [n] (ocr_lanms's layout: ocr_eval_collect takes them as they are), owner int32 [n,max_pool]."""
    n, max_pool, _ = _dims("quad_fuse", "pool", pool, 3)
    mode = FUSE_MODES.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError("quad_fuse: mode is 'nms' (0) or 'vote' (1), got %r" % (mode,))
    if max_pool > FUSE_MAX_POOL:
        raise ValueError("quad_fuse: max_pool %d is beyond the %d pooled quads per image it takes" % (max_pool, FUSE_MAX_POOL))
    _operands("quad_fuse", "n, max_pool", ("pool", pool, F32, (n, max_pool, 9)), ("pool_count", pool_count, I32, n),
              ("fused", fused, F32, (n, max_pool, 9)), ("keep_idx", keep_idx, I32, (n, max_pool)), ("n_keep", n_keep, I32, n),
              ("owner", owner, I32, (n, max_pool)))
    if fused.data_ptr() == pool.data_ptr():
        raise ValueError("quad_fuse: fused must not be the pool")
    L.call("ocr_quad_fuse", ptr(pool), ptr(pool_count), c_int(n), c_int(max_pool), c_float(iou_thresh), c_int(mode), ptr(fused),
           ptr(keep_idx), ptr(n_keep), ptr(owner), *_workspace(ws, "ocr_quad_fuse_workspace", c_int(n), c_int(max_pool)), _st())


# ------------------------------------------------------------------ score-map fusion of the link geometry (csrc/map_fuse.hip)
def link_map_accumulate(pixel_logits, link_logits, flip, weight, first, acc):
    """One forward pass's LOGITS (pixel_logits f32 [n,hs,ws,2], link_logits f32 [n,hs,ws,16]) -> softmax index 1, sampled
    on the fusion grid, times `weight` (a normalised weight, finite and > 0), stored in (`first`) or added to acc f32
    [9,n,hf,wf]: plane 0 = P(text), 1 + d = P(link d); `flip`: the pass saw the images mirrored left to right
    (include/ocr_map_fuse.h: ocr_link_map_accumulate)."""
    n, hs, ws, _ = _dims("link_map_accumulate", "pixel_logits", pixel_logits, 4)
    hf, wf = _dims("link_map_accumulate", "acc", acc, 4)[2:]
    _operands("link_map_accumulate", "n, hs, ws, hf, wf", ("pixel_logits", pixel_logits, F32, (n, hs, ws, 2)),
              ("link_logits", link_logits, F32, (n, hs, ws, 16)), ("acc", acc, F32, (9, n, hf, wf)))
    weight = float(weight)
    if not (weight > 0.0 and weight != float("inf")):
        raise ValueError("link_map_accumulate: weight must be finite and positive, got %r" % (weight,))
    L.call("ocr_link_map_accumulate", ptr(pixel_logits), ptr(link_logits), c_int(n), c_int(hs), c_int(ws), c_int(int(bool(flip))),
           c_float(weight), c_int(int(bool(first))), ptr(acc), c_int(hf), c_int(wf), _st())


# ------------------------------------------------------------------ link-geometry detections (csrc/link_boxes.hip)
def component_scores(labels, pixel_score, ncomp, comp_score, ws):
    """labels int32 [n,h,w] (ocr_link_cc), pixel_score f32 [n,h,w], ncomp int32 [n] -> comp_score f32 [n,max_comps]: the
    mean pixel score of every component, summed as exact integers (include/ocr_hip.h: ocr_component_scores)."""
    n, h, w = _dims("component_scores", "labels", labels, 3)
    max_comps = _dims("component_scores", "comp_score", comp_score, 2)[1]
    _operands("component_scores", "n, h, w, max_comps", ("labels", labels, I32, (n, h, w)), ("pixel_score", pixel_score, F32, (n, h, w)),
              ("ncomp", ncomp, I32, n), ("comp_score", comp_score, F32, (n, max_comps)))
    L.call("ocr_component_scores", ptr(labels), ptr(pixel_score), ptr(ncomp), c_int(n), c_int(h), c_int(w), c_int(max_comps),
           ptr(comp_score), *_workspace(ws, "ocr_component_scores_workspace", c_int(n), c_int(max_comps)), _st())


def link_boxes(hull_n, hull_head, calipers, comp_score, ncomp, min_side, min_area, merged, keep_idx, n_keep, passed, total):
    """ocr_min_area_rects' outputs + comp_score f32 [n,max_comps] + ncomp int32 [n] -> the rows ocr_eval_collect reads:
    merged f32 [n,max_comps,9] (truncated corners, score), keep_idx int32 [n,max_comps] (identity), n_keep int32 [n],
    passed uint8 [n,max_comps], total int32 [n] (include/ocr_hip.h: ocr_link_boxes)."""
    n, max_comps = _dims("link_boxes", "hull_n", hull_n, 2)
    _operands("link_boxes", "n, max_comps", *_hull_rows(n, max_comps, hull_n, hull_head, calipers),
              ("comp_score", comp_score, F32, (n, max_comps)), ("ncomp", ncomp, I32, n),
              *_lanms_rows(merged, keep_idx, n_keep, n, max_comps), ("passed", passed, U8, (n, max_comps)), ("total", total, I32, n))
    L.call("ocr_link_boxes", ptr(hull_n), ptr(hull_head), ptr(calipers), ptr(comp_score), ptr(ncomp), c_int(n),
           c_int(max_comps), c_float(min_side), c_float(min_area), ptr(merged), ptr(keep_idx), ptr(n_keep), ptr(passed),
           ptr(total), _st())


# ------------------------------------------------------------------ the link decode over a threshold grid (csrc/decode_grid.hip)
GRID_MAX_POINTS = 65          # 64 grid points and the base pair (include/ocr_decode_grid.h)


def _grid_table(values, name):
    vals = [float(v) for v in values]
    if not 1 <= len(vals) <= GRID_MAX_POINTS:
        raise ValueError("%s: 1 to %d grid points, got %d" % (name, GRID_MAX_POINTS, len(vals)))
    return (ctypes.c_float * len(vals))(*vals)


def link_cc_grid(pixel_score, link_score, stride, offset, pixel_thresholds, link_thresholds, min_size, labels, ncomp, comps,
                 ws):
    """ocr_link_cc for G (pixel, link) threshold pairs in one launch sequence (include/ocr_decode_grid.h:
    ocr_link_cc_grid): pixel_score f32 [n,h,w], link_score as `link_cc` takes it, the thresholds two sequences of G
    numbers (host values: they travel in the kernel arguments) -> labels int32 [G*n,h,w], ncomp int32 [G*n], comps int32
    [G*n,max_comps,2]; slice g*n + i is image i at point g."""
    n, h, w = _dims("link_cc_grid", "pixel_score", pixel_score, 3)
    tp, tl = _grid_table(pixel_thresholds, "link_cc_grid"), _grid_table(link_thresholds, "link_cc_grid")
    G = len(tp)
    if len(tl) != G:
        raise ValueError("link_cc_grid: %d pixel thresholds for %d link thresholds" % (G, len(tl)))
    max_comps = _dims("link_cc_grid", "comps", comps, 3)[1]
    _operands("link_cc_grid", "G, n, h, w, stride, max_comps", *_link_cc_rows(pixel_score, link_score, stride, n, h, w),
              ("labels", labels, I32, (G * n, h, w)), ("ncomp", ncomp, I32, G * n), ("comps", comps, I32, (G * n, max_comps, 2)))
    L.call("ocr_link_cc_grid", ptr(pixel_score), ptr(link_score), c_int(stride), c_int(offset), c_int(n), c_int(h), c_int(w),
           c_int(G), tp, tl, c_int(min_size), ptr(labels), ptr(ncomp), ptr(comps), c_int(max_comps),
           *_workspace(ws, "ocr_link_cc_grid_workspace", c_int(G), c_int(n), c_int(h), c_int(w)), _st())


def component_scores_grid(labels, pixel_score, ncomp, comp_score, ws):
    """`component_scores` for labels int32 [G*n,h,w] against pixel_score f32 [n,h,w], slice b reading map b mod n ->
    comp_score f32 [G*n,max_comps] (include/ocr_decode_grid.h: ocr_component_scores_grid)."""
    N, h, w = _dims("component_scores_grid", "labels", labels, 3)
    n = _dims("component_scores_grid", "pixel_score", pixel_score, 3)[0]
    max_comps = _dims("component_scores_grid", "comp_score", comp_score, 2)[1]
    G = N // max(n, 1)
    _operands("component_scores_grid", "G, n, h, w, max_comps", ("labels", labels, I32, (G * n, h, w)),
              ("pixel_score", pixel_score, F32, (n, h, w)), ("ncomp", ncomp, I32, N), ("comp_score", comp_score, F32, (N, max_comps)))
    L.call("ocr_component_scores_grid", ptr(labels), ptr(pixel_score), ptr(ncomp), c_int(G), c_int(n), c_int(h), c_int(w),
           c_int(max_comps), ptr(comp_score), *_workspace(ws, "ocr_component_scores_grid_workspace", c_int(G), c_int(n), c_int(max_comps)),
           _st())


# -------------------------------------------------------------------------- optimiser
def adam_step(w, g, m, v, ema, n_reg, lr_t, beta1, beta2, eps, wd, inv_scale, ema_decay):
    L.call("ocr_adam_step", ptr(w), ptr(g), ptr(m), ptr(v), ptr(ema), c_int64(w.numel()),
           c_int64(n_reg), c_float(lr_t), c_float(beta1), c_float(beta2), c_float(eps), c_float(wd),
           c_float(inv_scale), c_float(ema_decay), _st())


def momentum_step(w, g, acc, ema, n_reg, lr, momentum, wd, inv_scale, ema_decay):
    L.call("ocr_momentum_step", ptr(w), ptr(g), ptr(acc), ptr(ema), c_int64(w.numel()), c_int64(n_reg),
           c_float(lr), c_float(momentum), c_float(wd), c_float(inv_scale), c_float(ema_decay), _st())


# dynamic loss scaling: `state` is the 8-word device block ocr_loss_scale_state (include/ocr_hip.h) as an int32 tensor
LOSS_SCALE_WORDS = 8
LS_SCALE, LS_INV_SCALE_USED, LS_SKIP, LS_GOOD_STEPS, LS_SKIPPED_TOTAL, LS_FOUND, LS_TICKET = range(7)


def loss_scale_init(state, init_scale):
    assert state.numel() >= LOSS_SCALE_WORDS and state.element_size() == 4
    L.call("ocr_loss_scale_init", ptr(state), c_float(init_scale), _st())


def grad_check(grad, state, growth_factor, backoff_factor, growth_interval, min_scale, max_scale):
    """One pass over the f32 buffer `grad` (any 4-byte aligned view): sets state.skip / inv_scale_used and moves the scale."""
    L.call("ocr_grad_check_f32", ptr(grad), c_int64(grad.numel()), ptr(state), c_float(growth_factor), c_float(backoff_factor),
           c_int(growth_interval), c_float(min_scale), c_float(max_scale), _st())


def adam_step_dyn(w, g, m, v, ema, n_reg, lr_t, beta1, beta2, eps, wd, grad_scale, ema_decay, state):
    L.call("ocr_adam_step_dyn", ptr(w), ptr(g), ptr(m), ptr(v), ptr(ema), c_int64(w.numel()),
           c_int64(n_reg), c_float(lr_t), c_float(beta1), c_float(beta2), c_float(eps), c_float(wd),
           c_float(grad_scale), c_float(ema_decay), ptr(state), _st())


def momentum_step_dyn(w, g, acc, ema, n_reg, lr, momentum, wd, grad_scale, ema_decay, state):
    L.call("ocr_momentum_step_dyn", ptr(w), ptr(g), ptr(acc), ptr(ema), c_int64(w.numel()), c_int64(n_reg),
           c_float(lr), c_float(momentum), c_float(wd), c_float(grad_scale), c_float(ema_decay), ptr(state), _st())


# global-norm gradient clipping: `clip_state` is the 8-word device block ocr_grad_clip_state (include/ocr_hip.h) as an
# int32 tensor, `ws` a float64 tensor of grad_clip_workspace(n) bytes that belongs to the caller (no arena: a recorded
# plan replays its address)
GRAD_CLIP_WORDS = 8
GC_G_MUL, GC_NORM, GC_COEF, GC_SKIP, GC_CLIPPED_TOTAL, GC_NONFINITE_TOTAL, GC_TICKET = range(7)


def grad_clip_init(clip_state):
    assert clip_state.numel() >= GRAD_CLIP_WORDS and clip_state.element_size() == 4
    L.call("ocr_grad_clip_init", ptr(clip_state), _st())


def grad_clip_workspace(n):
    """Bytes of the f64 partials for a gradient buffer of n elements."""
    return L.call_size("ocr_grad_clip_workspace", c_int64(n))


def grad_clip(grad, clip_state, clip_norm, base, ws):
    """One pass over the f32 buffer `grad`: norm of grad * base, coef, g_mul = base * coef and skip into `clip_state`."""
    L.call("ocr_grad_clip_f32", ptr(grad), c_int64(grad.numel()), ptr(clip_state), c_float(clip_norm), c_float(base),
           ptr(ws), c_size_t(ws.numel() * ws.element_size()), _st())


def grad_check_clip(grad, state, growth_factor, backoff_factor, growth_interval, min_scale, max_scale, clip_state, clip_norm,
                    grad_scale, ws):
    """grad_check and grad_clip in the same single pass, base = grad_scale / (the scale the gradients were produced with)."""
    L.call("ocr_grad_check_clip_f32", ptr(grad), c_int64(grad.numel()), ptr(state), c_float(growth_factor),
           c_float(backoff_factor), c_int(growth_interval), c_float(min_scale), c_float(max_scale), ptr(clip_state),
           c_float(clip_norm), c_float(grad_scale), ptr(ws), c_size_t(ws.numel() * ws.element_size()), _st())


def adam_step_clip(w, g, m, v, ema, n_reg, lr_t, beta1, beta2, eps, wd, ema_decay, clip_state):
    L.call("ocr_adam_step_clip", ptr(w), ptr(g), ptr(m), ptr(v), ptr(ema), c_int64(w.numel()),
           c_int64(n_reg), c_float(lr_t), c_float(beta1), c_float(beta2), c_float(eps), c_float(wd),
           c_float(ema_decay), ptr(clip_state), _st())


def momentum_step_clip(w, g, acc, ema, n_reg, lr, momentum, wd, ema_decay, clip_state):
    L.call("ocr_momentum_step_clip", ptr(w), ptr(g), ptr(acc), ptr(ema), c_int64(w.numel()), c_int64(n_reg),
           c_float(lr), c_float(momentum), c_float(wd), c_float(ema_decay), ptr(clip_state), _st())


# gradient accumulation: `state` is the 8-word device block ocr_grad_accum_state (include/ocr_hip.h) as an int32 tensor
GRAD_ACCUM_WORDS = 8
GA_MICRO, GA_K, GA_WINDOWS_TOTAL = range(3)


def grad_accum_init(state, k):
    assert state.numel() >= GRAD_ACCUM_WORDS and state.element_size() == 4
    L.call("ocr_grad_accum_init", ptr(state), c_int(k), _st())


def grad_accum(grad, acc, state):
    """One pass over the f32 buffers `grad` and `acc` (equal length, equal address modulo 16): store, add or close the
    window, as state.micro and state.k say."""
    assert grad.numel() == acc.numel()
    L.call("ocr_grad_accum_f32", ptr(grad), ptr(acc), c_int64(grad.numel()), ptr(state), _st())


def grad_accum_advance(state):
    L.call("ocr_grad_accum_advance", ptr(state), _st())


# training summaries (summary.TensorStats): `table` is the device copy of ocr_tensor_stats_table's host table (uint8),
# `records` a uint8 tensor of n_segments * tensor_stats_record_bytes() bytes, `ws` a float64 tensor of
# tensor_stats_workspace(n_chunks) bytes; all three belong to the caller
def tensor_stats_num_buckets():
    return L.call_int("ocr_tensor_stats_num_buckets")


def tensor_stats_chunk():
    return L.call_int("ocr_tensor_stats_chunk")


def tensor_stats_record_bytes():
    return L.call_size("ocr_tensor_stats_record_bytes")


def tensor_stats_limits():
    """The 1551 bucket limits as the library builds them (numpy float64; host only)."""
    import numpy as np
    out = np.empty(tensor_stats_num_buckets(), np.float64)
    L.call("ocr_tensor_stats_limits", out.ctypes.data_as(ctypes.c_void_p), c_int(out.size))
    return out


def tensor_stats_table(offsets, sizes):
    """(host table as a numpy uint8 array, n_chunks) for segments [offset, offset + size) in elements."""
    import numpy as np
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    szs = np.ascontiguousarray(sizes, dtype=np.int64)
    assert offs.ndim == 1 and offs.shape == szs.shape and offs.size > 0
    table = np.zeros((L.call_size("ocr_tensor_stats_table_bytes", c_int(offs.size)) + 7) // 8, np.int64)
    n_chunks = c_int64(0)
    L.call("ocr_tensor_stats_table", c_int(offs.size), offs.ctypes.data_as(ctypes.c_void_p),
           szs.ctypes.data_as(ctypes.c_void_p), table.ctypes.data_as(ctypes.c_void_p), byref(n_chunks))
    return table.view(np.uint8), int(n_chunks.value)


def tensor_stats_workspace(n_chunks):
    return L.call_size("ocr_tensor_stats_workspace", c_int64(n_chunks))


def tensor_stats(x, table, n_segments, mul_host, mul_dev, records, ws):
    """Per-segment records of the f32 buffer `x` times mul_host * mul_dev[0] (mul_dev: a 1-element f32 device view or None)."""
    _operands("tensor_stats", "n_segments", ("x", x, F32, None), ("table", table, None, None), ("mul_dev", mul_dev, F32, 1, OPTIONAL),
              ("records", records, None, None), ("ws", ws, None, None))
    if records.numel() * records.element_size() < n_segments * tensor_stats_record_bytes():
        raise ValueError("tensor_stats: records holds fewer than n_segments = %d records" % n_segments)
    L.call("ocr_tensor_stats_f32", ptr(x), ptr(table), c_int(n_segments), c_float(mul_host), ptr(mul_dev), ptr(records),
           ptr(ws), c_size_t(ws.numel() * ws.element_size()), _st())


def summary_image_workspace():
    return L.call_size("ocr_summary_image_workspace")


def summary_image_u8(x, out, ws):
    """One image [h, w, c] f32 -> u8 [h, w, c] by tf.summary.image's float rule."""
    h, w, c = _dims("summary_image_u8", "x", x, 3)
    _operands("summary_image_u8", "h, w, c", ("x", x, F32, (h, w, c)), ("out", out, U8, h * w * c), ("ws", ws, None, None))
    if ws.numel() * ws.element_size() < summary_image_workspace():
        raise ValueError("summary_image_u8: ws holds fewer than the %d bytes it takes" % summary_image_workspace())
    L.call("ocr_summary_image_u8", ptr(x), c_int(h), c_int(w), c_int(c), ptr(out), ptr(ws), _st())


def scale_(x, s):
    L.call("ocr_scale_f32", ptr(x), c_int64(x.numel()), c_float(s), _st())


def fill_(x, value=0.0):
    """Fill a 4-byte-element tensor (or an even-length f16 tensor, value 0 only) with `value`."""
    nbytes = x.numel() * x.element_size()
    assert nbytes % 4 == 0 and (x.element_size() == 4 or value == 0.0)
    L.call("ocr_fill_f32", ptr(x), c_int64(nbytes // 4), c_float(value), _st())


# ------------------------------------------------------------------- f32 inference precision
# (product library: matrix-core f32 convolution + element-wise f32 kernels, csrc/f32_infer.hip; the plain direct
#  convolution of libocr_verify.so / include/ocr_verify.h is its independent checker: F32_CONV = "direct";
#  F32_CONV = "split" runs every convolution of an f32 graph as Graph(precision="f16x2") does, csrc/f16x2_infer.hip)
F32_CONV = os.environ.get("OCR_F32_CONV", "mfma")


def conv2d_f32_split_workspace(d):
    return L.call_size("ocr_conv2d_f32_split_workspace", byref(d))


class ConvF32Epilogue(ctypes.Structure):
    """ocr_conv_f32_epilogue (include/ocr_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("bias", "scale", "shift", "residual")]


def conv2d_same_geometry(size, k, stride, rate=1):
    """One spatial dim of resnet_utils.conv2d_same (nets/resnet_utils.py:74-123) -> (out, pad_before): explicit padding of
    k_eff - 1 (the smaller half first), then a VALID convolution at `stride`: out = ceil(size / stride).  At stride 1 this
    is TF 'SAME'; at stride s it is the [::s] subsample of the stride-1 SAME convolution, computed directly.  Pure host
    arithmetic (tests/test_fold_bn_host.py)."""
    k_eff = (k - 1) * rate + 1
    return -(-size // stride), (k_eff - 1) // 2


def conv2d_same_desc(x_shape, cout, k, stride=1, rate=1):
    """The descriptor of conv2d_same at its real stride."""
    _, h, w, _ = x_shape
    oh, pt = conv2d_same_geometry(h, k, stride, rate)
    ow, pl = conv2d_same_geometry(w, k, stride, rate)
    return conv_desc(x_shape, cout, k, k, stride, rate, pad=(pt, pl), out_hw=(oh, ow))


def conv2d_f32(d, x, w_hwio, y, bias=None, route=None, workspace=None, scale=None, shift=None, residual=None,
               accum_in=False):
    """route: None -> F32_CONV (OCR_F32_CONV: "mfma" | "direct" | "split"); "mfma" = v_mfma_f32_32x32x2_f32 (f32_infer.hip);
    "direct" = the checker of libocr_verify.so; "split" = split-f16 operands on v_mfma_f32_16x16x32_f16 (f16x2_infer.hip),
    the convolution of Graph(precision="f16x2").  workspace (split route only): a callable returning the caller's
    stream-ordered `Workspace` for the packed weights (Graph.split_workspace: one arena per tower, like its other scratch);
    without one the call takes a buffer of its own from the allocator.
    Epilogue (ocr_conv2d_f32_mfma_ep / ocr_conv2d_f32_split_ep; the flags are added to d.flags for the call, `d` itself is
    left alone): accum_in -> OCR_CONV_ACCUM_IN (conv += y first), scale + shift [cout] -> OCR_CONV_AFFINE, residual
    [n,oh,ow,cout] -> OCR_CONV_RESIDUAL; order: accum_in, affine, bias, residual, ReLU, OCR_CONV_ACCUM_F16.  The "direct"
    route computes the same unfused — its convolution, then the element-wise f32 kernels — for the combinations the layers
    use (affine [+ accum_in] [+ ReLU]; affine + residual + ReLU) and raises on any other."""
    route = route or F32_CONV
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come together")
    flags = d.flags | (L.CONV_AFFINE if scale is not None else 0) | (L.CONV_RESIDUAL if residual is not None else 0) | \
        (L.CONV_ACCUM_IN if accum_in else 0)
    if route == "direct":
        return _conv2d_f32_direct(d, flags, x, w_hwio, y, bias, scale, shift, residual)
    de = L.ConvDesc.from_buffer_copy(d)
    de.flags = flags
    ep = ConvF32Epilogue(_dp(bias), _dp(scale), _dp(shift), _dp(residual))
    if route == "split":
        nbytes = conv2d_f32_split_workspace(de)
        buf = workspace().get(nbytes) if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        L.call("ocr_conv2d_f32_split_ep", byref(de), ptr(x), ptr(w_hwio), byref(ep), ptr(y), ptr(buf), c_size_t(nbytes),
               _st())
    else:
        L.call("ocr_conv2d_f32_mfma_ep", byref(de), ptr(x), ptr(w_hwio), byref(ep), ptr(y), _st())


def _conv2d_f32_direct(d, flags, x, w_hwio, y, bias, scale, shift, residual):
    new = flags & (L.CONV_AFFINE | L.CONV_RESIDUAL | L.CONV_ACCUM_IN)
    if not new:
        L.call_verify("ocr_conv2d_f32", byref(d), ptr(x), ptr(w_hwio), ptr(bias), ptr(y), _st())
        return
    relu = bool(flags & L.CONV_RELU)
    tail = new == (L.CONV_AFFINE | L.CONV_RESIDUAL) and relu
    if not (new in (L.CONV_AFFINE, L.CONV_AFFINE | L.CONV_ACCUM_IN) or tail) or \
            flags & (L.CONV_BIAS | L.CONV_ACCUM_F16):
        raise NotImplementedError("conv2d_f32 route 'direct': no unfused form of flags %d" % flags)
    dr = L.ConvDesc.from_buffer_copy(d)
    dr.flags = L.CONV_ACCUM_F16 if flags & L.CONV_ACCUM_IN else 0
    raw = y.clone() if flags & L.CONV_ACCUM_IN else torch.empty_like(y)
    L.call_verify("ocr_conv2d_f32", byref(dr), ptr(x), ptr(w_hwio), ptr(None), ptr(raw), _st())
    if tail:
        bn_add_relu_f32(raw, scale, shift, residual, y)
    else:
        bn_relu_f32(raw, scale, shift, relu, 0, y, None)


def subsample_f32(x, stride, y):
    n, h, w, c = x.shape
    L.call("ocr_subsample_f32", ptr(x), c_int(n), c_int(h), c_int(w), c_int(c), c_int(stride), ptr(y), _st())


def channel_stats_f32_num_partials(npix, c):
    return L.call_int("ocr_channel_stats_f32_num_partials", c_int64(npix), c_int(c))


def channel_stats_f32(x, c, partial):
    L.call("ocr_channel_stats_f32", ptr(x), c_int64(x.numel() // c), c_int(c), ptr(partial), _st())


def bn_relu_f32(y, scale, shift, relu, pool, a_full=None, a_pool=None):
    n, h, w, c = y.shape
    L.call("ocr_bn_relu_f32", ptr(y), ptr(scale), ptr(shift), c_int(n), c_int(h), c_int(w), c_int(c),
           c_int(int(relu)), c_int(pool), ptr(a_full), ptr(a_pool), _st())


def maxpool_f32(x, k, stride, pad, y):
    n, h, w, c = x.shape
    _, oh, ow, _ = y.shape
    L.call("ocr_maxpool_f32", ptr(x), c_int(n), c_int(h), c_int(w), c_int(c), c_int(k), c_int(stride),
           c_int(pad[0]), c_int(pad[1]), c_int(oh), c_int(ow), ptr(y), _st())


def prep_images_f32(images, out, means):
    L.call("ocr_prep_images_f32", ptr(images), c_int64(images.numel() // 3), c_float(means[0]),
           c_float(means[1]), c_float(means[2]), ptr(out), _st())


def bn_add_relu_f32(y, scale, shift, shortcut, out):
    c = y.shape[-1]
    L.call("ocr_bn_add_relu_f32", ptr(y), ptr(scale), ptr(shift), ptr(shortcut), c_int64(y.numel() // c),
           c_int(c), ptr(out), _st())


def unpool_f32(x, y):
    n, h, w, c = x.shape
    L.call("ocr_unpool_f32", ptr(x), c_int(n), c_int(h), c_int(w), c_int(c), ptr(y), _st())
