"""GPU: the folded inference batch norm — the f32 epilogue of `ocr_conv2d_f32_mfma_ep` / `ocr_conv2d_f32_split_ep`
(csrc/f32_conv_ep.h: accumulate-in, affine, bias, residual, ReLU, accumulate) against float64 in the kernels' order; the
argument contract; conv2d_same at its real stride against the subsample of the stride-1 convolution; whole nets through
Graph(fold_bn=True) at the north star's 1e-3 against the f32 oracle; what a folded forward launches; HIP-graph replay; the
interface.  References are float64 / the f32 oracle, never the new path's own output (slim.conv2d + slim.batch_norm:
nets/resnet_v1.py:97-111, nets/resnet_utils.py:74-123, nets/model_vgg_16.py:85-136, nets/model.py:84-143)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

BIAS, RELU, ACCUM_F16, AFFINE, RESIDUAL, ACCUM_IN = 1, 2, 8, 16, 32, 64

# (n, h, w, cin, cout, k, stride, rate), all with the conv2d_same geometry (TF SAME at stride 1)
SHAPES = [
    (1, 17, 23, 64, 128, 3, 1, 1),       # odd map, 128-cout tile
    (2, 9, 11, 130, 66, 3, 1, 1),        # ragged cin and cout, scalar stores
    (1, 16, 16, 256, 64, 1, 1, 1),       # the 256 x 64 tile variant
    (1, 8, 8, 64, 256, 1, 1, 1),
    (1, 15, 15, 64, 64, 3, 2, 1),        # 3x3 / 2 of a block's last unit
    (1, 20, 20, 3, 64, 7, 2, 1),         # ResNet root 7x7 / 2
]
FLAGSETS = [AFFINE, AFFINE | RELU, AFFINE | BIAS, AFFINE | RESIDUAL | RELU, ACCUM_IN | AFFINE | RELU, RESIDUAL]
FLAG_IDS = ["affine", "affine_relu", "affine_bias", "affine_residual_relu", "accumin_affine_relu", "residual"]
ROUTES = ("split", "mfma")
MARGIN = 64                              # floats on either side of y (and of the residual) that must come back untouched
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands of one shape (numpy f32) and its float64 convolution, computed once and shared by every flag set / route."""
    from tensorflow_ocr_amd import ops
    n, h, w, cin, cout, k, stride, rate = shape
    rng = np.random.default_rng(1000 + sum(shape))
    d = ops.conv2d_same_desc((n, h, w, cin), cout, k, stride, rate)
    c = dict(
        x=rng.standard_normal((n, h, w, cin)).astype(np.float32),
        w=(rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32),
        scale=(rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32),     # some channels negative
        shift=rng.standard_normal(cout).astype(np.float32),
        bias=rng.standard_normal(cout).astype(np.float32),
        residual=rng.standard_normal((n, d.oh, d.ow, cout)).astype(np.float32),
        y_old=rng.standard_normal((n, d.oh, d.ow, cout)).astype(np.float32))
    k_eff = (k - 1) * rate + 1
    xt = torch.from_numpy(c["x"]).double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(c["w"]).double().permute(3, 2, 0, 1)
    pad = (d.pad_left, max(0, (d.ow - 1) * stride + k_eff - w - d.pad_left),
           d.pad_top, max(0, (d.oh - 1) * stride + k_eff - h - d.pad_top))
    c["conv64"] = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, pad), wt, stride=stride, dilation=rate).permute(0, 2, 3, 1)
    assert tuple(c["conv64"].shape) == (n, d.oh, d.ow, cout)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _ref64(c, flags):
    """(pre-ReLU, final) in float64, the steps in the kernels' order."""
    f = lambda name: torch.from_numpy(c[name]).double()
    v = c["conv64"].clone()
    if flags & ACCUM_IN:
        v = v + f("y_old")
    if flags & AFFINE:
        v = v * f("scale") + f("shift")
    if flags & BIAS:
        v = v + f("bias")
    if flags & RESIDUAL:
        v = v + f("residual")
    pre = v
    if flags & RELU:
        v = v.clamp_min(0)
    if flags & ACCUM_F16:
        v = v + f("y_old")
    return pre, v


def _framed(device, arr_or_shape, margin, fill=None):
    """A tensor of the given shape (or holding the given array) inside a larger buffer of sentinels -> (buffer, view)."""
    shape = arr_or_shape if isinstance(arr_or_shape, tuple) else arr_or_shape.shape
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * margin,), SENTINEL, dtype=torch.float32, device=device)
    view = buf[margin:margin + numel].view(shape)
    if not isinstance(arr_or_shape, tuple):
        view.copy_(torch.from_numpy(arr_or_shape))
    elif fill is not None:
        view.fill_(fill)
    return buf, view


def _run(device, shape, flags, route, margin=MARGIN):
    """Launch one epilogue case -> (y on the CPU, margins untouched?)."""
    from tensorflow_ocr_amd import ops
    n, h, w, cin, cout, k, stride, rate = shape
    c = _case(shape)
    d = ops.conv2d_same_desc((n, h, w, cin), cout, k, stride, rate)
    d.flags = flags & (BIAS | RELU | ACCUM_F16)
    dev = lambda name: torch.from_numpy(c[name]).to(device)
    reads_y = bool(flags & (ACCUM_IN | ACCUM_F16))
    if reads_y:
        ybuf, y = _framed(device, c["y_old"], margin)
    else:
        ybuf, y = _framed(device, (n, d.oh, d.ow, cout), margin, fill=float("nan"))     # every element must be stored
    rbuf, res = _framed(device, c["residual"], margin)
    ops.conv2d_f32(d, dev("x"), dev("w"), y, dev("bias") if flags & BIAS else None, route=route,
                   scale=dev("scale") if flags & AFFINE else None, shift=dev("shift") if flags & AFFINE else None,
                   residual=res if flags & RESIDUAL else None, accum_in=bool(flags & ACCUM_IN))
    torch.cuda.synchronize()
    clean = bool((ybuf[:margin] == SENTINEL).all()) and bool((ybuf[margin + y.numel():] == SENTINEL).all()) and \
        bool((rbuf[:margin] == SENTINEL).all()) and bool((rbuf[margin + res.numel():] == SENTINEL).all()) and \
        bool(torch.equal(res.cpu(), torch.from_numpy(c["residual"])))
    return y.cpu(), clean


@pytest.mark.parametrize("flags", FLAGSETS, ids=FLAG_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_epilogue_vs_float64(device, shape, flags):
    """Bar: 4e-6 of max|pre-ReLU reference|, the ratio test_gpu_f16x2.py / test_gpu_f32_mfma.py hold the plain convolutions
    to; the epilogue adds at most three f32 roundings (2^-24 each, of values of the reference's magnitude), below it."""
    pre, ref = _ref64(_case(shape), flags)
    scale = float(pre.abs().max())
    for route in ROUTES:
        y, clean = _run(device, shape, flags, route)
        assert bool(torch.isfinite(y).all()), route                     # no NaN left: every element of y was stored
        err = float((y.double() - ref).abs().max())
        print("%s flags %3d %-5s: %.2e of max|pre-ReLU ref| = %.2f" % (shape, flags, route, err / scale, scale))
        assert err <= 4e-6 * scale, route
        assert clean, route


@pytest.mark.parametrize("route", ROUTES)
def test_epilogue_unaligned_y_and_residual(device, route):
    """y and the residual 4 bytes off a 16-byte boundary: the scalar path, same arithmetic, same bar, same store contract."""
    shape, flags = SHAPES[0], AFFINE | RESIDUAL | RELU
    pre, ref = _ref64(_case(shape), flags)
    y, clean = _run(device, shape, flags, route, margin=MARGIN + 1)
    ya, _ = _run(device, shape, flags, route)
    err = float((y.double() - ref).abs().max()) / float(pre.abs().max())
    print("unaligned %s: %.2e" % (route, err))
    assert err <= 4e-6 and clean and torch.equal(y, ya)


@pytest.mark.parametrize("route", ROUTES)
def test_plain_entry_points_are_thin_callers(device, route):
    """ocr_conv2d_f32_mfma / ocr_conv2d_f32_split (the host layer no longer calls them) give the bits of the `_ep` entry points
    under the flags they always took, and refuse the new ones (OCR_ERR_INVALID_ARG, y as it was) instead of dropping them."""
    from tensorflow_ocr_amd import _lib as L, ops
    shape = SHAPES[1]
    n, h, w, cin, cout, k, stride, rate = shape
    c = _case(shape)
    x, wt, bias = (torch.from_numpy(c[nm]).to(device) for nm in ("x", "w", "bias"))
    for flags in (BIAS | RELU, ACCUM_F16, 0):
        d = ops.conv2d_same_desc((n, h, w, cin), cout, k, stride, rate)
        d.flags = flags
        want = torch.from_numpy(c["y_old"]).to(device)
        ops.conv2d_f32(d, x, wt, want, bias if flags & BIAS else None, route=route)
        got = torch.from_numpy(c["y_old"]).to(device)
        nbytes = ops.conv2d_f32_split_workspace(d)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

        def plain():
            if route == "split":
                return L._fn("ocr_conv2d_f32_split", ctypes.c_int)(ctypes.byref(d), L.ptr(x), L.ptr(wt), L.ptr(bias), L.ptr(got),
                                                                   L.ptr(buf), ctypes.c_size_t(nbytes), L.stream_ptr())
            return L._fn("ocr_conv2d_f32_mfma", ctypes.c_int)(ctypes.byref(d), L.ptr(x), L.ptr(wt), L.ptr(bias), L.ptr(got), L.stream_ptr())
        for new_flag in (AFFINE, RESIDUAL, ACCUM_IN, AFFINE | RESIDUAL | ACCUM_IN):
            d.flags = flags | new_flag                                     # not served by the plain entries: refused
            assert plain() == -1, (flags, new_flag)
        torch.cuda.synchronize()
        assert torch.equal(got, torch.from_numpy(c["y_old"]).to(device)), flags
        d.flags = flags
        assert plain() == 0
        torch.cuda.synchronize()
        assert torch.equal(got, want), flags


def test_epilogue_argument_errors(device):
    """OCR_ERR_INVALID_ARG: a flag whose pointer is NULL (scale / shift, residual, bias), ACCUM_IN together with ACCUM_F16.
    Nothing is launched, y stays as it was."""
    from tensorflow_ocr_amd import _lib as L, ops
    lib = L.load()
    d = ops.conv2d_same_desc((1, 8, 8, 32), 64, 3, 1, 1)
    x = torch.zeros((1, 8, 8, 32), dtype=torch.float32, device=device)
    wt = torch.zeros((3, 3, 32, 64), dtype=torch.float32, device=device)
    y = torch.full((1, 8, 8, 64), 7.0, dtype=torch.float32, device=device)
    vec = torch.ones((64,), dtype=torch.float32, device=device)
    res = torch.ones((1, 8, 8, 64), dtype=torch.float32, device=device)
    nbytes = ops.conv2d_f32_split_workspace(d)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    P = lambda t: t.data_ptr() if t is not None else None

    def call(flags, bias=None, scale=None, shift=None, residual=None, ep_null=False):
        d.flags = flags
        ep = ops.ConvF32Epilogue(P(bias), P(scale), P(shift), P(residual))
        epp = None if ep_null else ctypes.byref(ep)
        lib.ocr_conv2d_f32_mfma_ep.restype = lib.ocr_conv2d_f32_split_ep.restype = ctypes.c_int
        return (lib.ocr_conv2d_f32_mfma_ep(ctypes.byref(d), L.ptr(x), L.ptr(wt), epp, L.ptr(y), L.stream_ptr()),
                lib.ocr_conv2d_f32_split_ep(ctypes.byref(d), L.ptr(x), L.ptr(wt), epp, L.ptr(y), L.ptr(buf),
                                            ctypes.c_size_t(nbytes), L.stream_ptr()))
    bad = (-1, -1)
    assert call(AFFINE) == bad and call(AFFINE, scale=vec) == bad and call(AFFINE, shift=vec) == bad
    assert call(RESIDUAL) == bad and call(AFFINE | RESIDUAL, scale=vec, shift=vec) == bad
    assert call(BIAS) == bad
    assert call(ACCUM_IN | ACCUM_F16) == bad and call(ACCUM_IN | ACCUM_F16 | AFFINE, scale=vec, shift=vec) == bad
    assert call(AFFINE, ep_null=True) == bad
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # ... and the same descriptors with their pointers are accepted
    assert call(AFFINE | RESIDUAL | BIAS | RELU, bias=vec, scale=vec, shift=vec, residual=res) == (0, 0)
    assert call(ACCUM_IN, ep_null=True) == (0, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", SHAPES[4:], ids=["3x3s2_15", "7x7s2_20"])
def test_strided_conv_equals_subsampled_stride1(device, shape, route):
    """conv2d_same(stride 2) launched at its real stride == [::2, ::2] of the stride-1 SAME convolution, bit for bit: per
    output the taps and channels are accumulated in the same order, and a padded tap adds an exact zero in both."""
    from tensorflow_ocr_amd import ops
    n, h, w, cin, cout, k, stride, rate = shape
    c = _case(shape)
    x, wt = torch.from_numpy(c["x"]).to(device), torch.from_numpy(c["w"]).to(device)
    ds = ops.conv2d_same_desc((n, h, w, cin), cout, k, stride, rate)
    d1 = ops.conv_desc((n, h, w, cin), cout, k, k, 1, rate)
    ys = torch.full((n, ds.oh, ds.ow, cout), float("nan"), dtype=torch.float32, device=device)
    y1 = torch.full((n, d1.oh, d1.ow, cout), float("nan"), dtype=torch.float32, device=device)
    ops.conv2d_f32(ds, x, wt, ys, route=route)
    ops.conv2d_f32(d1, x, wt, y1, route=route)
    sub = torch.empty_like(ys)
    ops.subsample_f32(y1, stride, sub)
    torch.cuda.synchronize()
    assert torch.equal(sub, y1[:, ::stride, ::stride])
    assert bool(torch.isfinite(ys).all()) and torch.equal(ys, y1[:, ::stride, ::stride])


# ------------------------------------------------------------------------------------------------------- whole nets
SMALL = [("block1", [(128, 64, 1), (128, 64, 2)]), ("block2", [(256, 64, 1), (256, 64, 2)]),
         ("block3", [(256, 128, 1), (256, 128, 2)]), ("block4", [(512, 128, 1)])]
NETS = [("resnet", "small_128"), ("resnet", "full_64"), ("east", "small_128"), ("east", "full_64")]


def _moving(p, rng):
    for k in p:
        if k.endswith('moving_mean'):
            p[k] = rng.normal(0, 0.1, p[k].shape).astype(np.float32)
        if k.endswith('moving_variance'):
            p[k] = rng.uniform(0.5, 1.5, p[k].shape).astype(np.float32)
    return p


def _trained_regime(p):
    """An absolute 1e-3 on logits presupposes the activations of a trained detector.  With frozen statistics of variance
    ~1 nothing normalises a He-initialised net: the root convolution sees a +-128 image, every unit's residual branch adds
    at full weight, pool5 reaches 1e4 .. 1e6 and the logits 1e3 .. 2e5, where the f32 ORACLE is itself 1.2e-2 .. 0.24 from
    its own float64 run (measured on the CPU; no f32 implementation can be nearer).  So, for oracle and device alike: the root
    weights take the image range (/ 100, what its trained batch norm would do) and the last batch norm of each residual branch
    starts small (gamma x 0.25, the usual initialisation of deep residual nets).  Then pool5 <= 30, logits <= 30, the score
    maps span (0, 1) unsaturated, and the oracle's own f32 error is <= 2e-5: fifty times under the bar."""
    for k in p:
        if k.endswith("resnet_v1_50/conv1/weights"):
            p[k] = (p[k] / 100.0).astype(np.float32)
        if k.endswith("conv3/BatchNorm/gamma"):
            p[k] = (p[k] * 0.25).astype(np.float32)
    return p


def _p_link(lk):
    return torch.softmax(lk.reshape(lk.shape[:-1] + (8, 2)), -1)


@functools.lru_cache(maxsize=None)
def _net_case(net, size_id):
    """(params, images, oracle outputs) of one net: the oracle runs once, both precisions share it."""
    blocks, size = (SMALL, 128) if size_id == "small_128" else (None, 64)
    rng = np.random.default_rng(40 + len(net) + size)
    init = O.init_model_resnet_params if net == "resnet" else O.init_model_east_params
    p = _trained_regime(_moving(init(rng, blocks), rng))
    images, _, _, _ = O.synthetic_batch(rng, 2, size)
    tp = O.to_torch_params(p, requires_grad=False)
    with torch.no_grad():
        if net == "resnet":
            px, lk, _ = O.model_resnet(torch.from_numpy(images), tp, False, mixed=False, blocks=blocks)
            refs = [px, lk, torch.softmax(px, -1), _p_link(lk)]
        else:
            fs, geo, _ = O.model_east(torch.from_numpy(images), tp, False, mixed=False, blocks=blocks)
            refs = [fs, geo]
    return p, images, refs, blocks


def _forward(g, net, blocks, images):
    from tensorflow_ocr_amd.nets import model, model_vgg_16, resnet_model
    if net == "resnet":
        if blocks is None:
            px, lk = model.model(images, is_training=False, graph=g)                    # test.py's graph
        else:
            px, lk = resnet_model.model_resnet50_pixellink(images, is_training=False, graph=g, blocks=blocks)
        return [px.data, lk.data, torch.softmax(px.data, -1), _p_link(lk.data)]
    fs, geo = model_vgg_16.model(images, is_training=False, graph=g, blocks=blocks)
    return [fs.data, geo.data]


def _build(device, prec, fold, net, blocks, p, images):
    from tensorflow_ocr_amd import checkpoint
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device, precision=prec, fold_bn=fold)
    _forward(g, net, blocks, images)
    g.reset_tape()
    g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, p))
    outs = [t.clone().cpu() for t in _forward(g, net, blocks, images)]
    g.reset_tape()
    return outs


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
@pytest.mark.parametrize("net,size_id", NETS, ids=["%s_%s" % t for t in NETS])
def test_folded_nets_within_1e3(device, net, size_id, prec):
    """is_training=False, n = 2, randomised moving statistics: logits and softmax maps of `model.model` (test.py's graph),
    F_score and geo_map of `model_vgg_16.model`, all < 1e-3 of the f32 oracle."""
    p, images, refs, blocks = _net_case(net, size_id)
    folded = _build(device, prec, True, net, blocks, p, images)
    plain = _build(device, prec, False, net, blocks, p, images)
    torch.cuda.synchronize()
    labels = ["pixel logits", "link logits", "P(text)", "P(link)"] if net == "resnet" else ["F_score", "geo_map"]
    worst = 0.0
    for i, lab in enumerate(labels):
        e = float((folded[i] - refs[i]).abs().max())
        print("%s %s %s %s: folded vs oracle %.2e | unfolded vs oracle %.2e | folded vs unfolded %.2e" % (
            net, size_id, prec, lab, e, float((plain[i] - refs[i]).abs().max()), float((folded[i] - plain[i]).abs().max())))
        worst = max(worst, e)
    assert worst < 1e-3


def _count_calls(monkeypatch, device, fold, blocks, images, prec="f16x2"):
    """Every library call of one ResNet + heads forward -> [(name, args)]."""
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device, precision=prec, fold_bn=fold)
    _forward(g, "resnet", blocks, images)                 # creates the variables
    g.reset_tape()
    calls = []
    real = L.call

    def counting(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(L, "call", counting)
    _forward(g, "resnet", blocks, images)
    monkeypatch.setattr(L, "call", real)
    g.reset_tape()
    torch.cuda.synchronize()
    return calls


def test_launch_accounting(device, monkeypatch):
    """The folded ResNet forward: no ocr_bn_relu_f32, no ocr_bn_add_relu_f32, no 1x1 max-pool (subsample pass), as many
    convolutions as the unfolded one; the unfolded one (fold_bn=False): what the graph launched before the fold existed,
    counted from the block structure — per unit 3 convolutions (+1 projection), 2 bn_relu (+1), 1 bn_add_relu, and at stride 2
    a subsample of conv2 and one of the identity shortcut; the root: 1 convolution, 1 subsample, 1 bn_relu, 1 3x3 pool."""
    _, images, _, blocks = _net_case("resnet", "small_128")

    def tally(calls):
        names = [nm for nm, _ in calls]
        return dict(conv=sum(nm.startswith("ocr_conv2d_f32") for nm in names),
                    bn_relu=names.count("ocr_bn_relu_f32"), bn_add_relu=names.count("ocr_bn_add_relu_f32"),
                    pool1=sum(nm == "ocr_maxpool_f32" and a[5].value == 1 for nm, a in calls),
                    pool3=sum(nm == "ocr_maxpool_f32" and a[5].value == 3 for nm, a in calls),
                    subsample=names.count("ocr_subsample_f32"), bn_params=names.count("ocr_bn_inference_params"))
    units, cin = [], 64
    for _, us in blocks:
        for depth, _, stride in us:
            units.append((depth, stride, depth != cin))
            cin = depth
    n_proj = sum(proj for _, _, proj in units)
    n_s2 = sum(stride == 2 for _, stride, _ in units)
    n_sub_sc = sum(stride == 2 and not proj for _, stride, proj in units)
    heads = 4 * 2 + 2                            # four sources x (pixel, link) + the two final 1x1 convolutions at most
    plain = tally(_count_calls(monkeypatch, device, False, blocks, images))
    folded = tally(_count_calls(monkeypatch, device, True, blocks, images))
    print("unfolded", plain)
    print("folded  ", folded)
    trunk_convs = 1 + 3 * len(units) + n_proj
    assert plain["bn_relu"] == 1 + 2 * len(units) + n_proj and plain["bn_add_relu"] == len(units)
    assert plain["pool1"] == 1 + n_s2 + n_sub_sc and plain["pool3"] == 1 and plain["subsample"] == 0
    assert trunk_convs <= plain["conv"] <= trunk_convs + heads
    assert folded["bn_relu"] == 0 and folded["bn_add_relu"] == 0 and folded["pool1"] == 0
    assert folded["conv"] == plain["conv"] and folded["pool3"] == 1 and folded["subsample"] == n_sub_sc
    assert folded["bn_params"] == plain["bn_params"]            # still launches of the forward: a restore is followed


def test_graphed_folded_forward_equals_eager(device):
    """A captured folded `model.model` forward replays bit for bit what the launches give one by one, on two inputs and after a
    load_state_dict that changes weights and moving statistics (the affine is computed inside the captured forward)."""
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import model
    rng = np.random.default_rng(17)

    def fn(gr, x):
        px, lk = model.model(x, is_training=False, graph=gr)
        return px.data, lk.data
    ge, gg = (Graph(device, seed=3, precision="f16x2", fold_bn=True) for _ in range(2))
    fwd = GraphedForward(gg, fn, capture_after=0)

    def eager(x):
        out = fn(ge, x)
        ge.reset_tape()
        return [o.clone() for o in out]
    outs = []
    for i in range(3):
        if i == 2:
            sd = {}
            for k, v in ge.store.state_dict().items():
                sd[k] = v * 0.5 + 0.25 if k.endswith("moving_variance") else (v + 0.05 if k.endswith("moving_mean") else v * 0.75)
            ge.store.load_state_dict(sd)
            gg.store.load_state_dict(sd)
        x = torch.from_numpy(rng.uniform(0, 255, (1, 64, 96, 3)).astype(np.float32)).to(device)
        want = eager(x)
        got = fwd(x)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), i
        assert float(want[0].abs().sum()) > 0 and bool(torch.isfinite(want[1]).all())
        outs.append(want[0].clone())
    assert len(fwd.cache) == 1
    assert not torch.equal(outs[1], outs[0])


def test_fold_bn_interface(device):
    from tensorflow_ocr_amd.graph import Graph
    with pytest.raises(ValueError):
        Graph(device, precision="f16", fold_bn=True)
    assert Graph(device, precision="f16").fold_bn is False and Graph(device, precision="f32").fold_bn is False
    assert Graph(device, precision="f32", fold_bn=True).fold_bn and Graph(device, precision="f16x2", fold_bn=True).fold_bn


def test_east_test_script_runs_folded(device, tmp_path, capsys, monkeypatch):
    """test.py --precision f16x2 --fold-bn end to end (the set-up of test_gpu_drivers.py::test_east_test_script_end_to_end: a
    checkpoint whose trunk is switched off and whose pixel head says "text" everywhere -> one box per image)."""
    import importlib.util
    import os
    import re
    from tensorflow_ocr_amd import checkpoint, graph
    from tensorflow_ocr_amd.nets import model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ocr_test_script", os.path.join(root, "test.py"))
    east = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(east)
    rng = np.random.default_rng(2)
    os.makedirs(os.path.join(tmp_path, "in"))
    for i, (H, W) in enumerate([(200, 260), (160, 160)]):
        np.save(os.path.join(tmp_path, "in", "photo_%d.npy" % i), rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
    g0 = graph.Graph(device, seed=3)
    model.model(np.zeros((1, 64, 64, 3), np.float32), is_training=False, graph=g0)
    sd = checkpoint.internal_to_tf(g0.store.state_dict())
    sd["feature_fusion/Conv_9/weights"] = np.zeros_like(sd["feature_fusion/Conv_9/weights"])
    sd["feature_fusion/Conv_9/biases"] = np.zeros_like(sd["feature_fusion/Conv_9/biases"])
    for k in sd:
        if k.endswith("BatchNorm/gamma"):
            sd[k] = np.zeros_like(sd[k])
    sd["feature_fusion/Conv_8/biases"] = np.array([0.0, 3.0], np.float32)
    ck = os.path.join(tmp_path, "ckpt")
    checkpoint.save_tf_checkpoint(ck, 7, sd, {k: v for k, v in sd.items() if "moving_" not in k})
    built = []
    real = graph.Graph

    def spy(*a, **kw):
        built.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(graph, "Graph", spy)
    out_dir = os.path.join(tmp_path, "res")
    monkeypatch.setattr("sys.argv", ["test.py", "--test_data_path", os.path.join(tmp_path, "in"), "--output_dir", out_dir,
                                     "--checkpoint_path", ck, "--precision", "f16x2", "--fold-bn"])
    east.main()
    out = capsys.readouterr().out
    assert built and built[0] == {"precision": "f16x2", "fold_bn": True}
    assert "Find 2 images" in out and out.count("net time:") == 2 and "Restore from" in out
    for i in range(2):
        lines = open(os.path.join(out_dir, "res_photo_%d.txt" % i), newline="").read().split("\r\n")[:-1]
        assert len(lines) == 1 and re.fullmatch(r"-?\d+(,-?\d+){7}", lines[0]), lines
