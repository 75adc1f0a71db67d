"""GPU: the f16x2 inference precision — `ocr_conv2d_f32_split` (split-f16 operands on v_mfma_f32_16x16x32_f16,
csrc/f16x2_infer.hip) against float64 over the convolution shapes of the three nets and over wide dynamic ranges; whole nets
through Graph(precision="f16x2") at the north star's 1e-3 against the f32 oracle; HIP-graph replay; the interface.  Every
comparison is against float64 / the f32 oracle, never against the new route's own output (slim.conv2d: nets/vgg.py:14-39,
nets/resnet_v1.py:97-105)."""
import os

import numpy as np
import pytest
import torch

from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu

# (n, h, w, cin, cout, k, stride, rate, flags)   flags: 1 bias, 2 relu, 8 accumulate   (the list of test_gpu_f32_mfma.py)
SHAPES = [
    (2, 32, 32, 3, 64, 3, 1, 1, 0),          # conv1_1 (cin = 3: the scalar staging path)
    (2, 24, 40, 64, 64, 3, 1, 1, 0),
    (1, 17, 23, 64, 128, 3, 1, 1, 3),        # odd map, bias + ReLU
    (2, 16, 16, 256, 256, 3, 1, 1, 0),
    (1, 16, 16, 512, 1024, 3, 1, 6, 0),      # fc6: dilation 6
    (1, 16, 16, 1024, 1024, 1, 1, 1, 1),     # fc7
    (2, 33, 31, 64, 256, 1, 1, 1, 8),        # 1x1 accumulate (concat-free merge conv)
    (1, 30, 30, 64, 64, 3, 2, 1, 0),         # stride 2
    (1, 20, 20, 3, 64, 7, 2, 1, 0),          # ResNet root 7x7/2
    (1, 9, 9, 128, 18, 1, 1, 1, 1),          # head conv: cout 18
    (1, 8, 8, 130, 66, 3, 1, 1, 2),          # ragged cin / cout
]


def _ref64(d, x, wt, bias, y0, k, stride, rate, flags):
    """float64 convolution through torch on the CPU, bias / ReLU / accumulate in the kernels' order."""
    h, w = x.shape[1], x.shape[2]
    xt = x.double().cpu().permute(0, 3, 1, 2)
    wtt = wt.double().cpu().permute(3, 2, 0, 1)
    pad = (d.pad_left, max(0, (d.ow - 1) * stride + (k - 1) * rate + 1 - w - d.pad_left),
           d.pad_top, max(0, (d.oh - 1) * stride + (k - 1) * rate + 1 - h - d.pad_top))
    ref = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, pad), wtt, stride=stride, dilation=rate).permute(0, 2, 3, 1)
    if flags & 1:
        ref = ref + bias.double().cpu()
    if flags & 2:
        ref = ref.clamp_min(0)
    if flags & 8:
        ref = ref + y0.double().cpu()
    return ref


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_f32_split_vs_float64(device, shape):
    """Bar: 4e-6 of max|ref|, what the f32 MFMA route is held to (an f16-only kernel gives ~3e-4)."""
    from tensorflow_ocr_amd import ops
    n, h, w, cin, cout, k, stride, rate, flags = shape
    rng = np.random.default_rng(sum(shape))
    x = torch.from_numpy(rng.standard_normal((n, h, w, cin)).astype(np.float32)).to(device)
    wt = torch.from_numpy((rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)).to(device)
    bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(device)
    d = ops.conv_desc((n, h, w, cin), cout, k, k, stride, rate)
    d.flags = flags
    y0 = torch.from_numpy(rng.standard_normal((n, d.oh, d.ow, cout)).astype(np.float32)).to(device)
    ys = {}
    for route in ("split", "mfma", "direct"):
        ys[route] = y0.clone()
        ops.conv2d_f32(d, x, wt, ys[route], bias if flags & 1 else None, route=route)
    torch.cuda.synchronize()
    ref = _ref64(d, x, wt, bias, y0, k, stride, rate, flags)
    scale = float(ref.abs().max())
    e = {r: float((ys[r].double().cpu() - ref).abs().max()) for r in ys}
    print("split vs f64 %.2e | mfma vs f64 %.2e | direct vs f64 %.2e (scale %.2f; relative %.2e)" % (
        e["split"], e["mfma"], e["direct"], scale, e["split"] / scale))
    assert e["split"] <= 4e-6 * scale


@pytest.mark.parametrize("scale2", [0, -10], ids=["as_drawn", "times_2^-10"])
@pytest.mark.parametrize("shape", [(1, 16, 16, 512, 128, 3), (1, 24, 24, 1024, 128, 1)], ids=["3x3_cin512", "1x1_cin1024"])
def test_conv_f32_split_dynamic_range(device, shape, scale2):
    """Per-element magnitudes N(0,1) 10^U(-6,2) for x and N(0,1)/sqrt(K) 10^U(-3,0) for w (and every operand times 2^-10:
    the activations of an under-scaled net).  Bar 1e-5 of max|ref|: the host emulation's worst case for this distribution
    is 2.5e-6 (half subnormals flushed; 3.9e-7 if honoured), 4x over that for the device's accumulation order, 30x under a
    kernel without the correction terms."""
    from tensorflow_ocr_amd import ops
    n, h, w, cin, cout, k = shape
    K = k * k * cin
    rng = np.random.default_rng(20260 + cin)
    f = np.float32(2.0 ** scale2)
    x = (rng.standard_normal((n, h, w, cin)) * 10.0 ** rng.uniform(-6, 2, (n, h, w, cin))).astype(np.float32) * f
    wt = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(K) * 10.0 ** rng.uniform(-3, 0, (k, k, cin, cout))).astype(np.float32) * f
    x, wt = torch.from_numpy(x).to(device), torch.from_numpy(wt).to(device)
    d = ops.conv_desc((n, h, w, cin), cout, k, k, 1, 1)
    d.flags = 0
    ys = {}
    for route in ("split", "mfma"):
        ys[route] = torch.zeros((n, d.oh, d.ow, cout), dtype=torch.float32, device=device)
        ops.conv2d_f32(d, x, wt, ys[route], None, route=route)
    torch.cuda.synchronize()
    ref = _ref64(d, x, wt, None, None, k, 1, 1, 0)
    scale = float(ref.abs().max())
    e = {r: float((ys[r].double().cpu() - ref).abs().max()) / scale for r in ys}
    print("dynamic range %s x 2^%d: split %.2e | mfma %.2e of max|ref| = %.3e" % (shape, scale2, e["split"], e["mfma"], scale))
    assert e["split"] <= 1e-5


def _moving(p, rng):
    for k in p:
        if k.endswith('moving_mean'):
            p[k] = rng.normal(0, 0.1, p[k].shape).astype(np.float32)
        if k.endswith('moving_variance'):
            p[k] = rng.uniform(0.5, 1.5, p[k].shape).astype(np.float32)
    return p


def _p_link(lk):
    return torch.softmax(lk.reshape(lk.shape[:-1] + (8, 2)), -1)


def _both_routes(device, build, first, images, p):
    """{precision: outputs} of `build(graph, images)`; the weights are loaded AFTER the first build, on `first` images."""
    from tensorflow_ocr_amd import checkpoint
    from tensorflow_ocr_amd.graph import Graph
    outs = {}
    for prec in ("f16x2", "f32"):
        g = Graph(device, precision=prec)
        build(g, first)
        g.reset_tape()
        g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, p))
        outs[prec] = [t.clone().cpu() for t in build(g, images)]
        g.reset_tape()
    torch.cuda.synchronize()
    return outs


def _report(name, outs, refs, labels):
    errs = []
    for i, lab in enumerate(labels):
        e2, e32 = float((outs["f16x2"][i] - refs[i]).abs().max()), float((outs["f32"][i] - refs[i]).abs().max())
        print("%s %s: f16x2 vs oracle %.2e | f32 route vs oracle %.2e | f16x2 vs f32 route %.2e" % (
            name, lab, e2, e32, float((outs["f16x2"][i] - outs["f32"][i]).abs().max())))
        errs.append(e2)
    return max(errs)


@pytest.mark.parametrize("size,n", [(64, 2), (512, 1)])
def test_model_vgg_f16x2_within_1e3(device, size, n):
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    rng = np.random.default_rng(0)
    p = _moving(O.init_model_vgg_params(rng), rng)
    images, _, _, _ = O.synthetic_batch(rng, n, size)

    def build(g, im):
        px, lk = M.model_vgg(im, is_training=False, graph=g)
        return [px.data, lk.data, torch.softmax(px.data, -1), _p_link(lk.data)]
    outs = _both_routes(device, build, images[:, :64, :64], images, p)
    with torch.no_grad():
        fpx, flk, _ = O.model_vgg(torch.from_numpy(images), O.to_torch_params(p, requires_grad=False), False, mixed=False)
    refs = [fpx, flk, torch.softmax(fpx, -1), _p_link(flk)]
    worst = _report("model_vgg %d^2 n=%d" % (size, n), outs, refs, ["pixel logits", "link logits", "P(text)", "P(link)"])
    assert worst < 1e-3


@pytest.mark.parametrize("size,n", [(64, 2), (512, 1)])
def test_pixellink_f16x2_within_1e3(device, size, n):
    from tensorflow_ocr_amd.nets import pixellink
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    rng = np.random.default_rng(2)
    p = O.init_pixellink_params(rng)
    images, _, _, _ = O.synthetic_batch(rng, n, size)
    x = ((images - 120.0) / 60.0).astype(np.float32)

    def build(g, im):
        net = pixellink.PixelLinkNet(im, graph=g)
        return [net.pixel_cls.data, net.link_cls.data, net.pixel_scores, _p_link(net.link_cls.data)]
    outs = _both_routes(device, build, x[:, :64, :64], x, p)
    with torch.no_grad():
        opx, olk, _ = O.pixellink_net(torch.from_numpy(x), O.to_torch_params(p, requires_grad=False), mixed=False)
    refs = [opx, olk, torch.softmax(opx, -1), _p_link(olk)]
    worst = _report("PixelLinkNet %d^2 n=%d" % (size, n), outs, refs, ["pixel_cls", "link_cls", "P(text)", "P(link)"])
    assert worst < 1e-3


SMALL = [("block1", [(128, 64, 1), (128, 64, 2)]), ("block2", [(256, 64, 1), (256, 64, 2)]),
         ("block3", [(256, 128, 1), (256, 128, 2)]), ("block4", [(512, 128, 1)])]


@pytest.mark.parametrize("blocks", [SMALL, None], ids=["small_128", "resnet50_64"])
def test_model_east_f16x2_within_1e3(device, blocks):
    """ResNet-v1-50 EAST `model` as tests/test_gpu_f32_verify.py::test_model_east_score_geometry_within_1e3 sets it up."""
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    rng = np.random.default_rng(4)
    p = O.init_model_east_params(rng, blocks)
    images, _, _, _ = O.synthetic_batch(rng, 2, 64 if blocks is None else 128)

    def build(g, im):
        fs, geo = M.model(im, graph=g, blocks=blocks)
        return [fs.data, geo.data]
    outs = _both_routes(device, build, images, images, p)
    with torch.no_grad():
        ofs, ogeo, _ = O.model_east(torch.from_numpy(images), O.to_torch_params(p), True, mixed=False, blocks=blocks)
    worst = _report("EAST %s" % ("full" if blocks is None else "small"), outs, [ofs, ogeo], ["F_score", "geo_map"])
    assert worst < 1e-3


def test_graphed_f16x2_forward_equals_eager(device):
    """A captured f16x2 model_vgg forward replays bit for bit what the launches give one by one, on two input batches and
    after a checkpoint restore (stale packed weights or a pointer baked at capture would show)."""
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.infer import GraphedForward
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    rng = np.random.default_rng(7)

    def fn(gr, x):
        px, lk = M.model_vgg(x, is_training=False, graph=gr)
        return px.data, lk.data
    ge, gg = Graph(device, seed=3, precision="f16x2"), Graph(device, seed=3, precision="f16x2")
    fwd = GraphedForward(gg, fn, capture_after=0)

    def eager(x):
        out = fn(ge, x)
        ge.reset_tape()
        return [o.clone() for o in out]
    for i in range(3):
        if i == 2:
            sd = {k: v * 0.5 for k, v in ge.store.state_dict().items()}
            ge.store.load_state_dict(sd)
            gg.store.load_state_dict(sd)
        x = torch.from_numpy(rng.uniform(0, 255, (2, 64, 96, 3)).astype(np.float32)).to(device)
        want = eager(x)
        got = fwd(x)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), i
        assert float(want[0].abs().sum()) > 0 and bool(torch.isfinite(want[1]).all())
    assert len(fwd.cache) == 1


def test_f16x2_interface(device, monkeypatch):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.graph import Graph
    g = Graph(device, precision="f16x2")
    with pytest.raises(NotImplementedError):
        g.backward()
    with pytest.raises(ValueError):
        Graph(device, precision="f8")
    assert Graph(device, precision="f32").f32_conv_route is None and g.f32_conv_route == "split"
    # route=None still means ops.F32_CONV
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((1, 12, 12, 32)).astype(np.float32)).to(device)
    wt = torch.from_numpy(rng.standard_normal((3, 3, 32, 40)).astype(np.float32)).to(device)
    d = ops.conv_desc((1, 12, 12, 32), 40, 3, 3, 1, 1)
    d.flags = 0
    ya, yb = (torch.zeros((1, d.oh, d.ow, 40), dtype=torch.float32, device=device) for _ in range(2))
    monkeypatch.setattr(ops, "F32_CONV", "direct")
    ops.conv2d_f32(d, x, wt, ya, None, route=None)
    ops.conv2d_f32(d, x, wt, yb, None, route="direct")
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and float(ya.abs().sum()) > 0


def test_f32_graph_under_split_route_equals_f16x2(device, monkeypatch):
    """OCR_F32_CONV=split (ops.F32_CONV) turns a Graph(precision="f32") — what test_pixellink.py / test_pixellink_fast.py
    --precision f32 build — into the f16x2 computation: same launches, same bits."""
    from tensorflow_ocr_amd import checkpoint, ops
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    rng = np.random.default_rng(5)
    p = O.init_pixellink_params(rng)
    images, _, _, _ = O.synthetic_batch(rng, 2, 64)
    x = ((images - 120.0) / 60.0).astype(np.float32)
    outs = []
    for prec, env in (("f16x2", "mfma"), ("f32", "split"), ("f32", "mfma")):
        monkeypatch.setattr(ops, "F32_CONV", env)
        g = Graph(device, precision=prec)
        pixellink.PixelLinkNet(x, graph=g)
        g.reset_tape()
        g.store.load_state_dict(checkpoint.tf_to_internal(g.store.order, p))
        net = pixellink.PixelLinkNet(x, graph=g)
        outs.append((net.pixel_cls.data.clone(), net.link_cls.data.clone()))
        g.reset_tape()
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][1], outs[2][1])             # ... and it is not the mfma route under another name


def test_mfma_honours_half_subnormals_on_its_inputs(device):
    """Direct probe of what DESIGN.md section 4 states: one half-subnormal operand (2^-20: exactly representable, hi plane
    only, residual 0) times 1.0 through v_mfma_f32_16x16x32_f16 comes out as 2^-20, not 0 — on the A input (weights) and on
    the B input (activations).  The accuracy bars above hold either way; this pins the documented hardware fact."""
    from tensorflow_ocr_amd import ops
    tiny = np.float32(2.0 ** -20)
    for x_val, w_val in ((tiny, np.float32(1.0)), (np.float32(1.0), tiny)):
        x = torch.zeros((1, 4, 4, 8), dtype=torch.float32, device=device)
        x[..., 3] = float(x_val)
        wt = torch.zeros((1, 1, 8, 16), dtype=torch.float32, device=device)
        wt[0, 0, 3, :] = float(w_val)
        d = ops.conv_desc((1, 4, 4, 8), 16, 1, 1, 1, 1)
        d.flags = 0
        y = torch.full((1, 4, 4, 16), -1.0, dtype=torch.float32, device=device)
        ops.conv2d_f32(d, x, wt, y, None, route="split")
        torch.cuda.synchronize()
        print("subnormal half on %s: 2^-20 * 1 -> %.6e (2^-20 = %.6e)" % ("B (x)" if x_val == tiny else "A (w)", float(y[0, 0, 0, 0]), float(tiny)))
        assert bool((y == float(tiny)).all())


def test_nan_operand_is_not_made_finite(device):
    """The saturation of out-of-range operands must not swallow NaN: the outputs a NaN activation reaches are NaN, as on the
    f32 MFMA route; the others stay finite."""
    from tensorflow_ocr_amd import ops
    rng = np.random.default_rng(13)
    x = torch.from_numpy(rng.standard_normal((1, 8, 8, 16)).astype(np.float32)).to(device)
    x[0, 0, 0, 5] = float("nan")
    wt = torch.from_numpy(rng.standard_normal((3, 3, 16, 24)).astype(np.float32)).to(device)
    d = ops.conv_desc((1, 8, 8, 16), 24, 3, 3, 1, 1)
    d.flags = 0
    ys = {}
    for route in ("split", "mfma"):
        ys[route] = torch.zeros((1, 8, 8, 24), dtype=torch.float32, device=device)
        ops.conv2d_f32(d, x, wt, ys[route], None, route=route)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(ys["split"]), torch.isnan(ys["mfma"]))
    assert bool(torch.isnan(ys["split"][0, :2, :2]).all()) and bool(torch.isfinite(ys["split"][0, 4:]).all())
