"""GPU: training summaries (summary.TensorStats / ocr_tensor_stats_f32, ocr_summary_image_u8, the event file the
training scripts write).

The reference is a NumPy float64 restatement written here: the f32 products x * (mul_host * mul_dev) are formed in
NumPy's float32, a finite product goes to bucket np.searchsorted(limits, float64(v), side='right'), inf / NaN are
counted apart.  num, nonfinite, min, max and every bucket must be EQUAL; sum and sum_squares must lie within
n * 2^-52 * sum(|term|) of NumPy's float64 sums — the reordering bound of float64 addition (two orders of the same n
terms differ by at most 2 (n - 1) u sum|term|, u = 2^-53; the terms themselves, float64(v) and its square rounded once,
are the same in both) — derived, not measured.  Whole training steps must not notice a summary pass."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PAD = F32(1e30)                       # what the words between segments hold: counted nowhere
SENT = 0x5A5A5A5A5A5A5A5A
GUARD = 16                            # 8-byte words on either side of the records and of the workspace


def _limits():
    from tensorflow_ocr_amd import summary
    return summary.bucket_limits()


def _reference(v):
    """The record of the f32 products `v` (one segment), in float64."""
    lim = _limits()
    fin = np.isfinite(v)
    d = v[fin].astype(np.float64)
    return {"num": int(fin.sum()), "nonfinite": int((~fin).sum()),
            "min": float(d.min()) if d.size else 0.0, "max": float(d.max()) if d.size else 0.0,
            "sum": float(d.sum()), "sum_squares": float((d * d).sum()),
            "abs_sum": float(np.abs(d).sum()),
            "bucket": np.bincount(np.searchsorted(lim, d, side="right"), minlength=lim.size).astype(np.uint32)}


def _check(rec, ref, what):
    n = ref["num"]
    print("%s: num %d nonfinite %d min %r max %r sum %r (ref %r) sum_squares %r (ref %r)" % (
        what, rec["num"], rec["nonfinite"], rec["min"], rec["max"], rec["sum"], ref["sum"], rec["sum_squares"],
        ref["sum_squares"]))
    assert rec["num"] == n and rec["nonfinite"] == ref["nonfinite"], what
    assert rec["min"] == ref["min"] and rec["max"] == ref["max"], what
    assert rec["bucket"].shape == ref["bucket"].shape and np.array_equal(rec["bucket"], ref["bucket"]), what
    assert int(rec["bucket"].sum()) == n, what
    assert abs(rec["sum"] - ref["sum"]) <= n * 2.0 ** -52 * ref["abs_sum"], what
    assert abs(rec["sum_squares"] - ref["sum_squares"]) <= n * 2.0 ** -52 * ref["sum_squares"], what


def _special_values():
    """±0, denormals, values below 1e-12, ±3e38, inf, NaN, and for a dozen limits L float32(L) with its two neighbours,
    either sign."""
    lim = _limits()
    pos = lim[lim > 0][:-1]
    picks = pos[[0, 1, 57, 131, 200, 289, 290, 291, 400, 512, 640, 773]]           # within float32's range: 1e-12 .. 1e20
    vals = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 1e-13, -1e-13, 9.99e-13, -9.99e-13, 1e-12, -1e-12,
            3e38, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 1024.0, -1024.0]
    for L in picks:
        c = F32(L)
        for x in (np.nextafter(c, F32(0)), c, np.nextafter(c, F32(np.inf))):
            vals += [x, -x]
    return np.array(vals, dtype=F32)


@pytest.fixture(scope="module")
def layout(device):
    """One flat buffer: segments of 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 3 * chunk + 7 elements, each padded to a
    multiple of 4 as the variable store does, the pad words holding 1e30.  Built once and never written again."""
    from tensorflow_ocr_amd import ops
    chunk = ops.tensor_stats_chunk()
    sizes = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]
    rng = np.random.default_rng(11)
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += (s + 3) // 4 * 4
    x = np.full(o + 8, PAD, dtype=F32)
    sp = _special_values()
    for k, (off, s) in enumerate(zip(offs, sizes)):
        # mixed signs over many decades, so that hundreds of buckets are hit
        v = (rng.standard_normal(s) * 10.0 ** rng.uniform(-14, 6, size=s)).astype(F32)
        if s >= sp.size:
            at = rng.choice(s, size=sp.size, replace=False)
            v[at] = sp
            v[0], v[-1] = sp[k % sp.size], sp[(k + 5) % sp.size]                   # specials on the head and the tail too
        x[off:off + s] = v
    x[offs[0]] = F32(-0.0)
    x[offs[1]:offs[1] + 3] = [np.inf, 1e-45, np.nan]
    x[offs[2]:offs[2] + 4] = [np.nan, np.inf, -np.inf, np.nan]                     # a segment with no finite element
    x.setflags(write=False)
    return {"chunk": chunk, "sizes": sizes, "offs": offs, "x": x, "dev": torch.from_numpy(x.copy()).to(device)}


class _Run:
    """Table, records and workspace for the given segments, records and workspace between sentinel guard bands."""

    def __init__(self, device, offs, sizes):
        from tensorflow_ocr_amd import ops, summary
        self.n = len(offs)
        table, self.n_chunks = ops.tensor_stats_table(offs, sizes)
        self.table = torch.from_numpy(table.view(np.int64)).to(device)
        self.rec_words = self.n * summary.RECORD_DTYPE.itemsize // 8
        self.ws_words = ops.tensor_stats_workspace(self.n_chunks) // 8
        sent = torch.tensor(SENT, dtype=torch.int64)
        self._r = sent.repeat(GUARD + self.rec_words + GUARD).to(device)
        self._w = sent.repeat(GUARD + self.ws_words + GUARD).to(device)
        self.records = self._r[GUARD:GUARD + self.rec_words]
        self.ws = self._w[GUARD:GUARD + self.ws_words]

    def run(self, x, mul_host=1.0, mul_dev=None):
        from tensorflow_ocr_amd import ops, summary
        ops.tensor_stats(x, self.table, self.n, mul_host, mul_dev, self.records, self.ws)
        raw = self.records.cpu().numpy().copy()
        for band in (self._r[:GUARD], self._r[GUARD + self.rec_words:], self._w[:GUARD], self._w[GUARD + self.ws_words:]):
            assert bool((band == SENT).all()), "a guard band was written"
        return raw, [summary.record_dict(r) for r in raw.view(summary.RECORD_DTYPE)]


def _products(x, mul_host, mul_dev):
    mul = F32(mul_host) * (F32(1) if mul_dev is None else F32(mul_dev))
    with np.errstate(all="ignore"):
        return x * mul


@pytest.mark.parametrize("mul_host,mul_dev", [(1.0, None), (1.0 / 1024, None), (1.0, 0.75), (1.0 / 1024, 3.0)])
def test_records_equal_numpy(device, layout, mul_host, mul_dev):
    r = _Run(device, layout["offs"], layout["sizes"])
    assert r.n_chunks == sum((s + layout["chunk"] - 1) // layout["chunk"] for s in layout["sizes"])
    md = None if mul_dev is None else torch.tensor([mul_dev], dtype=torch.float32, device=device)
    raw1, recs = r.run(layout["dev"], mul_host, md)
    v = _products(layout["x"], mul_host, mul_dev)
    for k, (off, s) in enumerate(zip(layout["offs"], layout["sizes"])):
        _check(recs[k], _reference(v[off:off + s]), "segment %d (size %d)" % (k, s))
    assert recs[2]["num"] == 0 and recs[2]["nonfinite"] == 4 and recs[2]["min"] == 0.0 and recs[2]["max"] == 0.0
    assert sum(x["nonfinite"] for x in recs) >= 10 and (recs[7]["bucket"] > 0).sum() > 300
    raw2, _ = r.run(layout["dev"], mul_host, md)
    assert raw1.tobytes() == raw2.tobytes()                   # bitwise reproducible, the f64 sums included


def test_unaligned_segments_through_the_raw_abi(device, layout):
    chunk = layout["chunk"]
    offs = [1, 6, chunk + 3, 2]                                # any offset, overlapping or not, in any order
    sizes = [6, 1, 2 * chunk + 5, chunk + 1]
    r = _Run(device, offs, sizes)
    x = layout["dev"]
    _, recs = r.run(x)
    for k, (off, s) in enumerate(zip(offs, sizes)):
        _check(recs[k], _reference(layout["x"][off:off + s]), "segment %d (offset %d)" % (k, off))
    # and a view that itself starts off the 16-byte grid
    _, recs = r.run(x[1:])
    for k, (off, s) in enumerate(zip(offs, sizes)):
        _check(recs[k], _reference(layout["x"][1 + off:1 + off + s]), "shifted segment %d" % k)


def test_a_workspace_too_small_for_the_table_is_refused(device, layout):
    from tensorflow_ocr_amd import _lib, ops, summary
    r = _Run(device, layout["offs"], layout["sizes"])
    with pytest.raises(_lib.OcrHipError):                      # below one partial per segment: the host can tell
        ops.tensor_stats(layout["dev"], r.table, r.n, 1.0, None, r.records, r.ws[:4 * (r.n - 1)])
    # enough for n_segments but not for the table's chunks: only the device can tell; nothing is touched through it
    ops.tensor_stats(layout["dev"], r.table, r.n, 1.0, None, r.records, r.ws[:4 * r.n])
    raw = r.records.cpu().numpy().view(summary.RECORD_DTYPE)
    assert (raw["nonfinite"] == 0xFFFFFFFF).all() and (raw["num"] == 0).all() and not raw["bucket"].any()
    assert bool((r._w == SENT).all())
    with pytest.raises(RuntimeError):
        summary.record_dict(raw[0])


def _image_rule(x):
    fin = x[np.isfinite(x)]
    mn, mx = F32(fin.min()), F32(fin.max())
    if mn < 0:
        m = max(abs(mn), abs(mx))
        scale, offset = (F32(0) if m < F32(1e-6) else F32(127) / m), F32(128)
    else:
        scale, offset = (F32(0) if mx < F32(1e-6) else F32(255) / mx), F32(0)
    return ((x * scale).astype(F32) + offset).astype(F32).astype(np.uint8)


@pytest.mark.parametrize("kind", ["non_negative", "signed"])
def test_image_rule_equals_numpy(device, kind):
    from tensorflow_ocr_amd import summary
    rng = np.random.default_rng(3)
    if kind == "non_negative":
        x = rng.uniform(0, 7.3, size=(37, 53, 1)).astype(F32)
        x[0, 0, 0] = 0.0
    else:
        x = (rng.standard_normal((61, 45, 3)) * 40).astype(F32)
    out = summary.ImageSummary(device).u8(torch.from_numpy(x).to(device))
    ref = _image_rule(x)
    assert out.dtype == np.uint8 and out.shape == x.shape and np.array_equal(out, ref)
    assert (ref.min() == 0 and ref.max() >= 254) if kind == "non_negative" else (ref.min() >= 1 and ref.max() > 200)


# --------------------------------------------------------------------------- whole training steps
def _make(device, loss_scale=1024.0, clip_norm=None, accumulate_steps=1):
    """The smallest graph tests/test_gpu_train_step.py builds: model_vgg at 64 x 64, batch 2, recorded steps."""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph, parse_loss_scale
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=parse_loss_scale(loss_scale) if isinstance(loss_scale, str) else loss_scale, seed=3)
    rng = np.random.default_rng(5)
    batch = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(rng, 2, 64)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, batch, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3, clip_norm=clip_norm),
                               accumulate_steps=accumulate_steps)


def _state(g, s):
    out = {"flat": g.store.flat, "aux": g.store.flat_aux, "m": s.opt.m, "v": s.opt.v, "ema": s.opt.ema,
           "grad": g.store.flat_grad}
    if g.loss_scaler is not None:
        out["loss_scale_state"] = g.loss_scaler.state
    if s.opt.clip is not None:
        out["clip_state"] = s.opt.clip.state
    return {k: t.detach().cpu().numpy().copy() for k, t in out.items()}


def _device_factor(g, s):
    """The optimiser's factor of the step just taken, read back from the device states (float32)."""
    from tensorflow_ocr_amd import ops
    gs = s._grad_scale()
    if s.opt.clip is not None:
        return s.opt.clip.state.cpu().numpy()[ops.GC_G_MUL:ops.GC_G_MUL + 1].view(F32)[0]
    if g.loss_scaler is not None:
        return F32(gs) * g.loss_scaler.state.cpu().numpy()[ops.LS_INV_SCALE_USED:ops.LS_INV_SCALE_USED + 1].view(F32)[0]
    return F32(gs / g.loss_scale)


@pytest.mark.parametrize("mode", ["static", "dynamic", "dynamic_clip_accum2"])
def test_training_steps_do_not_notice_the_summary_pass(device, mode):
    from tensorflow_ocr_amd import summary
    kw = {"static": {}, "dynamic": {"loss_scale": "dynamic"},
          "dynamic_clip_accum2": {"loss_scale": "dynamic", "clip_norm": 0.5, "accumulate_steps": 2}}[mode]
    K = kw.get("accumulate_steps", 1)
    ga, ba, sa = _make(device, **kw)
    gb, bb, sb = _make(device, **kw)
    var_stats = grad_stats = None
    for step in range(1, 7):                          # optimiser steps; recorded from the third call on
        for _ in range(K):
            la, lb = sa(*ba), sb(*bb)
        assert sa.closes_window and sb.closes_window
        if step % 2 == 0:
            if var_stats is None:
                var_stats, grad_stats = summary.TensorStats(ga.store), summary.TensorStats(ga.store)
            var_stats.run(ga.store.flat)
            mul_host, mul_dev = sa.summary_factor()
            grad_stats.run(ga.store.flat_grad, mul_host, mul_dev)
            varis, grads = var_stats.read(), grad_stats.read()
            factor = _device_factor(ga, sa)
            with np.errstate(all="ignore"):
                gp = ga.store.flat_grad.cpu().numpy() * F32(factor)
            wp = ga.store.flat.cpu().numpy()
            base = ga.store.flat.data_ptr()
            for v in ga.store.trainable():
                off = (v.data.data_ptr() - base) // 4
                _check(grads[v.name], _reference(gp[off:off + v.size]), "%s gradient, step %d" % (v.name, step))
                _check(varis[v.name], _reference(wp[off:off + v.size]), "%s, step %d" % (v.name, step))
            assert set(grads) == {v.name for v in ga.store.trainable()}
    assert sa.plan is not None and sb.plan is not None and len(sa.plan) == len(sb.plan)
    assert len(sa.recorded) == len(sb.recorded)
    assert la.item() == lb.item()
    a, b = _state(ga, sa), _state(gb, sb)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert sa.opt.global_step == sb.opt.global_step == 6


# --------------------------------------------------------------------------- the script
def test_multigpu_train_writes_an_event_file(device, tmp_path, capsys):
    from tensorflow_ocr_amd import summary
    sys.path.insert(0, ROOT)
    mod = importlib.import_module("multigpu_train")
    ck = os.path.join(str(tmp_path), "ckpt")
    old = sys.argv
    sys.argv = ["multigpu_train.py", "--gpu_list", "0", "--batch_size_per_gpu", "2", "--input_size", "64", "--max_steps", "3",
                "--net", "model_vgg", "--training_data_path", os.path.join(str(tmp_path), "no_such_directory"),
                "--checkpoint_path", ck, "--save_summary_steps", "1", "--summary_variables", "--clip_norm", "1.0"]
    try:
        mod.main()
    finally:
        sys.argv = old
    capsys.readouterr()
    files = [f for f in os.listdir(ck) if f.startswith("events.out.tfevents.")]
    assert len(files) == 1
    events = summary.read_events(os.path.join(ck, files[0]))
    assert events[0].get("file_version") == "brain.Event:2" and not events[0]["values"]
    assert [e["step"] for e in events[1:]] == [1, 2, 3]
    # the trainable variables of the same net, from a graph of this test's own (tags carry the store's names)
    g, batch, step = _make(device)
    step.build(*batch)
    sizes = {v.name: v.size for v in g.store.trainable()}
    names = list(sizes)
    assert len(names) > 20 and "conv1/conv1_1/weights" in names
    for e in events[1:]:
        by_tag = {v["tag"]: v for v in e["values"]}
        assert len(by_tag) == len(e["values"])
        for tag in ("model_loss", "total_loss", "learning_rate", "grad_norm"):
            assert np.isfinite(by_tag[tag]["simple_value"])
        for tag, (h, w, c) in (("input", (64, 64, 3)), ("score_map", (16, 16, 1)), ("geo_map_0", (16, 16, 1))):
            im = by_tag[tag]["image"]
            assert (im["height"], im["width"], im["colorspace"]) == (h, w, c)
            assert summary.decode_png(im["encoded_image_string"]).shape == (h, w, c)
        for n in names:
            t = summary.variable_tags(n)
            for key in ("grad_histogram", "var_histogram"):
                hist = by_tag[t[key]]["histo"]
                assert hist["num"] == float(sizes[n]) and sum(hist["bucket"]) == hist["num"]
                assert len(hist["bucket"]) == len(hist["bucket_limit"])
            assert "simple_value" in by_tag[t["ratio"]] and "simple_value" in by_tag[t["var_mean"]]
            assert by_tag[t["nonfinite"]]["simple_value"] == 0.0
        assert len(by_tag) == 4 + 3 + 5 * len(names)
