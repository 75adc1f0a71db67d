"""CPU: host side of gradient accumulation — `accumulate_steps` validation on `TrainStep`, the training scripts'
`--accumulate_steps` flag, the C ABI's declarations and exports, the three rules as torch operators (the gloo path) against
NumPy float32, and a two-rank gloo run of the bucketed exchange with K = 2.  (The device rules and whole steps:
tests/test_gpu_grad_accum.py.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ocr_grad_accum_init", "ocr_grad_accum_f32", "ocr_grad_accum_advance"]


def test_accumulate_steps_is_validated_before_anything_is_allocated():
    from tensorflow_ocr_amd import graph as G
    from tensorflow_ocr_amd.train import TrainStep, check_accumulate_steps
    made = []

    def factory(gr):
        made.append(gr)
        raise AssertionError("the optimiser factory must not run")
    for bad in (0, -1, 2.5, "2", None, True):
        with pytest.raises(ValueError):
            TrainStep(G.Graph("cpu"), lambda *a: None, factory, accumulate_steps=bad)
        with pytest.raises(ValueError):
            check_accumulate_steps(bad)
    assert not made
    for ok in (1, 2, np.int64(7)):
        st = TrainStep(G.Graph("cpu"), lambda *a: None, factory, accumulate_steps=ok)
        assert st.accumulate_steps == int(ok) and st.accum is None and st.opt is None      # nothing allocated yet
        assert st.micro_step == 0 and st.closes_window is False and st.steps == 0
    assert TrainStep(G.Graph("cpu"), lambda *a: None, factory).accumulate_steps == 1         # off by default
    assert not made


@pytest.mark.parametrize("script", ["multigpu_train", "train_pixellink"])
def test_scripts_parse_the_accumulate_steps_flag(script):
    import importlib
    mod = importlib.import_module(script)
    assert mod.parse([]).accumulate_steps == 1                                # off by default
    v = mod.parse(["--accumulate_steps", "4"]).accumulate_steps
    assert isinstance(v, int) and v == 4
    assert mod.parse(["--accumulate_steps", "1", "--clip_norm", "2"]).accumulate_steps == 1
    for bad in ("0", "-1", "2.5", "two", ""):
        with pytest.raises(SystemExit):
            mod.parse(["--accumulate_steps", bad])


def test_header_declares_every_new_symbol_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert not [s for s in NEW_SYMBOLS if s not in declared]
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    m = re.search(r"typedef struct \{([^}]*)\}\s*ocr_grad_accum_state;", code)
    assert m
    fields = re.findall(r"\buint32_t\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert fields == [("micro", ""), ("k", ""), ("windows_total", ""), ("reserved", "5")]
    from tensorflow_ocr_amd import ops
    assert [ops.GA_MICRO, ops.GA_K, ops.GA_WINDOWS_TOTAL] == [0, 1, 2] and ops.GRAD_ACCUM_WORDS == 8


def test_both_product_libraries_export_the_new_symbols():
    import ctypes
    from tensorflow_ocr_amd import _lib
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_torch_rules_on_cpu_match_numpy_float32_bit_for_bit(K):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.train import GradAccum
    n = 1031
    rng = np.random.default_rng(K)
    grad = torch.zeros(n, dtype=torch.float32)
    ga = GradAccum(K, grad)
    assert ga.acc.shape == grad.shape and ga.state.tolist() == [0, K, 0, 0, 0, 0, 0, 0]
    ga.acc.fill_(float("nan"))                    # the first rule stores: nothing needs zeroing
    for window in range(2):
        gs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32) for _ in range(K)]
        ref = gs[0].copy()
        for m in range(K):
            assert ga.micro == m and ga.closing == (m == K - 1) and int(ga.state[ops.GA_MICRO]) == m
            grad.copy_(torch.from_numpy(gs[m]))
            acc_before = ga.acc.clone()
            # whole buffer on even windows, two unaligned slices on odd ones
            for s, e in ([(0, n)] if window == 0 else [(0, 517), (517, n)]):
                ga.run(s, e)
            if m > 0:
                ref = (ref + gs[m]).astype(np.float32)              # ((g1 + g2) + g3) + ...
            if m == K - 1:
                assert (_bits(grad.numpy()) == _bits(ref)).all()
                assert K == 1 or torch.equal(ga.acc.view(torch.int32), acc_before.view(torch.int32))     # grad only
            else:
                assert (_bits(ga.acc.numpy()) == _bits(ref)).all()
                assert (_bits(grad.numpy()) == _bits(gs[m])).all()                                        # acc only
            ga.advance()
        assert ga.micro == 0 and ga.windows() == window + 1
    if K == 1:
        assert bool(torch.isnan(ga.acc).all())    # never read, never written
    # inf / NaN in any micro-gradient reach the closing sum
    if K > 1:
        for m_bad in range(K):
            for bad in (np.inf, np.nan):
                for m in range(K):
                    grad.fill_(1.0)
                    if m == m_bad:
                        grad[7] = float(bad)
                    ga.run()
                    ga.advance()
                assert not np.isfinite(grad[7].item()) and grad[8].item() == K
    ga.advance()
    ga.reset()
    assert ga.micro == 0 and ga.state.tolist() == [0, K, 0, 0, 0, 0, 0, 0]


_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as td
from tensorflow_ocr_amd import dist
from tensorflow_ocr_amd.graph import VariableStore, constant
from tensorflow_ocr_amd.train import GradAccum
rank, world, _ = dist.init_process_group_from_env("gloo")
st = VariableStore(torch.device("cpu"))
a = st.get("a/weights", (3, 3, 2, 4), constant(1.0), regularized=True)
b = st.get("b/weights", (5, 7), constant(2.0), regularized=True)
c = st.get("a/BatchNorm/gamma", (4,), constant(1.0))
st.materialise()
K = 2
ga = GradAccum(K, st.flat_grad)
red = dist.GradientAllReduce(st, world, bucket_bytes=64 * 4, op="mean", fold_mean=True, accum=ga)
assert len(red.buckets) >= 2 and red.mode == "torch"
calls = []
real = td.all_reduce
def counted(*args, **kw):
    calls.append(1)
    return real(*args, **kw)
td.all_reduce = counted
n = st.flat_grad.numel()
def micro_grad(r, w, m):                     # rank r, window w, micro-step m
    return torch.from_numpy(np.random.default_rng(100 * r + 10 * w + m).standard_normal(n).astype(np.float32))
for w in range(3):
    for m in range(K):
        st.flat_grad.copy_(micro_grad(rank, w, m))
        red.closing = ga.closing
        assert red.closing == (m == K - 1)
        before = len(calls)
        red.on_grads_ready([b]); red.on_grads_ready([a, c])          # reverse creation order
        red.finish()
        ga.advance()
        if m < K - 1:
            assert len(calls) == before, "a micro-step inside its window exchanged"
            assert torch.equal(st.flat_grad, micro_grad(rank, w, m))      # acc only
        else:
            assert len(calls) - before == len(red.buckets), (len(calls) - before, len(red.buckets))
    # fold_mean: the SUM over ranks of the sequential sums is in the buffer; times grad_scale = the rank mean
    per_rank = [micro_grad(r, w, 0) + micro_grad(r, w, 1) for r in range(world)]
    want = per_rank[0].clone()
    for t in per_rank[1:]:
        want = want + t
    assert torch.equal(st.flat_grad, want), (w, (st.flat_grad - want).abs().max())
    mean = st.flat_grad * red.grad_scale
    assert torch.equal(mean, want * (1.0 / world))
assert len(calls) == 3 * len(red.buckets)    # one all-reduce per bucket and WINDOW, not per call
assert ga.windows() == 3 and ga.micro == 0
td.barrier(); td.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gradient_allreduce_accumulates_world2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER % ROOT)
    import socket

    def launch():
        with socket.socket() as sk:                  # a port nobody holds right now
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        ps = []
        for r in range(2):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            ps.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT))
        try:
            return ps, [p.communicate(timeout=120)[0].decode() for p in ps]
        except subprocess.TimeoutExpired:
            for p in ps:
                p.kill()
            return ps, None
    procs, outs = launch()
    if outs is None:
        procs, outs = launch()                       # one more try on a fresh port
    assert outs is not None, "two-rank rendezvous timed out twice"
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


def test_scheduler_keeps_accumulate_entries_behind_their_weight_gradients_and_in_front_of_their_exchange():
    """schedule_guests holds weight gradients back as hosts for the batch-norm guests: a bucket's accumulate entry reads
    every weight gradient recorded before it and is read by the bucket's exchange entries, in every placement."""
    from tensorflow_ocr_amd.train import schedule_guests

    def c(name, tag):
        return ["c", None, (0, 0), name, tag]
    rec = []
    for layer in range(6):
        rec += [c("pre%d" % layer, ("pre",)), c("guest%d" % layer, ("guest", 4.0e8)), c("dgrad%d" % layer, None),
                c("wgrad%d" % layer, ("side", 2.0e11)), c("sum%d" % layer, ("reduce",))]
        if layer % 2 == 1:                      # this weight gradient completed a bucket
            rec += [c("accum%d" % layer, ("accum",)), c("record%d" % layer, ("xchg", None, None)),
                    c("allreduce%d" % layer, ("xchg", "rccl", None))]
    rec += [c("bias", None), c("accum_last", ("accum",)), c("allreduce_last", ("xchg", "rccl", None)),
            c("wait", ("xchg", "finish", None)), c("advance", ("accum", "advance")), ["py", lambda: None, "opt"]]
    is_w = lambda e: e[0] == "c" and e[4] is not None and e[4][0] in ("side", "reduce")
    for kw in (dict(), dict(xchg_at_fork=False), dict(balance=False), dict(min_us=0.0), dict(min_us=0.0, xchg_at_fork=False),
               dict(min_us=1e9)):
        plan = schedule_guests(rec, **kw)
        pos = {id(e): i for i, e in enumerate(plan)}
        assert len(pos) >= len(rec) - 6 and all(id(e) in pos for e in rec if e[0] != "c" or e[4] is None or e[4][0] != "guest")
        seen_w, last_accum = [], None
        for e in rec:
            if is_w(e):
                seen_w.append(e)
            elif e[0] == "c" and e[4] is not None and e[4][0] == "accum":
                assert all(pos[id(w)] < pos[id(e)] for w in seen_w), (kw, e[3])
                if last_accum is not None:
                    assert pos[id(last_accum)] < pos[id(e)], (kw, e[3])
                last_accum = e
            elif e[0] == "c" and e[4] is not None and e[4][0] == "xchg":
                assert pos[id(last_accum)] < pos[id(e)], (kw, e[3])
        assert pos[id(rec[-2])] < pos[id(rec[-1])] and plan[-1] is rec[-1]
    # without accumulation the same recording is scheduled as before: the entries that are left keep their order
    plain = [e for e in rec if not (e[0] == "c" and e[4] is not None and e[4][0] == "accum")]
    a = [e[3] for e in schedule_guests(plain) if e[0] == "c"]
    b = [e[3] for e in schedule_guests(rec) if e[0] == "c" and not e[3].startswith(("accum", "advance"))]
    assert a == b


def test_eager_windows_on_the_cpu_step_once_per_window_with_the_mean_gradient():
    """TrainStep's control flow with everything on the CPU (torch closures on the tape, an optimiser made of torch
    operators): K - 1 calls change nothing but the second buffer, the closing call hands the sequential sum and
    grad_scale / K to the optimiser."""
    from tensorflow_ocr_amd import graph as G
    from tensorflow_ocr_amd.train import TrainStep
    K = 3
    applied = []

    class Sgd:
        def __init__(self, g):
            g.ensure_materialised()
            self.g, self.global_step = g, 0

        def apply_gradients(self, grad_scale=1.0):
            st = self.g.store
            applied.append((st.flat_grad.clone(), grad_scale))
            st.flat.sub_(st.flat_grad * grad_scale)
            st.version += 1
            self.global_step += 1

    def forward_loss(g, x):
        w = g.get_variable("w", (8,), G.constant(1.0))      # (a multiple of four: no padding in the flat buffer)

        def bwd():
            w.grad.copy_(x)                      # backward OVERWRITES the gradient buffer
        g.record(bwd, produces=(w,))
        return x.sum()
    g = G.Graph("cpu")
    step = TrainStep(g, forward_loss, Sgd, replay=False, accumulate_steps=K)
    xs = [torch.from_numpy(np.random.default_rng(i).standard_normal(8).astype(np.float32)) for i in range(2 * K + 1)]
    for i, x in enumerate(xs[:2 * K]):
        assert step.micro_step == i % K
        w_before = None if step.opt is None else g.store.flat.clone()
        step(x)
        assert step.steps == i + 1 and step.closes_window == (i % K == K - 1)
        assert step.opt.global_step == (i + 1) // K == len(applied) == g.store.version
        if not step.closes_window and w_before is not None:
            assert torch.equal(g.store.flat, w_before)
    for w in range(2):
        want = (xs[K * w] + xs[K * w + 1]) + xs[K * w + 2]
        assert torch.equal(applied[w][0].view(torch.int32), want.view(torch.int32)) and applied[w][1] == 1.0 / K
    assert step.accum.windows() == 2 and step.accum.micro == 0
    # reset_window in the middle of a window: the next K calls are a fresh window
    step(xs[-1])
    assert step.micro_step == 1
    step.reset_window()
    assert step.micro_step == 0 and step.accum.micro == 0 and step.accum.windows() == 0
    for x in xs[:K]:
        step(x)
    assert step.closes_window and torch.equal(applied[2][0], applied[0][0]) and step.opt.global_step == 3
    # K = 1: the plain step, nothing allocated
    applied.clear()
    plain = TrainStep(G.Graph("cpu"), forward_loss, Sgd, replay=False)
    plain(xs[0])
    assert plain.accum is None and plain.closes_window and applied[0][1] == 1.0 and torch.equal(applied[0][0], xs[0])
