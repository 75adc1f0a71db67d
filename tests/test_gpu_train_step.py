"""GPU: the full training step (forward, dice loss, backward, Adam+EMA) — eager vs recorded/replayed
execution must agree bit for bit (every kernel is deterministic: slab reductions, no atomics), the
Adam update must match the oracle's formula on the device gradients, and the loss must go down."""
import os

import numpy as np
import pytest
import torch

from oracle import ocr_oracle as O

pytestmark = pytest.mark.gpu


def _make(device, replay):
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    g = Graph(device, loss_scale=1024.0, seed=3)
    rng = np.random.default_rng(5)
    batch = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(rng, 2, 64)]

    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, batch, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3), replay=replay)


@pytest.mark.parametrize("batch_heads", [True, False])
def test_replay_equals_eager_bitwise(device, batch_heads, monkeypatch):
    from tensorflow_ocr_amd import head_layers
    # both head forms: one launch per kernel kind over the sources (head_layers.head_group, the default) and the per-source
    # convolutions (head_layers.head_conv_bn)
    monkeypatch.setattr(head_layers, "BATCH_HEADS", batch_heads)
    ge, be, se = _make(device, False)
    gr, br, sr = _make(device, True)
    le, lr = [], []
    for i in range(7):
        le.append(se(*be).item())
        lr.append(sr(*br).item())
    assert sr.plan is not None and se.plan is None
    assert le == lr, (le, lr)
    assert le[-1] < le[0]
    assert torch.equal(ge.store.flat, gr.store.flat)
    assert torch.equal(ge.store.flat_aux, gr.store.flat_aux)
    # fresh data goes through the recorded input buffers
    rng = np.random.default_rng(9)
    from tensorflow_ocr_amd import synthetic
    nb = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(rng, 2, 64)]
    assert se(*nb).item() == sr(*nb).item()


def _make_pixellink(device, replay, normalise_inside=False):
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.train import MomentumOptimizer, TrainStep
    g = Graph(device, seed=4)

    def fl(gr, im, px, lk):
        net = pixellink.PixelLinkNet((im - 120.0) / 60.0 if normalise_inside else im, graph=gr)
        return net.build_loss(px, lk)
    return g, TrainStep(g, fl, lambda gr: MomentumOptimizer(gr, base_lr=1e-3), replay=replay)


def _pixellink_batch(device, seed):
    from tensorflow_ocr_amd import synthetic
    im, px, lk, _ = synthetic.make_batch(np.random.default_rng(seed), 2, 64)
    return [torch.from_numpy(a).to(device) for a in (im, np.ascontiguousarray(px[..., 0]), lk)]


def test_pixellink_replay_equals_eager_on_a_fresh_batch_every_step(device):
    """Every step gets new data (as the feeder delivers it) and nothing synchronises in between:
    the replayed plan must consume the new batch, not anything left over from the recorded step."""
    ge, se = _make_pixellink(device, False)
    gr, sr = _make_pixellink(device, True)
    le, lr = [], []
    for i in range(8):
        b = _pixellink_batch(device, 20 + i)
        b[0] = (b[0] - 120.0) / 60.0
        le.append(se(*b).data.clone())
        lr.append(sr(*[t.clone() for t in b]).data.clone())
        del b
        torch.empty(1 << 20, device=device).fill_(float("nan"))       # recycle freed blocks with poison
    assert sr.plan is not None and se.plan is None
    le = [v[0].item() for v in le]
    lr = [v[0].item() for v in lr]
    assert le == lr, (le, lr)
    assert all(np.isfinite(le))
    assert torch.equal(ge.store.flat, gr.store.flat)


TAIL_PLANS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_tail_plans.json")
TAIL_CASES = [(w, m) for w in ("adam", "momentum") for m in ("static", "dynamic", "clip_static", "clip_dynamic")]


def plan_names(plan):
    """A plan without its pointers: [C entry, tag] per call, [kind, label] for a fork, a join or a host callback."""
    from tensorflow_ocr_amd import step_plan
    return [[e[3], list(e[4]) if e[4] is not None else None] if e[0] == "c" else [e[0], step_plan.py_label(e)] for e in plan]


def run_tail_case(device, which, mode):
    """Both towers of one case over four batches: (the recorded plan's names, replayed step, its eager twin)."""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import DynamicLossScale, Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer, TrainStep
    clip = 1.0 if mode.startswith("clip") else None

    def tower(replay):
        g = Graph(device, loss_scale=DynamicLossScale(init_scale=1024.0) if mode.endswith("dynamic") else 1024.0, seed=3)
        if which == "adam":
            def fl(gr, im, px, lk, mk):
                a, b = M.model_vgg(im, graph=gr)
                return M.loss(px, a, lk, b, mk, graph=gr)
            return g, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3, clip_norm=clip), replay=replay)

        def fl(gr, im, px, lk):
            return pixellink.PixelLinkNet(im, graph=gr).build_loss(px, lk)
        return g, TrainStep(g, fl, lambda gr: MomentumOptimizer(gr, base_lr=1e-3, clip_norm=clip), replay=replay)
    (gr, sr), (ge, se) = tower(True), tower(False)
    for i in range(4):                                  # two eager steps, the recorded third, one replay
        if which == "adam":
            b = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(40 + i), 2, 64)]
        else:
            b = _pixellink_batch(device, 40 + i)
            b[0] = (b[0] - 120.0) / 60.0
        sr(*[t.clone() for t in b])
        se(*b)
        if i == 2:
            names = plan_names(sr.plan)
    torch.cuda.synchronize()
    return names, sr, se


@pytest.mark.parametrize("which,mode", TAIL_CASES)
def test_every_tail_mode_records_the_parents_plan_and_replays_the_eager_step(device, which, mode):
    """Both optimisers under each gradient-factor policy (constant or dynamic loss scale, with and without clip_norm): the
    third step's plan is, entry for entry and tag for tag, the one recorded on the commit before the policies were pulled
    out of the optimisers (tests/golden/train_tail_plans.json, written by tests/golden/make_train_tail_plans.py), and the
    replayed fourth step leaves the parameters of a fourth eager step, bit for bit."""
    import json
    with open(TAIL_PLANS) as f:
        gold = json.load(f)
    want = gold["plans"][gold["cases"]["%s %s" % (which, mode)]]
    names, sr, se = run_tail_case(device, which, mode)
    got = json.loads(json.dumps(names))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert len(got) == len(want)
    assert sr.plan is not None and se.plan is None and sr.opt.global_step == se.opt.global_step == 4
    assert (sr.opt.clip is not None) == mode.startswith("clip") and (sr.g.loss_scaler is not None) == mode.endswith("dynamic")
    assert torch.equal(sr.g.store.flat, se.g.store.flat) and torch.isfinite(sr.g.store.flat).all()
    assert torch.equal(sr.g.store.flat_aux, se.g.store.flat_aux)
    if sr.opt.ema is not None:
        assert torch.equal(sr.opt.ema, se.opt.ema)


def test_recording_refuses_torch_operators_inside_the_step(device):
    """A torch operator on device data inside forward_loss runs once, at record time; replay would
    read its stale output.  The recording step must raise instead of producing such a plan."""
    g, step = _make_pixellink(device, True, normalise_inside=True)
    b = _pixellink_batch(device, 1)
    step(*b)
    step(*b)                                    # eager steps are fine
    with pytest.raises(RuntimeError, match="would not be replayed"):
        step(*b)
    g2, eager = _make_pixellink(device, False, normalise_inside=True)
    for _ in range(4):
        eager(*b)                               # replay=False keeps torch operators legal


def test_adam_ema_update_matches_oracle(device):
    g, batch, step = _make(device, False)
    step(*batch)                       # creates variables + optimiser, first update
    st = g.store
    w0 = st.flat.cpu().numpy().copy()
    m0, v0 = step.opt.m.cpu().numpy().copy(), step.opt.v.cpu().numpy().copy()
    e0 = step.opt.ema.cpu().numpy().copy()
    step(*batch)
    grad = st.flat_grad.cpu().numpy() / g.loss_scale
    grad[:st.n_reg] += 1e-5 * w0[:st.n_reg]                      # slim.l2_regularizer gradient
    w1, m1, v1 = O.adam_update(w0, grad, m0, v0, 2, O.exponential_decay(1e-3, 1))
    assert np.allclose(st.flat.cpu().numpy(), w1, rtol=1e-4, atol=2e-6)
    assert np.allclose(step.opt.m.cpu().numpy(), m1, rtol=1e-4, atol=1e-7)
    d = O.ema_decay(0.997, 1)
    assert np.allclose(step.opt.ema.cpu().numpy(), e0 - (1 - d) * (e0 - w1), rtol=1e-4, atol=2e-6)


_DP_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as td
from tensorflow_ocr_amd import dist, synthetic
from tensorflow_ocr_amd.graph import Graph
from tensorflow_ocr_amd.nets import model_vgg_16 as M
from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
os.environ["LOCAL_RANK"] = "0"                      # both ranks share the single GPU of the test box
rank, world, _ = dist.init_process_group_from_env("gloo")
dev = torch.device("cuda:0")
g = Graph(dev, loss_scale=1024.0, seed=3)            # same init on every rank
rng = np.random.default_rng(50 + rank)               # different data per rank
batch = [torch.from_numpy(a).to(dev) for a in synthetic.make_batch(rng, 2, 64)]
def fl(gr, im, px, lk, mk):
    a, b = M.model_vgg(im, graph=gr)
    return M.loss(px, a, lk, b, mk, graph=gr)
step = TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3), world_size=world, bucket_bytes=8 << 20)
for i in range(6):                                   # 2 eager + 1 recorded + 3 replayed
    step(*batch)
torch.cuda.synchronize()
assert step.plan is not None and len(step.reducer.buckets) >= 2
flat = g.store.flat.detach().cpu()
ref = flat.clone()
td.broadcast(ref, src=0)
assert torch.equal(flat, ref), "ranks diverged: max diff %%g" %% (flat - ref).abs().max().item()
assert torch.isfinite(flat).all()
td.barrier(); td.destroy_process_group()
print("rank", rank, "ok")
"""


def test_data_parallel_two_ranks_stay_in_sync(device, tmp_path):
    """multigpu_train.py:70-85 semantics: after every step all towers hold identical parameters
    (mean of tower gradients).  Two ranks share the GPU through gloo — a functional check of
    TrainStep's bucketed all-reduce hooks, side streams and step replay; RCCL itself is exercised by
    the driver's multi-GPU bench."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "dp.py"
    script.write_text(_DP_WORKER % root)
    import socket

    def launch():
        with socket.socket() as sk:                  # a port nobody holds right now
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        ps = []
        for r in range(2):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            ps.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT))
        try:
            return ps, [p.communicate(timeout=180)[0].decode() for p in ps]
        except subprocess.TimeoutExpired:
            for p in ps:                             # a rendezvous that never formed: do not sit on it
                p.kill()
            return ps, None
    procs, outs = launch()
    if outs is None:
        procs, outs = launch()                       # one more try on a fresh port
    assert outs is not None, "two-rank rendezvous timed out twice"
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]


def test_momentum_update_matches_oracle(device):
    """a18: tf.train.MomentumOptimizer + slim L2 5e-4 on the regularised range
    (train_pixellink.py:222-243,267-269) as `ocr_momentum_step` applies it to the device gradients."""
    g, step = _make_pixellink(device, False)
    b = _pixellink_batch(device, 3)
    b[0] = (b[0] - 120.0) / 60.0
    step(*b)                                   # creates variables + optimiser, first update
    st, opt = g.store, step.opt
    assert opt.wd == 5e-4 and opt.momentum == 0.9
    for it in range(2):
        w0, a0 = st.flat.cpu().numpy().copy(), opt.acc.cpu().numpy().copy()
        step(*b)
        grad = st.flat_grad.cpu().numpy() / g.loss_scale
        grad[:st.n_reg] += 5e-4 * w0[:st.n_reg]
        w1, a1 = O.momentum_update(w0, grad, a0, O.pixellink_lr(opt.global_step - 1, 1e-3), 0.9)
        assert np.allclose(opt.acc.cpu().numpy(), a1, rtol=1e-5, atol=1e-8)
        assert np.allclose(st.flat.cpu().numpy(), w1, rtol=1e-6, atol=1e-8)
    assert np.abs(a1).max() > 0


def test_regularization_loss_term(device):
    """total loss = model loss + sum(REGULARIZATION_LOSSES) (multigpu_train.py:36): wd/2 * sum(w^2)
    over the regularised variables, one device reduction."""
    g, batch, step = _make(device, False)
    step(*batch)
    st = g.store
    w = st.flat[:st.n_reg].cpu().numpy().astype(np.float64)
    ref = 0.5 * 1e-5 * float((w * w).sum())
    got = step.opt.regularization_loss().item()
    assert ref > 0 and abs(got - ref) < 1e-6 * ref + 1e-12
    assert step.opt.regularization_loss().item() == got          # fixed summation order


def test_checkpoint_resume_restores_optimizer_state(device, tmp_path):
    """`Saver(tf.global_variables())` holds the Adam slots, the EMA shadows and
    global_step; a resumed tower continues bit for bit where the saved one stood."""
    from tensorflow_ocr_amd import checkpoint
    g, batch, step = _make(device, False)
    for _ in range(3):
        step(*batch)
    prefix = checkpoint.save_training_state(str(tmp_path), g, step.opt)
    assert prefix.endswith("model.ckpt-3")
    for _ in range(2):
        step(*batch)
    g2, batch2, step2 = _make(device, False)
    step2.build(*batch2)                               # variables + optimiser, no update taken
    assert step2.opt.global_step == 0 and float(step2.opt.m.abs().max()) == 0.0
    mv = [v for n, v in g2.store.vars.items() if n.endswith("moving_variance")]
    assert mv and all(torch.equal(v.data, torch.ones_like(v.data)) for v in mv)     # dry run left no trace
    assert checkpoint.restore_training_state(str(tmp_path), g2, step2.opt) == 3
    assert step2.opt.global_step == 3
    for _ in range(2):
        step2(*batch2)
    assert torch.equal(g.store.flat, g2.store.flat) and torch.equal(g.store.flat_aux, g2.store.flat_aux)
    assert torch.equal(step.opt.m, step2.opt.m) and torch.equal(step.opt.v, step2.opt.v)
    assert torch.equal(step.opt.ema, step2.opt.ema)


def test_build_then_step_equals_plain_steps(device):
    g1, b1, s1 = _make(device, True)
    g2, b2, s2 = _make(device, True)
    s2.build(*b2)
    for _ in range(5):
        s1(*b1)
        s2(*b2)
    assert torch.equal(g1.store.flat, g2.store.flat) and torch.equal(g1.store.flat_aux, g2.store.flat_aux)


_RCCL1_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as td
from tensorflow_ocr_amd import dist, synthetic
from tensorflow_ocr_amd.graph import Graph
from tensorflow_ocr_amd.nets import model_vgg_16 as M
from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
rank, world, local = dist.init_process_group_from_env("nccl", force=True)      # ONE-rank RCCL communicator
assert (rank, world) == (0, 1) and td.get_backend() == "nccl"
dev = torch.device("cuda:0")
ones = torch.ones(4, device=dev); td.all_reduce(ones); assert ones.tolist() == [1.0] * 4
def make(force):
    g = Graph(dev, loss_scale=1024.0, seed=3)
    rng = np.random.default_rng(50)
    batch = [torch.from_numpy(a).to(dev) for a in synthetic.make_batch(rng, 2, 64)]
    def fl(gr, im, px, lk, mk):
        a, b = M.model_vgg(im, graph=gr)
        return M.loss(px, a, lk, b, mk, graph=gr)
    return g, batch, TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3), world_size=world,
                               bucket_bytes=8 << 20, force_reduce=force)
g0, b0, s0 = make(False)
g1, b1, s1 = make(True)
fired = []
for i in range(7):                                   # 2 eager + 1 recorded + 4 replayed
    s0(*b0)
    s1(*b1)
    fired.append(len(s1.reducer.handles))
torch.cuda.synchronize()
red = s1.reducer
assert s1.plan is not None and red.active and len(red.buckets) >= 2 and red.comm_stream is not None
assert not s0.reducer.active
# every bucket went through RCCL on the comm stream and was waited for before the optimiser
# (an all-reduce over one rank is the identity: the two towers must agree bit for bit)
assert torch.equal(g0.store.flat, g1.store.flat), (g0.store.flat - g1.store.flat).abs().max().item()
assert torch.equal(s0.opt.m, s1.opt.m) and torch.isfinite(g1.store.flat).all()
n_py = sum(1 for e in s1.plan if e[0] == "py")
n_x = sum(1 for e in s1.plan if e[0] == "c" and e[4] is not None and e[4][0] == "xchg")
names = [e[3] for e in s1.plan if e[0] == "c" and e[4] is not None and e[4][0] == "xchg"]
if os.environ.get("OCR_EXCHANGE") == "torch":
    assert red.mode == "torch" and n_x == 0
    assert n_py >= len(red.buckets) + 2, n_py        # bucket hooks + finish + optimiser are host callbacks of the plan
else:
    # the exchange is C-ABI calls of the plan: per bucket event-record, stream-wait, ocr_allreduce_bucket,
    # event-record, and one stream-wait per bucket before the optimiser; only optimiser + re-pack stay host callbacks
    assert red.mode == "abi" and red.comm.size() == 1
    nb = len(red.buckets)
    assert n_x == 5 * nb and names.count("ocr_allreduce_bucket") == nb and n_py == 2, (n_x, n_py, names)
    # ADVICE r5 (high), on the REAL recorded step: no exchange entry of the scheduled plan runs before a weight-gradient
    # launch (slab kernel, slab sum, conv1_1's sums form) that was recorded in front of it — at this size every guest is below
    # the pairing threshold, i.e. the advisor's case: all weight gradients held back, bucket 0 completed by an in-place launch.
    # Checked for every placement of the scheduler (exchange at the fork or behind the join, balanced or greedy hosts)
    from tensorflow_ocr_amd.train import schedule_guests
    rec = s1.recorded
    is_x = lambda e: e[0] == "c" and e[4] is not None and e[4][0] == "xchg"
    is_w = lambda e: e[0] == "c" and ((e[4] is not None and e[4][0] in ("side", "reduce")) or "wgrad" in e[3])
    assert sum(map(is_w, rec)) >= 20 and sum(map(is_x, rec)) == 5 * nb
    for kw in (dict(), dict(xchg_at_fork=False), dict(balance=False), dict(min_us=0.0), dict(min_us=0.0, xchg_at_fork=False)):
        pos = {id(e): i for i, e in enumerate(schedule_guests(rec, **kw))}
        seen_w = []
        for e in rec:
            if is_w(e):
                seen_w.append(e)
            elif is_x(e):
                assert all(pos[id(w)] < pos[id(e)] for w in seen_w), (kw, e[3], e[4])
    # bench.py's A/B switch: with the exchange disabled the replay skips those entries and still trains
    red.enabled = False
    s1(*b1); s0(*b0)
    red.enabled = True
    torch.cuda.synchronize()
    assert torch.equal(g0.store.flat, g1.store.flat)
td.barrier(); td.destroy_process_group()
print("rccl-1 ok buckets", red.bucket_nbytes(), red.mode)
"""


@pytest.mark.parametrize("exchange", ["abi", "torch"])
def test_rccl_one_rank_group_through_trainstep(device, tmp_path, exchange):
    """The `nccl` (= RCCL) path of dist.GradientAllReduce — comm stream, event from the compute
    stream, async all_reduce handles, `h.wait()` before the replayed optimiser launch — executed on
    hardware with the one GPU this box has: a ONE-rank communicator (multigpu_train.py:70-85,118-133)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl1.py"
    script.write_text(_RCCL1_WORKER % root)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OCR_EXCHANGE"] = exchange
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=540)
    assert r.returncode == 0 and b"rccl-1 ok" in r.stdout and exchange.encode() in r.stdout, r.stdout.decode()[-3000:]


def _bench(args, timeout=540):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    if "--with-config-legs" in args:
        args = [a for a in args if a != "--with-config-legs"]
    else:
        args = args + ["--no-config-legs"]
    # these tests check the exchange, replica and roofline records: a --full run's
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full"] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    # the contract: stdout is the ONE JSON line, nothing else (RCCL / gloo banners go to stderr: bench.py re-points fd 1)
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks(device):
    """`python bench.py --gpus 2` from a clean shell (no WORLD_SIZE): the parent spawns the ranks
    before touching the GPU and relays rank 0's single JSON line.  Two ranks share this box's one
    GPU through gloo (RCCL refuses two ranks on one device); the driver's SCALE run uses nccl."""
    out = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64",
                  "--backend", "gloo", "--share-gpu", "--no-cpu-baseline"])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 4 and out["config"]["parallelism"] == "dp2"
    ex = out["exchange"]
    assert ex["backend"] == "gloo" and ex["rccl_ranks"] == 2 and sum(ex["bucket_bytes"]) == ex["grad_bytes"]
    assert out["value"] > 0 and "comm_exposed_ms" in ex and out["scaling"] == "weak" and ex["in_timed_region"] is True


def test_bench_self_launches_four_ranks_with_replica_checks(device):
    """VERDICT r2 item 4, within this pool's process guard (at most 6 processes on the card: 4 ranks + this test; the
    8-rank launcher itself is exercised on the CPU in test_host_cpu.py): `python bench.py --gpus 4` spawns its ranks,
    every rank trains on a different shard and all hold identical parameters after the steps."""
    out = _bench(["--gpus", "4", "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "64",
                  "--backend", "gloo", "--share-gpu", "--no-cpu-baseline"])
    assert out["n_gpus"] == 4 and out["config"]["global_batch"] == 8 and out["config"]["parallelism"] == "dp4"
    assert out["exchange"]["rccl_ranks"] == 4 and out["exchange"]["mode"] == "torch"
    assert out["replicas"] == {"parameters_identical": True, "data_shards_distinct": True, "ranks": 4}


def test_bench_one_rank_rccl_exchange(device):
    out = _bench(["--gpus", "1", "--force-pg", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64",
                  "--no-cpu-baseline"])
    ex = out["exchange"]
    # the one-rank `nccl` group exists (--force-pg) and the buckets travel through the C ABI on a communicator of
    # the library's own (dist.AbiComm: ocr_comm_init_rank / ocr_allreduce_bucket)
    assert ex["backend"].startswith("rccl") and ex["mode"] == "abi" and ex["rccl_ranks"] == 1 and len(ex["bucket_bytes"]) >= 2
    assert out["n_gpus"] == 1 and np.isfinite(out["loss"])


def test_bench_default_single_gpu_line_reports_the_exchange(device):
    """the N = 1 line carries `exchange` (one-rank RCCL communicator through
    ocr_allreduce_bucket, no torch.distributed group at all) so the driver's record shows RCCL loaded; and
    OCR_EXCHANGE=torch keeps the torch.distributed path selectable."""
    out = _bench(["--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--no-cpu-baseline"])
    ex = out["exchange"]
    assert ex["mode"] == "abi" and ex["rccl_ranks"] == 1 and sum(ex["bucket_bytes"]) == ex["grad_bytes"]
    assert "comm_exposed_ms" in ex and "ms_per_step_with_exchange" in ex and ex["in_timed_region"] is False
    # round 6: the stand-in at both footprints (ocr_comm_proxy_set_footprint) and with the buckets issued at the next fork
    # (train.schedule_guests(xchg_at_fork=True)); the plan's projection is a bracket over the two footprints
    assert {"backward_stretch_ms", "exposed_ms_overlapped", "exposed_ms_after_backward"} <= set(ex["proxy_fat"])
    assert {"exposed_ms_overlapped", "exposed_ms_overlapped_fat"} <= set(ex["proxy_at_fork"])
    br = ex["plan"]["projected_scaling_of_8_bracket"]
    assert all(0 < lo <= 8.0 and 0 < hi <= 8.0 for lo, hi in (br["under_backward"], br["after_backward"]))
    rf = out["roofline"]
    assert set(rf["counters_from"]["files"]) == {"traffic", "mfma_busy", "clock_ghz"}
    for f, v in rf["counters_from"]["files"].items():      # a counter is reported only with current provenance
        key = {"traffic": "traffic", "mfma_busy": "mfma_busy", "clock_ghz": "clock_ghz"}[f]
        assert v["current"] or rf[key] is None
    out2 = _bench(["--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--no-cpu-baseline", "--no-pg"])
    assert "exchange" not in out2
    assert abs(out2["loss"] - out["loss"]) < 1e-6            # a one-rank exchange changes nothing


def test_bench_plain_run_dumps_the_last_timed_step(device, tmp_path):
    """`bench.py --dump-outputs DIR` without --full: the result line carries the headline fields only, and DIR holds what
    the LAST timed step computed — the same loss, score maps and updated parameters as an eager TrainStep taking the same
    number of steps (3 engine-build + warm-up + timed) on bench.py's batch and initial weights."""
    import json
    import os
    import subprocess
    import sys
    from tensorflow_ocr_amd import _lib, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    n, size, warmup, steps = 2, 64, 1, 2
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", str(n), "--size", str(size),
                        "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["dtype"] == _lib.STORAGE and out["higher_is_better"] is True
    assert not {"roofline", "exchange", "configs", "cpu_baseline"} & set(out)
    names = {"loss", "pixel_cls", "link_cls", "params_sample", "moving_stats"}
    assert set(out["dumped"]) == names and {p.name for p in d.iterdir()} == {x + ".npy" for x in names}
    got = {x: np.load(d / (x + ".npy")) for x in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(os.path.getsize(d / (x + ".npy")) for x in names) <= 64 << 20
    assert abs(float(got["loss"][0]) - out["loss"]) < 1e-5

    g = Graph(device, loss_scale=1024.0, seed=1)
    batch = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), n, size)]
    maps = {}

    def fl(gr, im, px, lk, mk):
        maps["pixel_cls"], maps["link_cls"] = M.model_vgg(im, is_training=True, graph=gr)
        return M.loss(px, maps["pixel_cls"], lk, maps["link_cls"], mk, graph=gr)
    step = TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-4), replay=False)
    for _ in range(3 + warmup + steps):
        loss = step(*batch)
    torch.cuda.synchronize()
    assert abs(float(got["loss"][0]) - loss.item()) < 1e-5
    for k in ("pixel_cls", "link_cls"):
        ref = maps[k].data.float().cpu().numpy()
        assert got[k].shape == ref.shape and np.abs(got[k] - ref).max() < 1e-3, k
    ref = bench._sample(g.store.flat.cpu().numpy(), bench.DUMP_PARAM_SAMPLE, 1)
    assert got["params_sample"].shape == ref.shape and np.allclose(got["params_sample"], ref, rtol=1e-5, atol=1e-7)
    assert np.allclose(got["moving_stats"], g.store.flat_aux.cpu().numpy(), rtol=1e-4, atol=1e-6)
