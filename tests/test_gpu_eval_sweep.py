"""GPU: ocr_eval_curve_batch / ocr_eval_ic15_curve_batch / ocr_eval_ap (csrc/eval_curve.hip, tool/metrics.DeviceCurve,
evaluate.py's `sweep`) against tests/sweep_ref.py, which FILTERS the detection list by every threshold and RE-RUNS the
matcher's reference.  The curve entries are fed from the real ocr_eval_match_batch / ocr_eval_ic15_match_batch outputs.
Counts and flags are integers and must be equal; AP must lie within (K + 2) 2^-53 of the exact Fraction value, relative, K
the number of matched slots (one rounding per term, a K-term sum of non-negative terms, one division).
Shapes n = 3, max_d = 70 (crosses a wave), max_g = 5, T = 6: sweep_ref.gpu_images, whose edge cases
tests/test_sweep_host.py checks on the CPU."""
import ctypes
import importlib
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import eval_support as E
import sweep_ref as S
from eval_support import EVAL

pytestmark = pytest.mark.gpu
N, MAX_D, MAX_G, T = S.N, S.MAX_D, S.MAX_G, S.T
RULES = ("raster", "icdar15")
SENT = 0x5A
f32 = np.float32


@pytest.fixture(scope="module")
def graph(device):
    from tensorflow_ocr_amd.graph import Graph
    return Graph(device)


@pytest.fixture(scope="module")
def rbox_eval_dir(graph, tmp_path_factory):
    return E.rbox_eval_dir(graph, str(tmp_path_factory.mktemp("eval")))


@pytest.fixture(scope="module")
def link_eval_dir(device, graph, tmp_path_factory):
    return E.link_eval_dir(str(tmp_path_factory.mktemp("link_eval")), E.host_best_box(graph, device))


@pytest.fixture(scope="module")
def expected():
    """per rule: the states of one full matching, the re-run rows, per image — computed once"""
    images = S.gpu_images()
    out = {}
    for rule in RULES:
        per = {}
        for name, (dets, scores, gts, flags) in images.items():
            state, care_gt = S.match_states(rule, dets, gts, flags)
            per[name] = dict(state=state, care_gt=care_gt, rows=S.rerun_rows(rule, images[name], S.THRESHOLDS))
        out[rule] = per
    return images, out


def _pack(images, order, device):
    """the images in `order` -> device tensors; score rows beyond nd hold a value that would be kept and break the order"""
    dets = np.zeros((N, MAX_D, 4, 2), np.int32)
    gts = np.zeros((N, MAX_G, 4, 2), np.int32)
    score = np.full((N, MAX_D), 999.0, f32)
    nd, ng = np.zeros(N, np.int32), np.zeros(N, np.int32)
    flags = np.zeros((N, MAX_G), np.uint8)
    for i, name in enumerate(order):
        d, s, g, c = images[name]
        fill = d[0] if len(d) else g[0]
        dets[i], gts[i] = fill, fill                                        # rows beyond a count would match everything
        dets[i, :len(d)], score[i, :len(d)], gts[i, :len(g)], flags[i, :len(g)] = d, s, g, c
        nd[i], ng[i] = len(d), len(g)
    up = lambda a: torch.from_numpy(a).to(device)
    return dict(dets=up(dets), nd=up(nd), gts=up(gts), ng=up(ng), flags=up(flags), score=up(score))


def _match(rule, p, graph):
    """the real matcher -> (its outputs, the record int64 [4])"""
    from tensorflow_ocr_amd.tool import bboxes
    if rule == "raster":
        tp, fp, rec = bboxes.bboxes_matching_batch(p["dets"], p["nd"], p["gts"], p["ng"], p["flags"], 0.5, graph=graph, mask_hw=(400, 400))
        return (tp, fp), rec
    dm, gm, rec = bboxes.ic15_matching_batch(p["dets"], p["nd"], p["gts"], p["ng"], p["flags"], graph=graph)
    return (dm, gm), rec


def _device_states(rule, outs):
    a, b = (t.cpu().numpy() for t in outs)
    return np.where(a != 0, 2, np.where(b != 0, 1, 0)) if rule == "raster" else np.where(a >= 0, 2, np.where(a == -1, 1, 0))


class Bufs:
    """curve / flag / pool / AP with sentinel bytes behind every one of them"""

    def __init__(self, device, thresholds=S.THRESHOLDS, n=N, max_d=MAX_D):
        from tensorflow_ocr_amd import ops
        t = len(thresholds)
        mk = lambda nbytes: torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=device)
        self.raw = dict(curve=mk(t * 32), uns=mk(4), ps=mk(n * max_d * 4), pc=mk(n * max_d * 8), pn=mk(n * 4), ap=mk(8))
        self.size = dict(curve=t * 32, uns=4, ps=n * max_d * 4, pc=n * max_d * 8, pn=n * 4, ap=8)
        v = lambda k, dt, *shape: self.raw[k][:self.size[k]].view(dt).view(*shape)
        self.curve, self.uns, self.ap = v("curve", torch.int64, t, 4), v("uns", torch.int32, 1), v("ap", torch.float64, 1)
        self.pool = (v("ps", torch.float32, n, max_d), v("pc", torch.int32, n, max_d, 2), v("pn", torch.int32, n))
        self.thr = torch.tensor(thresholds, dtype=torch.float32, device=device)
        ops.eval_curve_init(self.curve, self.uns, self.ap)

    def untouched(self, *keys):
        return all(bool((self.raw[k][:self.size[k]] == SENT).all()) for k in keys)

    def tails_intact(self):
        return all(bool((self.raw[k][self.size[k]:] == SENT).all()) for k in self.raw)


def _curve(rule, outs, p, b, pool=True):
    from tensorflow_ocr_amd import ops
    if rule == "raster":
        ops.eval_curve_batch(outs[0], outs[1], p["score"], p["nd"], p["ng"], p["flags"], b.thr, b.curve, b.uns, pool=b.pool if pool else None)
    else:
        ops.eval_ic15_curve_batch(outs[0], outs[1], p["score"], p["nd"], p["ng"], b.thr, b.curve, b.uns, pool=b.pool if pool else None)


# ------------------------------------------------------------------------------------------------ curve, pool, AP
@pytest.mark.parametrize("order", S.ORDERS, ids=["-".join(o) for o in S.ORDERS])
@pytest.mark.parametrize("rule", RULES)
def test_curve_pool_and_ap_equal_the_rerun_reference(device, graph, expected, rule, order):
    from tensorflow_ocr_amd import ops
    images, exp = expected
    exp = exp[rule]
    p = _pack(images, order, device)
    outs, rec = _match(rule, p, graph)
    states = _device_states(rule, outs)
    for i, name in enumerate(order):                                        # the matcher itself decides as its reference
        assert states[i, :len(exp[name]["state"])].tolist() == exp[name]["state"].tolist(), (rule, name)
    b = Bufs(device)
    assert b.curve.tolist() == [[0] * 4] * T and b.uns.item() == 0 and b.ap.item() == 0.0      # ocr_eval_curve_init
    _curve(rule, outs, p, b)
    torch.cuda.synchronize()
    want = S.sum_rows([exp[name]["rows"] for name in order])
    got = b.curve.cpu().numpy()
    print("sweep %s %s: curve %s" % (rule, order[0], got.tolist()))
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert exp["crowd"]["state"][-1] == S.CARE                              # the NaN-scored detection is a false positive of the record
    r = rec.tolist()
    assert got[0].tolist() == [r[0], r[1], r[2] - 1, r[3] - 1]              # below every score: the operating point, less the NaN-scored one
    assert got[1, 1:].tolist() == [0, 0, 0] and got[3, 1:].tolist() == [0, 0, 0] and got[1, 0] == rec[0].item()    # NaN / above all: nothing kept
    assert b.uns.item() == 0                                                # collect's order
    # the pool rows
    ps, pc, pn = (t.cpu().numpy() for t in b.pool)
    assert pn.tolist() == [len(images[name][0]) for name in order]
    for i, name in enumerate(order):
        k = len(images[name][0])
        assert np.array_equal(pc[i], S.pool_cum(exp[name]["state"], images[name][1], MAX_D)), (rule, name)
        assert np.array_equal(ps[i, :k].view(np.int32), images[name][1].view(np.int32)) and np.isnan(ps[i, k:]).all()
    # a second call on the same buffers ADDS to the curve (and rewrites the same pool rows)
    _curve(rule, outs, p, b, pool=False)
    torch.cuda.synchronize()
    assert np.array_equal(b.curve.cpu().numpy(), 2 * want) and b.uns.item() == 0
    # AP over the pool, G read from the matcher's record on the device
    ops.eval_ap(*b.pool, rec, b.ap, graph.workspace())
    torch.cuda.synchronize()
    exact, k_matched = S.average_precision([(exp[name]["state"], images[name][1]) for name in order], int(rec[0].item()))
    got_ap = b.ap.item()
    err = abs(Fr(got_ap) - exact)
    room = (k_matched + 2) * Fr(1, 2 ** 53) * exact
    print("sweep %s %s: AP %.17g, exact %.17g, |AP - exact| = %.3g = %.3g of the bound (K = %d)"
          % (rule, order[0], got_ap, float(exact), float(err), float(err / room), k_matched))
    assert exact > 0 and k_matched >= 2 and err <= room
    assert b.tails_intact()
    # G = 0: AP is 0
    zero = torch.zeros((4,), dtype=torch.int64, device=device)
    b.ap.fill_(7.0)
    ops.eval_ap(*b.pool, zero, b.ap, graph.workspace())
    assert b.ap.item() == 0.0


def test_ap_tie_rule_decides_between_the_two_image_orders(expected):
    """the two orders of the fixture give different exact APs under both rules: the tie between 'crowd' and 'no_gt' counts"""
    images, exp = expected
    for rule in RULES:
        g = sum(exp[rule][name]["care_gt"] for name in images)
        a, b = (S.average_precision([(exp[rule][name]["state"], images[name][1]) for name in order], g)[0] for order in S.ORDERS)
        assert a < b, (rule, float(a), float(b))                            # 'no_gt' first: its unmatched 2.75s come before the matched one


@pytest.mark.parametrize("rule", RULES)
def test_unsorted_flag_is_raised_by_a_swap_and_by_a_nan_inside(device, graph, expected, rule):
    images, _ = expected
    p = _pack(images, S.ORDERS[0], device)
    outs, _ = _match(rule, p, graph)
    for what in ("swap", "nan", "second_wave"):
        q = dict(p, score=p["score"].clone())
        if what == "swap":
            q["score"][1, 2], q["score"][1, 3] = p["score"][1, 3].item(), p["score"][1, 2].item()       # 2.75 <-> 2.625
        elif what == "nan":
            q["score"][0, 4] = float("nan")                                 # a NaN before finite scores
        else:
            q["score"][1, 64] = 5.0                                         # a rise at the first detection of the second wave
        b = Bufs(device)
        _curve(rule, outs, q, b, pool=False)
        assert b.uns.item() != 0, what
        _curve(rule, outs, p, b, pool=False)                                # OR-ed into: a clean batch does not clear it
        assert b.uns.item() != 0
    # equal neighbours and a NaN tail are in order
    q = dict(p, score=p["score"].clone())
    q["score"][0, 10:12] = float("nan")
    b = Bufs(device)
    _curve(rule, outs, q, b, pool=False)
    assert b.uns.item() == 0 and b.untouched("ps", "pc", "pn")             # and without a pool nothing of it is written


def test_every_status_code_leaves_the_outputs_alone(device, graph, expected):
    from tensorflow_ocr_amd import _lib as L
    images, _ = expected
    p = _pack(images, S.ORDERS[0], device)
    (tp, fp), rec_r = _match("raster", p, graph)
    (dm, gm), rec_i = _match("icdar15", p, graph)
    b = Bufs(device)
    b.raw["curve"][:b.size["curve"]] = SENT                                 # (undo the init: everything is sentinel)
    b.raw["uns"][:4] = SENT
    b.raw["ap"][:8] = SENT
    ptr, SZ = L.ptr, ctypes.c_size_t
    ra = lambda tp=tp, fp=fp, sc=p["score"], nd=p["nd"], ng=p["ng"], ign=p["flags"], thr=b.thr, n=N, d=MAX_D, g=MAX_G, t=T, cur=b.curve, uns=b.uns, ps=b.pool[0], pc=b.pool[1], pn=b.pool[2]: (
        ptr(tp), ptr(fp), ptr(sc), ptr(nd), ptr(ng), ptr(ign), ptr(thr), n, d, g, t, ptr(cur), ptr(uns), ptr(ps), ptr(pc), ptr(pn), L.stream_ptr())
    ia = lambda dm=dm, gm=gm, sc=p["score"], nd=p["nd"], ng=p["ng"], thr=b.thr, n=N, d=MAX_D, g=MAX_G, t=T, cur=b.curve, uns=b.uns, ps=b.pool[0], pc=b.pool[1], pn=b.pool[2]: (
        ptr(dm), ptr(gm), ptr(sc), ptr(nd), ptr(ng), ptr(thr), n, d, g, t, ptr(cur), ptr(uns), ptr(ps), ptr(pc), ptr(pn), L.stream_ptr())
    for name, a, required in (("ocr_eval_curve_batch", ra, ("tp", "fp", "sc", "nd", "ng", "ign", "thr", "cur", "uns")),
                              ("ocr_eval_ic15_curve_batch", ia, ("dm", "gm", "sc", "nd", "ng", "thr", "cur", "uns"))):
        fn = L._fn(name, ctypes.c_int)
        for k in required:
            assert fn(*a(**{k: None})) == -1, (name, k)
        for kw in (dict(n=0), dict(d=0), dict(g=-1), dict(ps=None), dict(pc=None, pn=None)):
            assert fn(*a(**kw)) == -1, (name, kw)
        for kw in (dict(d=1025), dict(g=255), dict(n=65536), dict(t=0), dict(t=65)):
            assert fn(*a(**kw)) == -2, (name, kw)
    nbytes = L.call_size("ocr_eval_ap_workspace", ctypes.c_int(N), ctypes.c_int(MAX_D))
    assert nbytes == 8                                                      # 210 slots: one partial
    ws = torch.full((nbytes,), SENT, dtype=torch.uint8, device=device)
    ap = L._fn("ocr_eval_ap", ctypes.c_int)
    aa = lambda ps=b.pool[0], pc=b.pool[1], pn=b.pool[2], n=N, d=MAX_D, rec=rec_i, out=b.ap, wsp=ws, wsb=nbytes: (
        ptr(ps), ptr(pc), ptr(pn), n, d, ptr(rec), ptr(out), ptr(wsp), SZ(wsb), L.stream_ptr())
    for k in ("ps", "pc", "pn", "rec", "out", "wsp"):
        assert ap(*aa(**{k: None})) == -1, k
    assert ap(*aa(n=0)) == -1 and ap(*aa(d=0)) == -1
    assert ap(*aa(d=1025)) == -2 and ap(*aa(n=65536, wsb=1 << 40)) == -2
    assert ap(*aa(wsb=nbytes - 1)) == -4 and ap(*aa(wsb=0)) == -4
    init = L._fn("ocr_eval_curve_init", ctypes.c_int)
    assert init(ptr(None), T, ptr(b.uns), ptr(None), L.stream_ptr()) == -1 and init(ptr(b.curve), 65, ptr(b.uns), ptr(None), L.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert b.untouched("curve", "uns", "ps", "pc", "pn", "ap") and b.tails_intact() and bool((ws == SENT).all())
    # and the same arguments, complete, run
    init(ptr(b.curve), T, ptr(b.uns), ptr(b.ap), L.stream_ptr())
    assert L._fn("ocr_eval_ic15_curve_batch", ctypes.c_int)(*ia()) == 0 and ap(*aa()) == 0
    torch.cuda.synchronize()
    assert b.curve[0].tolist()[:2] == rec_i.tolist()[:2] and b.ap.item() > 0 and b.tails_intact()


# ------------------------------------------------------------------------------------------------ the evaluators
CHAIN_SWEEP = [-1.0, 0.9, 0.97, 1e9, 2.5]      # below every score of both geometries, inside the link scores, above all, inside the RBOX sums


def _sweep_case(ev, calls, monkeypatch):
    """one pass with every chain's `last` kept (device tensors, no read) -> (result, reads, the reference's rows, exact AP, K)"""
    chains = E.keep_lasts(ev)
    reads = E.spy_reads(monkeypatch, calls)
    res = ev.run()
    monkeypatch.undo()
    rule = "icdar15" if ev.protocol == "icdar15" else "raster"
    rows, pool, care = [], [], 0
    for last in chains:
        host = {k: v.cpu().numpy() for k, v in last.items()}
        flags = host["gdontcare" if rule == "icdar15" else "gignored"].astype(bool)
        for i in range(len(host["nd"])):
            k, n_g = int(host["nd"][i]), int(host["ng"][i])
            image = (host["dets"][i, :k], host["det_score"][i, :k], host["gts"][i, :n_g], flags[i, :n_g])
            state, care_gt = S.match_states(rule, image[0], image[2], image[3])
            rows.append(S.rerun_rows(rule, image, CHAIN_SWEEP))
            pool.append((state, image[1]))
            care += care_gt
    exact, k_matched = S.average_precision(pool, care)
    return res, reads, S.sum_rows(rows), exact, k_matched


def _check_sweep_result(evaluate, res, plain, reads, want, exact, k_matched, n_chains, tag):
    print("%s: %s\n%s" % (tag, evaluate.format_line(res), evaluate.format_sweep(res)))
    assert reads == [("cpu", n_chains)], reads                              # exactly one device-to-host read, after the last chain
    for k, v in plain.items():                                              # the operating point: bitwise what a run without a sweep gives
        assert res[k] == v and type(res[k]) is type(v), k
        if isinstance(v, float):
            assert np.float64(res[k]).tobytes() == np.float64(v).tobytes(), k
    assert sorted(set(res) - set(plain)) == ["ap", "best", "sweep"]
    assert evaluate.format_line(res) == evaluate.format_line(plain)
    got = [[res["num_gt"], r["tp"], r["fp"], r["num_det"]] for r in res["sweep"]]
    assert got == want.tolist() and [r["threshold"] for r in res["sweep"]] == CHAIN_SWEEP
    low = res["sweep"][0]                                                   # the threshold below every score: the operating point
    assert [low[k] for k in ("precision", "recall", "hmean", "tp", "fp", "num_det")] == [plain[k] for k in ("precision", "recall", "hmean", "tp", "fp", "num_det")]
    assert res["sweep"][3]["num_det"] == 0 and res["sweep"][3]["hmean"] == 0.0
    assert res["best"] is max(res["sweep"], key=lambda r: r["hmean"]) and res["best"]["hmean"] >= low["hmean"]
    err = abs(Fr(res["ap"]) - exact)
    print("%s: AP %.17g, exact %.17g, |AP - exact| = %.3g (K = %d)" % (tag, res["ap"], float(exact), float(err), k_matched))
    assert exact > 0 and err <= (k_matched + 2) * Fr(1, 2 ** 53) * exact


@pytest.mark.parametrize("protocol", RULES)
def test_evaluator_with_a_sweep_reads_once_and_keeps_the_operating_point(device, graph, rbox_eval_dir, monkeypatch, protocol):
    from tensorflow_ocr_amd import evaluate
    d, maps, _ = rbox_eval_dir
    forward, calls = E.rbox_stub_forward(device, maps)
    plain = evaluate.Evaluator(graph, forward, d, batch_size=2, protocol=protocol).run()
    del calls[:]
    ev = evaluate.Evaluator(graph, forward, d, batch_size=2, protocol=protocol, sweep=CHAIN_SWEEP)
    res, reads, want, exact, k_matched = _sweep_case(ev, calls, monkeypatch)
    assert ev.acc.reads == 1
    _check_sweep_result(evaluate, res, plain, reads, want, exact, k_matched, 2, "evaluator sweep [%s]" % protocol)
    assert ev.run() == res and ev.acc.reads == 2                            # a second pass starts from zero


@pytest.mark.parametrize("protocol", RULES)
def test_link_evaluator_with_a_sweep_reads_once_and_keeps_the_operating_point(device, graph, link_eval_dir, monkeypatch, protocol):
    from tensorflow_ocr_amd import evaluate
    d, maps = link_eval_dir
    forward, calls = E.link_stub_forward(device, maps)
    kw = dict(batch_size=2, eval_image_height=EVAL, eval_image_width=EVAL, protocol=protocol)
    plain = evaluate.LinkEvaluator(graph, forward, d, **kw).run()
    del calls[:]
    ev = evaluate.LinkEvaluator(graph, forward, d, sweep=CHAIN_SWEEP, **kw)
    res, reads, want, exact, k_matched = _sweep_case(ev, calls, monkeypatch)
    assert ev.acc.reads == 1
    _check_sweep_result(evaluate, res, plain, reads, want, exact, k_matched, 2, "link evaluator sweep [%s]" % protocol)
    assert 0 < sum(r["num_det"] for r in res["sweep"][1:3]) < 2 * res["num_det"]          # the link scores lie around the inner thresholds


def test_an_unsorted_score_list_is_an_error_of_the_pass(device, graph, rbox_eval_dir, monkeypatch):
    from tensorflow_ocr_amd import evaluate, ops
    d, maps, _ = rbox_eval_dir
    forward, _ = E.rbox_stub_forward(device, maps)
    ev = evaluate.Evaluator(graph, forward, d, batch_size=2, sweep=[0.5])
    collect = ops.eval_collect

    def reversed_scores(*a):
        collect(*a)
        a[5][:, 1] = a[5][:, 0]                                             # dets: two copies of the best detection ...
        a[6][:, 0], a[6][:, 1] = 1.0, 2.0                                   # ... whose scores rise
        a[7].fill_(2)                                                       # nd
    monkeypatch.setattr(ops, "eval_collect", reversed_scores)
    with pytest.raises(ValueError, match="descending order"):
        ev.run()


def test_training_with_a_sweep_records_the_same_step_and_trains_the_same_weights(device, tmp_path, monkeypatch):
    d = str(tmp_path)
    E.write_training_eval_dir(d)
    calls0, kinds0, state0, _, _ = E.train_east_rbox(device, d, False)
    import sys
    sys.path.insert(0, E.ROOT)
    T_ = importlib.import_module("multigpu_train")
    parse = T_.parse
    monkeypatch.setattr(T_, "parse", lambda argv: parse(argv + ["--eval_sweep", "0:40:5"]))
    calls1, kinds1, state1, results, te = E.train_east_rbox(device, d, True)
    assert te.evaluator.sweep == [0.0, 10.0, 20.0, 30.0, 40.0] and te.evaluator.curve is not None
    assert calls1 == calls0 and kinds1 == kinds0 and len(calls0) > 50       # the recorded call list is identical
    for a, b in zip(state0, state1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # weights, moving statistics, EMA, Adam slots: bit for bit
    assert len(results) == 5 and te.evaluator.acc.reads == 5
    for r in results:
        assert len(r["sweep"]) == 5 and r["best"] in r["sweep"] and 0.0 <= r["ap"] <= 1.0
        assert [r["sweep"][0][k] for k in ("tp", "fp", "num_det")] == [r["tp"], r["fp"], r["num_det"]]

    class Writer:
        def __init__(self):
            self.scalars, self.steps = {}, []

        def add_scalar(self, tag, value):
            self.scalars[tag] = value

        def flush_step(self, step):
            self.steps.append(step)
    w = Writer()
    te.write(w, 5)
    assert sorted(w.scalars) == ["eval/ap", "eval/best_hmean", "eval/best_threshold", "eval/hmean", "eval/precision", "eval/recall"]
    assert w.scalars["eval/ap"] == te.last["ap"] and w.scalars["eval/best_threshold"] == te.last["best"]["threshold"] and w.steps == [5]
