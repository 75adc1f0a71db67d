"""tensorflow_ocr_amd/step_plan.py without a GPU: the scheduler against plans recorded from the commit it was split out of
(tests/golden/guest_plans.json, written by tests/golden/make_guest_plans.py), what a plan must keep of its recording,
the warning of the silent fallback, and the tag vocabulary.

The corpus is RECORDINGS synthetic recordings of the shape `schedule_guests`' docstring describes, each scheduled under
the 12 SETTINGS; the golden keeps one SHA-256 per plan.  Whether a plan forked, took several hosts, met more than 12
pending hosts, was short of hosts or moved an exchange entry to a later fork is read off the recording and the plan
(`traits`): the golden's plans and the rewritten scheduler's are the same lists, so the same figures hold for both."""
import ctypes
import hashlib
import itertools
import json
import os
import random
import warnings

import pytest

try:
    from tensorflow_ocr_amd import step_plan as P
except ImportError:              # tests/golden/make_guest_plans.py, run on the commit from before the module: it needs
    P = None                     # the corpus and `traits` only

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "guest_plans.json")
RECORDINGS = 320
# (balance, xchg_at_fork, cover, min_us)
SETTINGS = [(b, x, c, m) for b in (0, 1) for x in (0, 1) for c, m in ((2.1, 40), (1.0, 0), (3.0, 100))]
GUEST_BYTES_PER_US, HOST_FLOP_PER_US = 5.0e6, 1.3e9           # (written out: the corpus must not move with the module's)


# ---------------------------------------------------------------------------------------------------- the corpus
def _c(name, tag=None, grid=0):
    return ["c", None, (ctypes.c_int(grid), ctypes.c_void_p(0)), name, tag]


def _nothing():
    pass


def recording(seed):
    """One synthetic recorded step, backward part: layers of [pre] guest dgrad wgrad reduce [[accum] xchg{1,3}], then the
    closing exchange entries, the accumulate phase's advance and the two host callbacks.  Only `random()` is drawn from."""
    r = random.Random(seed).random
    pick = lambda xs: xs[int(r() * len(xs))]
    log_between = lambda lo, hi: lo * (hi / lo) ** r()
    layers = 1 + int(r() * 16)
    if r() < 0.35:
        layers = 13 + int(r() * 4)                                 # deep ones often enough for more than 12 pending hosts
    no_guest, no_host = r() < 0.05, r() < 0.05
    small_guests = r() < 0.45                                      # a step of short passes: hosts pile up
    p_late = pick((0.0, 0.0, 0.15, 0.35))                          # a "late" exchange entry needs every gradient: it flushes
    p_bucket = pick((0.1, 0.3, 0.3, 0.5))
    # more than 12 hosts pending needs a deep step whose early passes are far too short for its weight gradients (no host
    # is spent on a guest it would outlast 3 times over) and whose last passes are long: one recording in five is such
    pile_up = r() < 0.2 and not (no_guest or no_host)
    if pile_up:
        layers, p_late = 15 + int(r() * 2), 0.0
    out = []
    for l in range(layers, 0, -1):
        if r() < 0.7:
            out.append(_c("pre%d" % l, ("pre",)))
        if not no_guest:
            us = log_between(5.0, 120.0) if small_guests and r() < 0.8 else log_between(5.0, 800.0)
            if pile_up:
                us = log_between(5.0, 12.0) if l > 2 else log_between(100.0, 800.0)
            tag = ("guest", us * GUEST_BYTES_PER_US, "as_is") if r() < 0.2 else ("guest", us * GUEST_BYTES_PER_US)
            out.append(_c("g%d" % l, tag, grid=1024 + l))
        out.append(_c("dgrad%d" % l))
        hosts = not no_host and r() >= (0.03 if pile_up else 0.15)
        flop = (log_between(200.0, 900.0) if pile_up else log_between(20.0, 900.0)) * HOST_FLOP_PER_US
        out.append(_c("w%d" % l, ("side", flop) if hosts else ("side",)))
        out.append(_c("red%d" % l, ("reduce",)))
        if r() < p_bucket:
            if r() < 0.4:
                out.append(_c("acc%d" % l, ("accum",)))
            for k in range(1 + int(r() * 3)):
                when = "late" if r() < p_late else pick((None, "early", "early"))
                out.append(_c("x%d_%d" % (l, k), ("xchg", pick((None, "rccl", "proxy")), when)))
    for k in range(int(r() * 3)):
        out.append(_c("fin%d" % k, ("xchg", "finish", None)))
    if r() < 0.4:
        out.append(_c("adv", ("accum", "advance")))
    out.append(["py", _nothing, "opt"])
    out.append(["py", _nothing, "repack"])
    return out


def canonical(plan):
    """A plan as a list of strings: fork, join, py:<label>, or <name>|<tag text>|<a guest's grid argument>."""
    out = []
    for e in plan:
        if e[0] != "c":
            out.append(e[0] if e[0] != "py" else "py:" + (e[2] if len(e) > 2 else "hook"))
            continue
        t = e[4]
        text = "" if t is None else ",".join(repr(v) if isinstance(v, float) else str(v) for v in t)
        grid = ""
        if t is not None and t[0] == "guest" and len(e[2]) >= 2 and isinstance(e[2][-2], ctypes.c_int):
            grid = str(e[2][-2].value)
        out.append("%s|%s|%s" % (e[3], text, grid))
    return out


def digest(plan):
    return hashlib.sha256("\n".join(canonical(plan)).encode()).hexdigest()


def schedule(fn, rec, setting, **kw):
    b, x, c, m = setting
    return fn(rec, cover=c, min_us=m, xchg_at_fork=bool(x), balance=bool(b), **kw)


def _tag(e):
    return e[4] if e[0] == "c" and e[4] is not None else (None,)


def traits(rec, plan, setting):
    """What happened in one plan, read off the recording and the plan alone (names are unique in a recording)."""
    b, x, cover, min_us = setting
    names = [e[3] if e[0] == "c" else e[0] for e in plan]
    pos = {n: i for i, n in enumerate(names)}
    t = {"fork": "fork" in names, "multi": False, "over12": False, "scarce": False, "deferred": False}
    for i, n in enumerate(names):
        if n == "fork":
            j = names.index("join", i)
            g = next(k for k in range(i + 1, j) if _tag(plan[k])[0] == "guest")
            t["multi"] |= j - g - 1 > 1
            t["deferred"] |= g > i + 1                           # exchange entries of earlier hosts between fork and guest
    wants = [(i, cover * _tag(e)[1] / GUEST_BYTES_PER_US) for i, e in enumerate(rec)
             if _tag(e)[0] == "guest" and _tag(e)[1] / GUEST_BYTES_PER_US >= min_us]
    for i, need in wants:
        # held back when the guest was reached: a hosting weight gradient recorded before it and issued behind it
        held = [_tag(e)[1] / HOST_FLOP_PER_US for e in rec[:i] if _tag(e)[0] == "side" and len(_tag(e)) > 1 and pos[e[3]] > pos[rec[i][3]]]
        if not held:
            continue
        if len(held) > 12:
            t["over12"] |= bool(b)
        elif b:
            last = wants[-1][0]
            supply = sum(_tag(e)[1] / HOST_FLOP_PER_US for e in rec[i + 1:last + 1] if _tag(e)[0] == "side" and len(_tag(e)) > 1)
            t["scarce"] |= sum(held) + supply < sum(w for q, w in wants if q >= i)
    return t


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpus():
    """[(seed, recording, [plan per setting])], scheduled once."""
    out = []
    for seed in range(RECORDINGS):
        rec = recording(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out.append((seed, rec, [schedule(P.schedule_guests, rec, s) for s in SETTINGS]))
    return out


# ---------------------------------------------------------------------------------------------------- (a) equivalence
def test_every_corpus_plan_is_the_plan_of_the_commit_the_scheduler_was_split_out_of(golden, corpus):
    assert golden["recordings"] == RECORDINGS >= 300 and [list(s) for s in SETTINGS] == golden["settings"]
    assert len(golden["parent"]) == 40
    bad = [(seed, SETTINGS[k]) for seed, rec, plans in corpus for k, p in enumerate(plans) if digest(p) != golden["plans"][str(seed)][k]]
    assert not bad, "%d of %d plans differ, first: seed %d, (balance, xchg_at_fork, cover, min_us) = %r" % (
        (len(bad), RECORDINGS * len(SETTINGS)) + bad[0])


def test_the_corpus_is_not_degenerate(golden, corpus):
    n = RECORDINGS * len(SETTINGS)
    count = dict.fromkeys(("fork", "multi", "over12", "scarce", "deferred"), 0)
    for seed, rec, plans in corpus:
        for s, p in zip(SETTINGS, plans):
            for k, v in traits(rec, p, s).items():
                count[k] += v
    assert count == golden["traits"], (count, golden["traits"])           # (the generator script's own count, same code)
    assert count["fork"] >= 0.30 * n and count["multi"] >= 0.10 * n, count
    assert count["over12"] >= 0.05 * n and count["scarce"] >= 0.05 * n and count["deferred"] >= 0.05 * n, count
    differ = sum(canonical(plans[k]) != canonical(plans[k + 6]) for _, _, plans in corpus for k in range(6))
    assert differ >= 1, "balance=0 and balance=1 never disagree"
    layers = [sum(1 for e in rec if e[3 if e[0] == "c" else 0].startswith("dgrad")) for _, rec, _ in corpus]
    assert min(layers) == 1 and max(layers) == 16
    assert any(not any(_tag(e)[0] == "guest" for e in rec) for _, rec, _ in corpus)
    assert any(not any(_tag(e)[0] == "side" and len(_tag(e)) > 1 for e in rec) for _, rec, _ in corpus)


# ---------------------------------------------------------------------------------------------------- (b) identity
def test_a_plan_holds_every_recorded_entry_once_and_no_exchange_overtakes_a_weight_gradient(corpus):
    for seed, rec, plans in corpus:
        by_name = {e[3]: e for e in rec if e[0] == "c"}
        for s, plan in zip(SETTINGS, plans):
            what = (seed, s)
            body = [e for e in plan if e[0] not in ("fork", "join")]
            rewritten = [e for e in body if e[0] == "c" and by_name[e[3]] is not e]
            for g in rewritten:
                o = by_name[g[3]]
                assert P.is_paired(g) and not P.is_paired(o) and P.kind(o) == "guest", what
                assert g[:2] == o[:2] and g[3] == o[3] and g[4] == ("guest", o[4][1], "paired") and len(g) == len(o), what
                grid = o[2][0].value if P.keeps_grid(o) else P.GUEST_PAIRED_GRID
                assert len(g[2]) == 2 and g[2][0].value == grid and g[2][1] is o[2][1], what
            gone = {id(by_name[g[3]]) for g in rewritten}
            assert sorted(id(e) for e in body if not any(e is g for g in rewritten)) == sorted(id(e) for e in rec if id(e) not in gone), what
            assert len(rewritten) == len(gone) == sum(1 for e in plan if e[0] == "fork") == sum(1 for e in plan if e[0] == "join"), what
            pos = {(e[3] if e[0] == "c" else id(e)): i for i, e in enumerate(plan)}
            first_side = len(plan)                               # walking the recording backwards: the earliest position
            for e in reversed(rec):                              # in the plan of anything that needs all gradients so far
                k = P.kind(e)
                if k == "side":
                    assert pos[e[3]] < first_side, what + (e[3],)
                elif k in ("xchg", "accum"):                     # (travelling ones too: test_host_cpu's invariant)
                    first_side = min(first_side, pos[e[3]])


# ---------------------------------------------------------------------------------------------------- (c) the fallback
def _pending(n):
    rec = [_c("w%d" % k, ("side", (100.0 + k) * HOST_FLOP_PER_US)) for k in range(n)]
    return rec + [_c("pre", ("pre",)), _c("g", ("guest", 300.0 * GUEST_BYTES_PER_US), 999), _c("dgrad"), ["py", _nothing, "opt"]]


def test_more_than_12_pending_hosts_fall_back_to_the_greedy_choice_with_one_warning():
    rec = _pending(13) + _pending(14)                              # (two guests past the limit: still one warning)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        shared = P.schedule_guests(rec, cover=2.1, min_us=40, balance=True)
    assert len(w) == 1 and "12" in str(w[0].message), [str(x.message) for x in w]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        greedy = P.schedule_guests(rec, cover=2.1, min_us=40, balance=False)
        assert canonical(shared) == canonical(greedy) and "fork" in canonical(greedy)
        twelve = P.schedule_guests(_pending(12), cover=2.1, min_us=40, balance=True)
    assert canonical(twelve).count("fork") == 1


def test_the_fallback_warns_in_exactly_the_corpus_cases_past_the_limit():
    for seed in range(0, RECORDINGS, 7):
        rec = recording(seed)
        for s in SETTINGS:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                plan = schedule(P.schedule_guests, rec, s)
            assert len(w) == int(traits(rec, plan, s)["over12"]), (seed, s)


# ---------------------------------------------------------------------------------------------------- (d) vocabulary
def test_tag_constructors_write_the_stored_tuples_and_the_readers_read_them():
    e = lambda tag: ["c", None, (), "f", tag]
    assert P.side_tag() == ("side",) and P.side_tag(2.6e9) == ("side", 2.6e9)
    assert P.guest_tag(1.0e7) == ("guest", 1.0e7) and P.guest_tag(1.0e7, as_is=True) == ("guest", 1.0e7, "as_is")
    assert P.xchg_tag("rccl", "early") == ("xchg", "rccl", "early") and P.xchg_tag(None, None) == ("xchg", None, None)
    assert P.accum_tag() == ("accum",) and P.accum_tag(advance=True) == ("accum", "advance")
    assert P.pre_tag() == ("pre",) and P.reduce_tag() == ("reduce",)
    assert (P.GUEST_BYTES_PER_US, P.HOST_FLOP_PER_US) == (GUEST_BYTES_PER_US, HOST_FLOP_PER_US)
    # kinds
    assert [P.kind(x) for x in (["fork"], ["join"], ["py", None], ["py", None, "opt"], e(None), e(("pre",)), e(("w4s", 1e9, "fwd")))] == [
        "fork", "join", "py", "py", "c", "pre", "w4s"]
    assert [P.py_label(x) for x in (["py", None], ["py", None, "opt"], ["py", None, "repack"])] == [None, "opt", "repack"]
    # weight gradients
    assert P.kind(e(P.side_tag())) == P.kind(e(P.side_tag(1.0))) == "side"
    assert not P.can_host(e(P.side_tag())) and P.can_host(e(P.side_tag(2.6e9))) and P.host_us(e(P.side_tag(2.6e9))) == 2.0
    assert not P.can_host(e(P.guest_tag(1.0))) and not P.can_host(e(None)) and not P.can_host(["py", None])
    # guests
    g, a = e(P.guest_tag(1.0e7)), e(P.guest_tag(1.0e7, as_is=True))
    p = e(("guest", 1.0e7, "paired"))
    assert P.kind(g) == P.kind(a) == P.kind(p) == "guest" and P.guest_us(g) == P.guest_us(a) == P.guest_us(p) == 2.0
    assert P.guest_us(e(("guest",))) == 0.0
    assert [P.is_paired(x) for x in (g, a, p, e(None), ["fork"])] == [False, False, True, False, False]
    assert [P.keeps_grid(x) for x in (g, a, p)] == [False, True, False]
    # the exchange and the accumulation
    for kind, when in itertools.product((None, "rccl", "proxy", "finish"), (None, "early", "late")):
        x = e(P.xchg_tag(kind, when))
        assert (P.kind(x), P.xchg_kind(x), P.xchg_when(x)) == ("xchg", kind, when)
        assert P.travels(x) == (kind != "finish" and when != "late") and P.needs_all_gradients(x)
    assert (P.xchg_kind(e(("xchg",))), P.xchg_when(e(("xchg", "finish")))) == (None, None)
    assert P.travels(e(("xchg",))) and not P.travels(e(("xchg", "finish")))
    assert P.travels(e(P.accum_tag())) and not P.travels(e(P.accum_tag(advance=True)))
    assert P.needs_all_gradients(e(P.accum_tag())) and P.needs_all_gradients(e(P.accum_tag(advance=True)))
    assert P.needs_all_gradients(["py", None, "opt"]) and P.needs_all_gradients(["py", None])
    assert not any(P.needs_all_gradients(x) or P.travels(x) for x in (e(None), g, e(P.side_tag(1.0)), e(P.reduce_tag()), e(("w4s", 1e9, "fwd"))))
    # the convolutions' (variant, FLOP, phase)
    assert P.is_timed_kernel(e(("w4s", 1e9, "fwd"))) and P.is_timed_kernel(e(("igemm", 1e9, "dgrad")))
    assert not any(P.is_timed_kernel(x) for x in (e(None), g, a, p, e(P.side_tag(1.0)), e(P.xchg_tag("rccl", "early")), e(("pre",)), ["py", None, "opt"]))


def test_kind_is_the_expression_bench_spells_out_on_every_corpus_entry(corpus):
    for seed, rec, plans in corpus:
        for plan in plans:
            by_hand = [e[0] if e[0] != "c" else (e[4][0] if e[4] is not None else "c") for e in plan]
            assert P.kinds(plan) == by_hand == [P.kind(e) for e in plan], seed


def test_train_keeps_the_names_it_had():
    from tensorflow_ocr_amd import train
    assert train.schedule_guests is P.schedule_guests and train._record_audit is P._record_audit and train._VIEW_OPS is P._VIEW_OPS
    for name in ("USE_GUESTS", "GUEST_COVER", "GUEST_PAIRED_GRID", "GUEST_MIN_US", "XCHG_AT_FORK", "GUEST_BALANCE"):
        assert name in vars(train) and getattr(train, name) == getattr(P, name), name
