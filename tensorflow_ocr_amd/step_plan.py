"""The recorded training step's PLAN: its vocabulary, its scheduler and its replay walk.

`train.TrainStep` records its third step as a flat list of entries (`_lib.Recorder`):

    ["c", fn, args, name, tag]      a C-ABI call; tag None or one of the tuples below
    ["py", fn] | ["py", fn, label]  a host callback; label "opt" / "repack" for the optimiser and the operand re-pack
    ["fork"] | ["join"]             schedule_guests' markers around a guest / host pair

    ("pre",)                        a guest's coefficient call: stays in front of the fork
    ("guest", bytes)                a batch-norm backward pass that can run as a guest; ("guest", bytes, "as_is") keeps its
                                    recorded grid; ("guest", bytes, "paired") is written by schedule_guests alone
    ("side", FLOP)                  a weight gradient's slab kernel that can host a guest; ("side",) one that cannot
    ("reduce",)                     the slab sum behind it
    ("xchg", kind, when)            the gradient exchange (dist.GradientAllReduce): kind None / "rccl" / "proxy" / "finish",
                                    when None / "early" / "late"
    ("accum",)                      a bucket's (or the whole buffer's) accumulate call; ("accum", "advance") the phase's step
    (variant, FLOP, phase)          a convolution: kernel instantiation, FLOP, "fwd" / "dgrad"

What is stored is read by position elsewhere (bench.py, tests/golden/layer_trace.json) and does not change; inside the
package the tuples are written by the constructors and read by the small functions below, and nowhere else."""
import bisect
import ctypes
import os
import warnings

import torch

_VIEW_OPS = frozenset((
    "empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "view", "_unsafe_view", "reshape",
    "_reshape_alias", "slice", "select", "permute", "transpose", "t", "as_strided", "detach", "alias", "unsqueeze",
    "squeeze", "expand", "narrow", "unbind", "split", "split_with_sizes", "unfold", "view_as_real", "lift_fresh",
    "is_pinned", "_has_compatible_shallow_copy_type", "size", "stride", "sym_size", "sym_stride", "numel", "dim"))


def _record_audit():
    """Dispatch mode for the RECORDED step: the plan holds C-ABI calls only, so a torch operator that
    launches device work inside `forward_loss` (arithmetic on an input, a dtype cast, a `zeros`) would
    run once, at record time, and every replayed step would read its stale result.  Collects the names
    of such operators so `TrainStep` can refuse the recording; views and allocations are fine."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Audit(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.offenders = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func)
            if name not in _VIEW_OPS:
                flat = list(args) + list((kwargs or {}).values()) + (list(out) if isinstance(out, (tuple, list)) else [out])
                if any(isinstance(t, torch.Tensor) and t.is_cuda for t in flat):
                    self.offenders.append(name)
            return out
    return Audit()


# The switches.  `train` imports them by name and TrainStep hands train's values to schedule_guests, so that a test (or a
# caller) that sets train.GUEST_MIN_US changes the next recording; schedule_guests called without them uses these.
USE_GUESTS = os.environ.get("OCR_GUEST_STREAM", "1") == "1"


GUEST_COVER = float(os.environ.get("OCR_GUEST_COVER", "2.1"))
GUEST_PAIRED_GRID = int(os.environ.get("OCR_GUEST_PAIRED_GRID", "256"))
GUEST_MIN_US = float(os.environ.get("OCR_GUEST_MIN_US", "40"))
# a completed bucket's exchange entries at the NEXT fork instead of right behind the join that followed its last weight
# gradient: the comm kernel then starts beside held-back weight gradients (456 of 512 registers: the
# only kernels of the step it can share a CU with) instead of beside the next input-gradient launch (512: it cannot).
# Measured with the one-GPU stand-ins (bench.py exchange.proxy_at_fork): 1.34 -> 1.23 ms of the stand-in's 1.10-1.19 ms
# exposed per step, either footprint; on.  (Issuing an exchange entry later than recorded is always correct.)
XCHG_AT_FORK = os.environ.get("OCR_XCHG_AT_FORK", "1") == "1"
# hosts shared out with the guests still to come in view (round 6): the greedy choice covered conv2_1's apply pass with two
# weight gradients (791 us for a 577 us pass) and left conv1_2's pooled pass — the last and largest — 306 us of host for 585,
# 0.28 ms exposed on the critical path (profiles/r05_guest_pairs_trace.txt).  0: the round-5 greedy choice (A/B).
GUEST_BALANCE = os.environ.get("OCR_GUEST_BALANCE", "1") == "1"

GUEST_BYTES_PER_US = 5.0e6       # a guest pass alone: its bytes at 5 TB/s (measured rates: profiles/r05_guest_pairs.json)
HOST_FLOP_PER_US = 1.3e9         # a weight gradient's slab kernel: its FLOP at 1.3 PFLOP/s
BALANCE_MAX_PENDING = 12         # the balanced choice enumerates the subsets of the pending hosts: 4095 at the most


# ------------------------------------------------------------------------------------------------ the vocabulary: writers
def pre_tag():
    return ("pre",)


def guest_tag(nbytes, as_is=False):
    return ("guest", nbytes, "as_is") if as_is else ("guest", nbytes)


def side_tag(flop=None):
    return ("side",) if flop is None else ("side", flop)


def reduce_tag():
    return ("reduce",)


def xchg_tag(kind, when):
    return ("xchg", kind, when)


def accum_tag(advance=False):
    return ("accum", "advance") if advance else ("accum",)


def kernel_tag(variant, flop, phase):
    return (variant, flop, phase)


# ------------------------------------------------------------------------------------------------ the vocabulary: readers
def _tag(e):
    return e[4] if (e[0] == "c" and e[4] is not None) else (None,)


def kind(e):
    """"fork" / "join" / "py"; for a call the first element of its tag, "c" for an untagged one."""
    if e[0] != "c":
        return e[0]
    return "c" if e[4] is None else e[4][0]


def kinds(plan):
    return [kind(e) for e in plan]


def amount(e):
    """The tag's figure — a convolution's or a weight gradient's FLOP, a guest's bytes — or None."""
    t = _tag(e)
    return t[1] if len(t) > 1 else None


def note(e):
    """The tag's third element — a convolution's phase, a guest's "as_is" / "paired", an exchange entry's `when` — or ""."""
    t = _tag(e)
    return t[2] if len(t) > 2 else ""


def py_label(e):
    return e[2] if (e[0] == "py" and len(e) > 2) else None


def can_host(e):
    t = _tag(e)
    return t[0] == "side" and len(t) >= 2


def host_us(e):
    return e[4][1] / HOST_FLOP_PER_US


def guest_bytes(e):
    t = _tag(e)
    return t[1] if (t[0] == "guest" and len(t) > 1) else 0.0


def guest_us(e):
    """A guest's stand-alone time; 0 for one recorded without a byte count."""
    t = e[4]
    return (t[1] / GUEST_BYTES_PER_US) if len(t) > 1 else 0.0


def is_paired(e):
    t = _tag(e)
    return t[0] == "guest" and t[-1] == "paired"


def keeps_grid(e):
    return e[4][-1] == "as_is"


def xchg_kind(e):
    return e[4][1] if len(e[4]) > 1 else None


def xchg_when(e):
    return e[4][2] if len(e[4]) > 2 else None


def travels(e):
    """An exchange entry that belongs to the weight gradient in front of it.  A bucket's accumulate call (GradAccum.run)
    sits in front of its exchange entries and travels like them: it reads every weight gradient recorded before it; the
    step's one advance call does not."""
    t = _tag(e)
    if t[0] == "accum":
        return len(t) < 2
    return t[0] == "xchg" and (len(t) < 2 or t[1] != "finish") and (len(t) < 3 or t[2] in (None, "early"))


def needs_all_gradients(e):
    """Host callbacks (optimiser, torch-mode exchange), the exchange's entries and the accumulate calls: a bucket's
    all-reduce and its accumulate call read every weight gradient recorded before them, the held-back ones included."""
    return e[0] != "c" or _tag(e)[0] in ("xchg", "accum")


def is_timed_kernel(e):
    """A convolution's (kernel instantiation, FLOP, phase)."""
    t = _tag(e)
    return len(t) > 2 and t[0] not in ("side", "guest", "xchg")


# ------------------------------------------------------------------------------------------------ the scheduler
def _segment(entries, cover, min_us):
    """One pass over the recording -> (kinds, tail, ahead, wants, supplies):
    tail[i]    may entry i follow a held-back weight gradient as part of its tail (slab sum, a weight gradient that cannot
               host, a travelling exchange / accumulate entry);
    ahead[i]   is there a guest behind entry i, before anything that needs the gradients;
    wants      [(index, cover x time)] of the guests long enough to be paired, supplies [(index, time)] of the hosting
               weight gradients, both in recording order (`_outlook` sums slices of them)."""
    ks = kinds(entries)
    n = len(entries)
    tail, ahead, wants, supplies = [False] * n, [False] * n, [], []
    seen = False                     # the scan's answer from entry q on
    for q in range(n - 1, -1, -1):
        e, k = entries[q], ks[q]
        ahead[q] = seen
        moves = travels(e)
        if k == "guest":
            seen = True
        elif e[0] != "c" or (k in ("xchg", "accum") and not moves):
            seen = False
        tail[q] = k == "reduce" or (k == "side" and not can_host(e)) or moves
    for q in range(n):
        e = entries[q]
        if ks[q] == "guest" and len(e[4]) > 1 and e[4][1] / GUEST_BYTES_PER_US >= min_us:
            wants.append((q, cover * e[4][1] / GUEST_BYTES_PER_US))
        elif can_host(e):
            supplies.append((q, host_us(e)))
    return ks, tail, ahead, wants, supplies


def _outlook(i0, wants, supplies):
    """(what the guests from entry i0 on want of hosts, us; what the weight gradients recorded behind i0 and in front of
    the last of those guests will supply, us), each summed in recording order."""
    if not wants or wants[-1][0] < i0:
        return 0.0, 0.0
    last = wants[-1][0]
    want = sum(w for _, w in wants[bisect.bisect_left(wants, (i0,)):])
    supply = sum(s for _, s in supplies[bisect.bisect_right(supplies, (i0, float("inf"))):bisect.bisect_right(supplies, (last, float("inf")))])
    return want, supply


# A pending host is (head, tail, us, closes): the slab kernel's entry, what was recorded behind it, its estimated time and
# whether its weight gradient completed an exchange bucket.  Such a host may only go once every weight gradient recorded
# before it has gone: the bucket's all-reduce (and its accumulate call) reads all of them.
def choose_hosts_balanced(pending, need, want, supply):
    """What is exposed of a guest is what its hosts do not cover, and every host a guest can use the later guests can use
    too: when the guests still to come want more than all hosts can give, each gets its SHARE (target), and the subset of
    the pending hosts whose sum is closest to the target goes — a miss either way costs a guest (this one or a later one)
    the same; with hosts to spare, covering counts.  -> indices into `pending`, ascending."""
    us = [p[2] for p in pending]
    have = sum(us) + supply
    scarce = have < want
    target = need * have / want if scarce else need
    closers = [k for k, p in enumerate(pending) if p[3]]
    best = None
    for m in range(1, 1 << len(pending)):
        if any(m >> k & 1 and m & ((1 << k) - 1) != (1 << k) - 1 for k in closers):
            continue
        ks = [k for k in range(len(pending)) if m >> k & 1]
        tot = sum(us[k] for k in ks)
        miss = abs(tot - target) if scarce else (2.0 * (target - tot) if tot < target else 0.25 * (tot - target))
        key = (miss, len(ks), ks)
        if best is None or key < best[0]:
            best = (key, ks, tot)
    return best[1] if best is not None and best[2] <= 3.0 * need else []


def choose_hosts_greedy(pending, need):
    """Oldest first, as many as cover the guest without a large overshoot (the round-5 choice)."""
    take, acc, skipped = [], 0.0, False
    for k, (_, _, us, closes) in enumerate(pending):
        if acc >= 0.85 * need:
            break
        if acc + us <= 1.3 * need and not (skipped and closes):
            take.append(k)
            acc += us
        else:
            skipped = True
    return take


def smallest_admissible_host(pending, need):
    """Where a choice took nothing: the single smallest host that may go, unless it outlasts the guest 3 times over."""
    k = min((q for q in range(len(pending)) if q == 0 or not pending[q][3]), key=lambda q: pending[q][2])
    return [k] if pending[k][2] <= 3.0 * need else []


def _paired_guest(e, paired_grid):
    """The guest entry as it runs beside hosts: tagged "paired" and, unless it keeps its grid, with the entry point's
    `max_workgroups` (second to last argument) at one workgroup per CU."""
    g = list(e)
    g[4] = ("guest", guest_bytes(e), "paired")
    if len(e[2]) >= 2 and not keeps_grid(e):
        g[2] = tuple(e[2][:-2]) + (ctypes.c_int(paired_grid),) + (e[2][-1],)
    return g


def _emit_pair(out, pending, deferred, guest, take, xchg_at_fork):
    """fork, [the exchange of buckets completed by EARLIER hosts: it starts with these hosts], guest, hosts, join, the
    hosts' tails — their exchange entries to `deferred` instead when they wait for the next fork."""
    out.append(["fork"])
    out.extend(deferred)
    del deferred[:]
    out.append(guest)
    hosts = [pending[k] for k in take]
    for k in reversed(take):
        del pending[k]
    out.extend(h[0] for h in hosts)
    out.append(["join"])
    for h in hosts:
        for te in h[1]:
            (deferred if (xchg_at_fork and kind(te) == "xchg") else out).append(te)


def _flush(out, pending, deferred):
    out.extend(deferred)         # (recorded before anything still pending: their buckets are complete)
    del deferred[:]
    for p in pending:
        out.append(p[0])
        out.extend(p[1])
    del pending[:]


def schedule_guests(entries, cover=None, min_us=None, xchg_at_fork=None, balance=None, paired_grid=None):
    """Run the HBM-bound batch-norm backward passes of the recorded step as GUESTS beside its weight gradients
    (csrc/guest_bn.hip; measured rates: profiles/r05_guest_pairs.json).

    Recorded order (layers._conv_backward, layers.conv2d): ... coefficients(L) ["pre"], apply(L) ["guest", bytes],
    dgrad(L), wgrad(L) = slab kernel ["side", FLOP] + slab sum ["reduce"], [exchange entries of the bucket that wgrad(L)
    completed], coefficients(L-1), apply(L-1), ...  The chain apply -> dgrad -> apply is the critical path; a weight
    gradient depends on its layer's apply pass only, and nothing but the optimiser (and the exchange) waits for it.
    So weight gradients are HELD BACK and spent as hosts: at every guest the plan forks, the guest goes to the second
    stream, and held-back slab kernels go to the main stream — chosen, oldest first, so that their estimated time
    covers `cover` x the guest's stand-alone time without overshooting it by much (beside a host a guest moves ~0.42 of
    its stand-alone rate, the host keeps ~0.9 of its own: small guests take small hosts, the deep layers' weight
    gradients — little HBM traffic of their own — are left for the large passes of conv2 / conv1, which come last) —
    then the plan joins: the next input-gradient kernel owns the whole register file and would only time-slice with a
    straggler.  The slab sums (and whatever was recorded behind them: a re-layout of the gradient, the exchange entries
    of the bucket it completed) follow the join: alone they take 13 us, beside a streaming guest 60-370.  A guest's
    waves (<= 56 registers per lane) are placed beside the weight gradient's resident workgroups (456 of 512).  What is
    still held back when something needs the gradients (the exchange's closing entries, the optimiser, any host
    callback) is issued there, in order; a guest with nothing to run beside stays on the main stream.  Exchange entries
    issued later than recorded are always correct: they order the comm stream behind the compute stream at that
    point."""
    cover = GUEST_COVER if cover is None else cover
    min_us = GUEST_MIN_US if min_us is None else min_us
    xchg_at_fork = XCHG_AT_FORK if xchg_at_fork is None else xchg_at_fork
    balance = GUEST_BALANCE if balance is None else balance
    paired_grid = GUEST_PAIRED_GRID if paired_grid is None else paired_grid
    ks, tail, ahead, wants, supplies = _segment(entries, cover, min_us)
    out, pending, i, n = [], [], 0, len(entries)
    deferred = []                # exchange entries of hosts already run, waiting for the next fork (xchg_at_fork)
    warned = False
    while i < n:
        e, k = entries[i], ks[i]
        if k == "side" and can_host(e) and ahead[i]:
            j = i + 1
            while j < n and tail[j]:
                j += 1
            pending.append((e, entries[i + 1:j], host_us(e), any(ks[q] in ("xchg", "accum") for q in range(i + 1, j))))
            i = j
            continue
        if k == "side" and can_host(e):
            out.extend(deferred)             # no guest left to host (a net without batch norm: every call stays in place, and
            del deferred[:]                  # the exchange sees its buckets as early as it was recorded): no fork will come
        elif k == "guest" and pending and guest_us(e) >= min_us:      # (a fork + join costs the main queue ~25 us of idle time)
            need = cover * guest_us(e)
            if balance and len(pending) <= BALANCE_MAX_PENDING:
                take = choose_hosts_balanced(pending, need, *_outlook(i, wants, supplies))
            else:
                if balance and not warned:
                    warned = True
                    warnings.warn("schedule_guests: more than %d weight gradients held back at one guest; the balanced "
                                  "choice of hosts falls back to the greedy one there" % BALANCE_MAX_PENDING, stacklevel=2)
                take = choose_hosts_greedy(pending, need)
            take = take or smallest_admissible_host(pending, need)
            if take:
                _emit_pair(out, pending, deferred, _paired_guest(e, paired_grid), take, xchg_at_fork)
                i += 1
                continue
        elif k != "guest" and needs_all_gradients(e):
            # also an exchange entry that TRAVELS behind a weight gradient which stayed in place (one that cannot host, or
            # conv1_1's sums form): the held-back weight gradients of its bucket go first
            _flush(out, pending, deferred)
        out.append(e)                        # (a weight gradient that cannot host, ops.conv2d_wgrad, stays in place too)
        i += 1
    _flush(out, pending, deferred)
    return out


# ------------------------------------------------------------------------------------------------ the replay walk
class Replay:
    """What one replayed step's walk needs besides the plan: the two streams (guest_*: None while the plan has no fork),
    the reducer, whether the step closes its accumulation window, bench.py's end-of-backward event, ops.KERNEL_TIMING."""

    def __init__(self, main, guest_stream, guest_ptr, guest_event, reducer, closing, backward_end_event, timing):
        self.main, self.guest_stream, self.guest_ptr, self.guest_event = main, guest_stream, guest_ptr, guest_event
        self.reducer, self.closing, self.backward_end_event, self.timing = reducer, closing, backward_end_event, timing
        self.backward_marked = False

    def mark_backward_end(self):
        """Once per step: the end of backward on the compute stream."""
        if self.backward_end_event is not None and not self.backward_marked:
            self.backward_end_event.record(self.main)
            self.backward_marked = True


def _run(e, args=None):
    from . import _lib
    rc = e[1](*(e[2] if args is None else args))
    if rc != 0:
        _lib.check(rc, e[3])


_OWN_BRANCH = frozenset(("fork", "join", "py", "xchg", "guest"))


def run_plan(plan, plan_kinds, ctx):
    """Issue every entry of `plan` (plan_kinds: kinds(plan), computed when the plan was set), in order."""
    from . import _lib
    main, reducer, closing, timing = ctx.main, ctx.reducer, ctx.closing, ctx.timing
    for e, k in zip(plan, plan_kinds):
        if k in _OWN_BRANCH:
            if k == "fork":
                # a weight gradient and the guest pass paired with it (schedule_guests): the guest stream starts here
                ctx.guest_event.record(main)
                ctx.guest_stream.wait_event(ctx.guest_event)
                continue
            if k == "join":
                main.wait_stream(ctx.guest_stream)
                continue
            if k == "py":
                label = e[2] if len(e) > 2 else None
                if not closing and label in ("opt", "repack"):
                    continue                                      # a micro-step inside its window: gradients only
                if label == "opt":
                    ctx.mark_backward_end()                       # (no exchange in this step: backward ends here)
                e[1]()
                continue
            if k == "xchg":
                # the gradient exchange as C-ABI calls (dist.GradientAllReduce, abi mode); once per window
                if not (reducer.enabled and closing):
                    continue
                what, when = xchg_kind(e), xchg_when(e)
                # a bucket's comm-stream launch: the RCCL all-reduce OR its one-GPU stand-in (dist: proxy)
                if (what == "proxy" and not reducer.use_proxy) or (what == "rccl" and reducer.use_proxy):
                    continue
                # a plan that holds both placements of the exchange (under backward / after it) runs one
                if when is not None and when != ("early" if reducer.overlap else "late"):
                    continue
                if what == "finish" or when == "late":
                    ctx.mark_backward_end()
                _run(e)
                continue
            if e[4][-1] == "paired":                              # a guest beside its hosts: on the guest stream
                _run(e, e[2][:-1] + (ctx.guest_ptr,))
                continue
        # every other call (an unpaired guest among them) as it was recorded.  The call and its status check stand here
        # and not in _run: this is the branch nearly every entry takes
        if timing is not None and is_timed_kernel(e):
            t = e[4]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = e[1](*e[2])
            e1.record()
            timing.append((t[0], t[1], t[2], e0, e1))
        else:
            rc = e[1](*e[2])
        if rc != 0:
            _lib.check(rc, e[3])
