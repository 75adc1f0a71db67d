"""Host: what the ten convolution wrappers of ops.py hand to the library and to the recorder — entry point, argument
count (descriptor first, stream last) and the (variant, FLOP, phase) tag train.schedule_guests and bench.py read —
with L.call, conv2d_variant, the recorder and the HIP events replaced by fakes.  The expected values are the wrappers'
behaviour before they became callers of one helper, written down as literals: the operand-transforming 1x1 entries
rename conv_pw_kernel to conv_pwx_kernel, only conv2d and conv2d_relu_pool are bracketed by events under
KERNEL_TIMING, and their tuple is the tag followed by the two events."""
import pytest

from tensorflow_ocr_amd import _lib as L
from tensorflow_ocr_amd import ops

F3 = 2.0 * 2 * 8 * 16 * 128 * 64 * 9      # the 3x3 descriptor below: 37748736 FLOP
F1 = 2.0 * 2 * 8 * 16 * 128 * 64          # the 1x1 descriptor
assert (F3, F1) == (37748736.0, 4194304.0)
PW, PWX = "conv_pw_kernel<128,2>", "conv_pwx_kernel<128,2>"      # the fake conv2d_variant answers PW for every descriptor

BN = (None, None, None, None, None, True)               # bn_ctx
FIRST = (None, None, None, None, None, None, True)      # first_ctx
TAIL = (None, None, None, None, None)                   # tail_ctx with mask bits
COEF = (None, None, None)

# wrapper: (descriptor kind, arguments after the descriptor, entry point, number of C arguments, tag)
CASES = {
    "conv2d": ("3x3", (None, None, None), "ocr_conv2d_f16", 7, (PW, F3, "fwd")),
    "conv2d_dgrad": ("3x3flip", (None, None, None, None, None), "ocr_conv2d_f16", 7, (PW, F3, "dgrad")),
    "conv2d_relu_pool": ("3x3", (None, None, None, None), "ocr_conv2d_relu_pool_f16", 7, (PW, F3, "fwd")),
    "conv2d_bnred": ("3x3", (None, None, None, None, BN, True), "ocr_conv2d_bnred_f16", 13, (PW, F3, "dgrad")),
    "conv2d_bnred_first": ("3x3", (None, None, None, None, FIRST), "ocr_conv2d_bnred_first_f16", 13, (PW, F3, "dgrad")),
    "conv2d_bnred_first_wgrad": ("3x3", (None, None, None, FIRST, None), "ocr_conv2d_bnred_first_wgrad_f16", 13, (PW, F3, "dgrad")),
    "conv2d_bnred_tail": ("3x3", (None, None, None, None, TAIL, None), "ocr_conv2d_bnred_tail_f16", 12, (PW, F3, "dgrad")),
    "conv2d_pw_bnaddrelu": ("1x1", (None,) * 11, "ocr_conv2d_pw_bnaddrelu_f16", 13, (PWX, F1, "fwd")),
    "conv2d_pw_bnrelu": ("1x1", (None,) * 7, "ocr_conv2d_pw_bnrelu_f16", 9, (PWX, F1, "fwd")),
    "conv2d_pw_bnbwd_bnred": ("1x1", (None, None, COEF, None, None, None, None, BN), "ocr_conv2d_pw_bnbwd_bnred_f16", 17, (PWX, F1, "dgrad")),
    "conv2d_pw_bnbwd_tail": ("1x1", (None, None, COEF, None, None, None, None, None, TAIL, None), "ocr_conv2d_pw_bnbwd_tail_f16", 18,
                             (PWX, F1, "dgrad")),
}
TIMED = ("conv2d", "conv2d_dgrad", "conv2d_relu_pool")


def _desc(kind):
    d = ops.conv_desc((2, 8, 16, 64), 128, 1, 1) if kind == "1x1" else ops.conv_desc((2, 8, 16, 64), 128, 3, 3)
    if kind == "3x3flip":
        d.flip_taps = 1
    return d


@pytest.fixture
def fakes(monkeypatch):
    """-> log: ("call", name, args) per library call and ("event", id) per recorded event, in order."""
    log = []

    def call(name, *args):
        log.append(("call", name, args))
        if L.RECORDER is not None:
            L.RECORDER.c(None, args, name)
        return 0

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            log.append(("event", self))

    monkeypatch.setattr(L, "call", call)
    monkeypatch.setattr(ops, "conv2d_variant", lambda d: PW)
    monkeypatch.setattr(ops, "_st", lambda: "stream")
    monkeypatch.setattr(ops.torch.cuda, "Event", Event)
    monkeypatch.setattr(ops, "KERNEL_TIMING", None)
    monkeypatch.setattr(L, "RECORDER", None)
    return log


def _run(case):
    kind, args, _, _, _ = CASES[case]
    d = _desc(kind)
    getattr(ops, "conv2d" if case == "conv2d_dgrad" else case)(d, *args)
    return d


@pytest.mark.parametrize("case", list(CASES))
def test_entry_point_arguments_and_recorded_tag(fakes, monkeypatch, case):
    _, _, entry, nargs, tag = CASES[case]
    rec = L.Recorder()
    monkeypatch.setattr(L, "RECORDER", rec)
    d = _run(case)
    assert [e[:2] for e in fakes] == [("call", entry)]
    args = fakes[0][2]
    assert len(args) == nargs and args[0]._obj is d and args[-1] == "stream"
    assert len(rec.entries) == 1
    kind_, fn_, args_, name_, tag_ = rec.entries[0]
    assert (kind_, name_, args_) == ("c", entry, args)
    assert tag_ == tag and type(tag_[1]) is float


@pytest.mark.parametrize("case", list(CASES))
def test_without_a_recorder_the_call_is_all(fakes, case):
    _, _, entry, nargs, _ = CASES[case]
    _run(case)
    assert [(e[1], len(e[2])) for e in fakes] == [(entry, nargs)]


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_timing_brackets_one_call_between_two_events(fakes, monkeypatch, case):
    _, _, entry, _, tag = CASES[case]
    timing = []
    monkeypatch.setattr(ops, "KERNEL_TIMING", timing)
    rec = L.Recorder()
    monkeypatch.setattr(L, "RECORDER", rec)
    _run(case)
    if case not in TIMED:                 # only the plain and the pooled entry are timed
        assert [e[:2] for e in fakes] == [("call", entry)] and timing == []
    else:
        assert [e[0] for e in fakes] == ["event", "call", "event"] and fakes[1][1] == entry
        assert len(timing) == 1 and timing[0][:3] == tag
        assert timing[0][3:] == (fakes[0][1], fakes[2][1]) and fakes[0][1] is not fakes[2][1]
    assert rec.entries[0][4] == tag
