"""CPU: the operand statements of the decode / label / resize / evaluation / multi-scale / map-fusion / grid / summary
wrappers of `ops`, on the operand sets of tests/golden/make_ops_calls.py with the library stubbed as there.

1. A valid set makes exactly the calls of tests/golden/ops_calls.json, recorded before the wrappers' hand-written checks
   became rows of `ops._operands`: same entries, same argument types and values, same pointers.
2. From each valid set, for every tensor operand in turn: one wrong dimension, a wrong dtype, a non-contiguous view of the
   right shape (two dimensions or more) and None (unless optional) each raise a ValueError that names the wrapper and the
   operand, before the library is reached; every optional operand given as None goes through."""
import importlib.util
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_ops_calls", os.path.join(HERE, "golden", "make_ops_calls.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
SETS = M.operand_sets()
OTHER_DTYPE = {M.F32: M.F64, M.F64: M.F32, M.I32: M.I64, M.I64: M.I32, M.U8: M.I32}


def strided(t):
    """a non-contiguous view with t's shape and dtype, or None when every such view is contiguous"""
    big = [k for k, s in enumerate(t.shape) if s > 1]
    if len(big) < 2:
        return None
    a, b = big[:2]
    shape = list(t.shape)
    shape[a], shape[b] = shape[b], shape[a]
    v = torch.zeros(shape, dtype=t.dtype).transpose(a, b)
    assert tuple(v.shape) == tuple(t.shape) and not v.is_contiguous()
    return v


def faults(name):
    """(operand, kind, arguments) of every fault of wrapper `name`"""
    args = SETS[name]
    for op, t in M.operands(args).items():
        dim = M.DIM.get(name, {}).get(op, -1)
        if dim is not None:
            if dim == "rank":
                bad = t.unsqueeze(-1)
            elif isinstance(dim, tuple):
                bad = torch.zeros(dim, dtype=t.dtype)
            else:
                shape = list(t.shape)
                shape[dim] += 1
                bad = torch.zeros(shape, dtype=t.dtype)
            yield op, "dimension", M.replaced(args, op, bad)
        if op not in M.RAW.get(name, ()):
            yield op, "dtype", M.replaced(args, op, t.to(OTHER_DTYPE[t.dtype]))
        if strided(t) is not None:
            yield op, "layout", M.replaced(args, op, strided(t))
        if op not in M.OPTIONAL.get(name, ()):                       # (a member of an optional tuple is not optional by itself)
            yield op, "None", M.replaced(args, op, None)


def test_a_valid_call_makes_the_recorded_calls():
    with open(M.GOLDEN) as f:
        assert M.dumps(M.record_all()) == f.read()


def test_the_sets_cover_every_wrapper_in_scope_and_every_tensor_parameter():
    import inspect
    from tensorflow_ocr_amd import ops
    assert len(SETS) == 40
    for name, args in SETS.items():
        assert sorted(inspect.signature(getattr(ops, name)).parameters) == sorted(args), name


@pytest.mark.parametrize("name", list(SETS))
def test_every_fault_of_every_operand_is_refused_by_name(name):
    with M.stubbed() as log:
        for op, kind, args in faults(name):
            with pytest.raises(ValueError) as e:
                M.invoke(name, args, log)
            text = str(e.value)
            assert text.startswith(name + ":") and re.search(r"\b%s\b" % op, text), (op, kind, text)
            assert not log, (op, kind, log)


@pytest.mark.parametrize("name", list(M.OPTIONAL))
def test_an_optional_operand_may_be_none(name):
    nulls = lambda calls: sum(a == ["c_void_p", "null"] for a in calls[-1][1])
    with M.stubbed() as log:
        valid = M.invoke(name, SETS[name], log)
        for arg in M.OPTIONAL[name]:
            calls = M.invoke(name, dict(SETS[name], **{arg: None}), log)
            assert nulls(calls) == nulls(valid) + len(M.TUPLES.get(arg, (arg,))) and len(calls) == len(valid)


def test_operands_on_two_devices_are_refused():
    from tensorflow_ocr_amd import ops
    a, b = torch.zeros(4, dtype=M.I64), torch.zeros(1, device="meta")
    with pytest.raises(ValueError, match="tensor_stats: tensors on one device only .*mul_dev"):
        ops._operands("tensor_stats", "n_segments", ("x", a, None, None), ("mul_dev", b, M.F32, 1, ops.OPTIONAL))
