"""CPU: what tests/test_gpu_optim_matrix.py rests on.  The inventory in its docstring against the __global__ names and
extern "C" entries of csrc/optim.hip and csrc/s2d.hip; its update bounds from both sides — on every update row's operands
each of the ten near misses of the kernel's formula (MUTATIONS) lies at least 4x outside the bound in some element of
some output, and the kernel's own sequence restated operation by operation in f32, without contraction, stays inside it —
and its integer round-to-nearest-even restatement against the conversion `_h` uses, for both storage types.

A mutation that IS the kernel's formula on a row cannot be seen there and is asserted to be the identity instead:
`i <= n_reg` at n_reg = n; the four that move, drop or rescale the decay term at n_reg = 0 (and `i < n_reg - 1` is
`i < n_reg` there); the two EMA ones on the rows that pass no EMA buffer; beta2-for-m and eps-in-the-root are Adam's,
the folded learning rate is Momentum's."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_optim_matrix as M
from matrix_support import f32, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_kernel_and_entry_of_the_optimiser_files_is_named():
    src = _read("tensorflow_ocr_amd", "csrc", "optim.hip") + _read("tensorflow_ocr_amd", "csrc", "s2d.hip")
    test = _read("tests", "test_gpu_optim_matrix.py")
    doc = ast.get_docstring(ast.parse(test))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    entries = set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', src))
    assert len(kernels) == 16 + 4 and len(entries) == 24 + 4, (sorted(kernels), sorted(entries))
    missing = sorted(k for k in kernels if not re.search(r"\b%s\b" % k, doc))
    assert not missing, "kernels of the optimiser files that the inventory does not name: %s" % missing
    called = set(re.findall(r'"(ocr_\w+)"', test)) | set(M.ENTRY.values())          # (the six steps are named by M.ENTRY)
    assert set(M.ENTRY.values()) <= entries
    uncalled = sorted(entries - called)
    assert not uncalled, "entries of the optimiser files that no test calls: %s" % uncalled


def test_the_test_count_the_bf16_child_checks():
    tree = ast.parse(_read("tests", "test_gpu_optim_matrix.py"))
    names = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")]
    assert len(names) == len(set(names)) == 16                    # (a second definition of a name would hide the first)
    assert M.N_TESTS == 116


# ------------------------------------------------------------------------------------------------ the bound discriminates
def _applies(mut, kind, ema, n, n_reg):
    if mut == "reg_le":
        return n_reg < n
    if mut in ("reg_lt_minus_1", "no_decay", "decay_after_moments", "scale_after_decay"):
        return n_reg >= 1
    if mut in ("ema_old_w", "ema_decay_swapped"):
        return ema
    return kind == ("mom" if mut == "lr_in_accumulator" else "adam")


def _subset(n, n_reg):
    """every element of a small row; of the large one both ends, the workgroup cap and the neighbourhood of n_reg.  The
    step is elementwise, so a reference on a subset IS the reference there."""
    if n <= 4096:
        return np.arange(n)
    parts = [np.arange(512), np.arange(n - 512, n), np.arange(256 * 4096 - 8, 256 * 4096 + 5), np.arange(max(n_reg - 8, 0), min(n_reg + 8, n))]
    return np.unique(np.concatenate(parts))


def _take(o, idx):
    return M.NS(**{k: v[idx] for k, v in vars(o).items()})


def _f32_step(kind, o, idx, n_reg, s, ema):
    """the kernel's own sequence, every operation rounded to f32, nothing fused"""
    H = M.HP[kind]
    reg = idx < n_reg
    one = f32(1)
    gs = o.g * s
    gi = np.where(reg, gs + H.wd * o.w, gs)
    out = {}
    if kind == "adam":
        out["m"] = H.b1 * o.m + (one - H.b1) * gi
        out["v"] = H.b2 * o.v + (one - H.b2) * gi * gi
        out["w"] = o.w - H.lr * out["m"] / (np.sqrt(out["v"]) + H.eps)
    else:
        out["m"] = H.mom * o.m + gi
        out["w"] = o.w - H.lr * out["m"]
    if ema:
        out["ema"] = o.ema - (one - H.decay) * (o.ema - out["w"])
    assert all(v.dtype == f32 for v in out.values())
    return out


def _worst(got, ref, bnd):
    return max(float((np.abs(got[k].astype(f64) - ref[k]) / bnd[k]).max()) for k in ref)


@pytest.mark.parametrize("kind,form,ema,n", M.UPDATE_ROWS, ids=["%s-%s-%s-n%d" % (k, f, "ema" if e else "noema", n) for k, f, e, n in M.UPDATE_ROWS])
def test_update_bound_sees_every_mutation_and_holds_the_f32_restatement(kind, form, ema, n):
    o_all, s = M._operands(kind, n), M._factor(form)
    for n_reg in M._nregs(n):
        full = form == "plain" or n <= 4096                   # the three forms differ in the scalar s alone
        idx = np.arange(n) if full else _subset(n, n_reg)
        o = _take(o_all, idx)
        ref, bnd = M.update_ref(kind, o, idx, n_reg, s, ema)
        assert all((b > 0).all() and np.isfinite(b).all() for b in bnd.values())
        faithful = _worst(_f32_step(kind, o, idx, n_reg, s, ema), ref, bnd)
        assert faithful <= 1.0, (n_reg, faithful)
        sub = _subset(n, n_reg)
        pos = np.searchsorted(idx, sub)
        o_s, ref_s, bnd_s = _take(o, pos), {k: v[pos] for k, v in ref.items()}, {k: v[pos] for k, v in bnd.items()}
        seen = {}
        for mut in M.MUTATIONS:
            mref, _ = M.update_ref(kind, o_s, sub, n_reg, s, ema, mut)
            assert set(mref) == set(ref_s)
            if _applies(mut, kind, ema, n, n_reg):
                seen[mut] = _worst(mref, ref_s, bnd_s)
                assert seen[mut] >= 4.0, (n_reg, mut, seen[mut])
            else:
                assert all(np.array_equal(mref[k], ref_s[k]) for k in ref_s), (n_reg, mut)
        print("n_reg %d: f32 restatement %.3f of the bound; smallest mutation %s %.3g" % (
            (n_reg, faithful) + min(seen.items(), key=lambda kv: kv[1])))


def test_every_mutation_is_seen_somewhere_and_the_list_is_the_whole_list():
    assert len(M.MUTATIONS) == len(set(M.MUTATIONS)) == 10
    for mut in M.MUTATIONS:
        rows = [(k, e, n, r) for k, _, e, n in M.UPDATE_ROWS for r in M._nregs(n) if _applies(mut, k, e, n, r)]
        assert len(rows) >= 24, (mut, len(rows))


# ------------------------------------------------------------------------------------------------ the rounding restatement
@pytest.mark.parametrize("kind,dtype", [("f16", torch.float16), ("bf16", torch.bfloat16)])
def test_rne_restatement_is_the_storage_rounding(kind, dtype):
    """directed operands, one f32 ulp either side of each, and a random sample over the whole exponent range"""
    d = M.directed(kind)
    bits = d.view(np.uint32).astype(np.int64)
    near = np.concatenate([bits, bits + 1, bits - 1]) & 0xFFFFFFFF
    rng = np.random.default_rng(20)
    x = np.concatenate([near.astype(np.uint32), rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)]).view(f32)
    want = torch.from_numpy(x).to(dtype).view(torch.int16).numpy().view(np.uint16)
    got = M._rne(x, kind)
    nan = np.isnan(x)
    assert nan.any() and np.array_equal(M._isnan16(got, kind), nan) and np.array_equal(M._isnan16(want, kind), nan)
    assert np.array_equal(got[~nan], want[~nan])
    as_f = torch.from_numpy(got.view(np.int16)).view(dtype).float().numpy()
    rounds_up, rounds_down = (np.abs(as_f) > np.abs(x))[~nan].sum(), (np.abs(as_f) < np.abs(x))[~nan].sum()
    assert rounds_up > 100 and rounds_down > 100 and np.isinf(as_f[~nan & np.isfinite(x)]).any()        # no truncation, no clamp
    dd = M._rne(d, kind).astype(np.int64)
    sub = (dd & (0x7C00 if kind == "f16" else 0x7F80)) == 0
    assert (sub & ((dd & 0x7FFF) != 0)).sum() >= 8 and (sub & ((dd & 0x7FFF) == 0) & (d != 0)).sum() >= 4   # subnormal results; flushes to 0 by rounding
    if M.KIND16 == kind:
        assert np.array_equal(M.matrix_support._h(x[~nan]).view(np.int32), as_f[~nan].view(np.int32))   # _h itself
