"""CPU: the inventory of tests/test_gpu_infer_matrix.py against the __global__ names and extern "C" entries of
csrc/f32_infer.hip and csrc/f16x2_infer.hip, and a check that the matrix's split-route reference can see what it claims to
see: on three of its rows, with their keys, an emulation that drops one correction product or the 2^-11 misses bound (a)
by 8x or more, while the faithful emulation accumulated in f32 in another order stays inside it."""
import ast
import os
import re

import numpy as np
import pytest

import test_gpu_infer_matrix as M
from matrix_support import _g, f32, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEING_ROWS = ["P255", "P257", "k1x3"]                   # K = 7, 9, 24: the 8x below is a condition on this choice


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_kernel_and_entry_of_the_inference_files_is_named():
    src = _read("tensorflow_ocr_amd", "csrc", "f32_infer.hip") + _read("tensorflow_ocr_amd", "csrc", "f16x2_infer.hip")
    test = _read("tests", "test_gpu_infer_matrix.py")
    doc = ast.get_docstring(ast.parse(test))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    entries = set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', src))
    assert len(kernels) == 10 and len(entries) == 13, (sorted(kernels), sorted(entries))
    missing = sorted(k for k in kernels if not re.search(r"\b%s\b" % k, doc))
    assert not missing, "kernels of the inference files that the inventory does not name: %s" % missing
    uncalled = sorted(e for e in entries if '"%s"' % e not in test)
    assert not uncalled, "entries of the inference files that no test calls: %s" % uncalled


def _f32_emulation(x, w, r):
    """the split sum as the device forms it, every step in f32, taps walked from the LAST to the first"""
    xh, xl = (M._cols(p, r).astype(f32) for p in M.split_planes(x))
    wh, wl = (p.reshape(r.K, r.cout).astype(f32) for p in M.split_planes(w))
    main, corr = np.zeros((r.P, r.cout), f32), np.zeros((r.P, r.cout), f32)
    for k in reversed(range(r.K)):
        main += xh[:, k, None] * wh[None, k]             # a product of two halves is exact in f32
        corr += xl[:, k, None] * wh[None, k]
        corr += xh[:, k, None] * wl[None, k]
    return main + corr * f32(2.0 ** -11)


@pytest.mark.parametrize("rid", SEEING_ROWS)
def test_split_reference_sees_a_missing_term(rid):
    r, o, _, S, Smag, m_sum = M._case("split", rid, "random")           # asserts bound (b) on the way
    assert r.K <= 96 and m_sum == 3 * r.K + 1
    bound = _g(m_sum) * Smag
    worst = {}
    for name, kw in (("without xlo' whi", dict(terms=(1, 1, 0))), ("without xhi wlo'", dict(terms=(1, 0, 1))),
                     ("without the 2^-11", dict(corr=1.0))):
        worst[name] = float((np.abs(M.split_sum(o.x, o.w, r, **kw)[0] - S) / bound).max())
    faithful = float((np.abs(_f32_emulation(o.x, o.w, r).astype(f64) - S) / bound).max())
    print("row %s (K = %d): faithful f32 emulation %.3f of bound (a); %s" % (
        rid, r.K, faithful, ", ".join("%s %.1f" % kv for kv in worst.items())))
    assert faithful <= 1.0
    assert all(v >= 8.0 for v in worst.values()), worst


@pytest.mark.parametrize("rid", SEEING_ROWS + ["wide", "wide3"])
def test_split_truncation_bound(rid):
    """bound (b): the split sum S against the float64 convolution, for ordinary and for wide-range operands"""
    for kind in ("random", "wide", "wide_2^-10") if rid.startswith("wide") else ("random",):
        r, o, o64, S, _, _ = M._case("split", rid, kind)
        true = M._cols(o64.x, r) @ o64.w.reshape(r.K, r.cout)
        b, _ = M.split_truncation_bound(o.x, o.w, r)
        ratio = float((np.abs(S - true) / b).max())
        print("row %s/%s: |S - conv| <= %.3f of bound (b)" % (rid, kind, ratio))
        assert ratio <= 1.0


def test_single_rounding_reference():
    """_fma32 against exact rational arithmetic, ties included"""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(f32)
    b = rng.standard_normal(4000).astype(f32)
    c = rng.standard_normal(4000).astype(f32)
    a[:4], b[:4] = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12)             # 1 + 2^-11 + 2^-24: half way, decided by c
    c[:4] = [0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -30]
    got = M._fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], f32(-np.inf)), np.nextafter(got[i], f32(np.inf))
        e = abs(exact - Fraction(float(got[i])))
        assert e <= abs(exact - Fraction(float(lo))) and e <= abs(exact - Fraction(float(hi))), i
    assert got[1] != got[2]                                             # the float64 sum alone would round both the same way
