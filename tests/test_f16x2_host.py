"""CPU: the host side of the f16x2 inference precision — the split / recombine emulation of scripts/f16x2_emulate.py (what
the device kernel computes, with its roundings), the C ABI's declaration and exports, and the command-line choice."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulate():
    spec = importlib.util.spec_from_file_location("f16x2_emulate", os.path.join(ROOT, "scripts", "f16x2_emulate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_split_recombine_accuracy_and_why_lo_is_scaled():
    E = _emulate()
    # N(0,1) . N(0,1)/sqrt(K), K = 27: as accurate as an f32 GEMM
    x, w = E.operands("normal", 27)
    ref = x.astype(np.float64) @ w.astype(np.float64)
    e = E.rel_err(E.split_matmul(x, w), ref)
    print("normal K=27: scaled split %.2e" % e)
    assert e <= 1e-6
    assert E.rel_err(E.split_matmul(x, w, correction=False), ref) > 1e-4      # hi*hi alone is an f16 GEMM
    # per-element magnitudes over 8 / 3 decades, K = 4608
    x, w = E.operands("wide", 4608)
    ref = x.astype(np.float64) @ w.astype(np.float64)
    e = E.rel_err(E.split_matmul(x, w), ref)
    print("wide K=4608: scaled split %.2e" % e)
    assert e <= 4e-6
    # without the 2^11 factor the residual planes fall into the half subnormals: small activations lose the correction
    x, w = E.operands("normal_small_x", 4608)
    ref = x.astype(np.float64) @ w.astype(np.float64)
    e_s, e_u = E.rel_err(E.split_matmul(x, w), ref), E.rel_err(E.split_matmul(x, w, scaled=False), ref)
    print("x * 2^-16, K=4608: scaled %.2e, unscaled %.2e" % (e_s, e_u))
    assert e_s <= 4e-6 and e_u > 1e-4


def test_split_planes_are_finite_and_exact_where_they_can_be():
    E = _emulate()
    v = np.array([0.0, 1.0, -1.0, 1.0 + 2.0 ** -12, 0.1, 65504.0, 7e4, -1e30, 2.0 ** -20], dtype=np.float32)
    hi, lo = E.split(v)
    assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
    back = hi.astype(np.float64) + lo.astype(np.float64) / 2048.0
    inside = np.abs(v) <= 65504.0
    assert np.abs(back[inside] - v[inside].astype(np.float64)).max() <= 2.0 ** -22 * np.abs(v[inside]).max()
    assert float(hi[6]) == 65504.0 and float(hi[7]) == -65504.0                  # saturated, not infinite


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", txt))


def test_split_conv_is_declared_and_exported_by_both_product_libraries_only():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    names = ["ocr_conv2d_f32_split", "ocr_conv2d_f32_split_workspace"]
    assert set(names) <= _declared("ocr_hip.h") and not set(names) & _declared("ocr_verify.h")
    here = os.path.dirname(_lib.LIB_PATH)
    for lib in ("libocr_hip.so", "libocr_hip_bf16.so"):
        so = ctypes.CDLL(os.path.join(here, lib))
        assert not [n for n in names if not hasattr(so, n)], lib
    ver = ctypes.CDLL(_lib.VERIFY_LIB_PATH)
    assert not [n for n in names if hasattr(ver, n)]
    # the size query needs no GPU: room for at least the two half planes of the unpadded weights, 16-byte granular (tile
    # and chunk padding are the kernel's business)
    so = ctypes.CDLL(_lib.LIB_PATH)
    so.ocr_conv2d_f32_split_workspace.restype = ctypes.c_size_t
    for cin, cout, k in ((130, 200, 3), (3, 64, 3), (1024, 1024, 1)):
        d = _lib.ConvDesc(1, 16, 16, cin, 16, 16, cout, k, k, 1, 1, 1, 1, 0, 0)
        n = so.ocr_conv2d_f32_split_workspace(ctypes.byref(d))
        assert n >= k * k * cin * cout * 2 * 2 and n % 16 == 0, (cin, cout, k, n)
    d = _lib.ConvDesc(1, 16, 16, 0, 16, 16, 64, 3, 3, 1, 1, 1, 1, 0, 0)
    assert so.ocr_conv2d_f32_split_workspace(ctypes.byref(d)) == 0                        # invalid descriptor
    d = _lib.ConvDesc(1, 16, 16, 3, 16, 16, 64, 3, 3, 1, 1, 1, 1, 0, 0)
    so.ocr_conv2d_f32_split.restype = ctypes.c_int
    assert so.ocr_conv2d_f32_split(ctypes.byref(d), None, None, None, None, None, ctypes.c_size_t(0), None) == -1


def test_cli_lists_f16x2():
    """test.py --help (argparse only, no GPU).  test_pixellink.py / test_pixellink_fast.py keep their argument lists; they
    reach the same convolutions through OCR_F32_CONV=split with --precision f32 (next test)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "f16x2" in r.stdout


def test_env_selects_the_split_route_for_f32_graphs():
    env = dict(os.environ, OCR_F32_CONV="split")
    r = subprocess.run([sys.executable, "-c", "from tensorflow_ocr_amd import ops; print(ops.F32_CONV)"],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "split", r.stderr[-2000:]
