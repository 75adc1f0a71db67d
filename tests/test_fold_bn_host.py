"""CPU: the host side of the folded inference batch norm (Graph(fold_bn=True)) — the conv2d_same geometry the strided layers
are launched with (ops.conv2d_same_geometry against the oracle's conv2d_same, nets/resnet_utils.py:74-123), the C ABI's
declaration and exports, and test.py's flag."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import ocr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("size", [15, 16, 20, 33])
def test_conv2d_same_geometry_matches_the_oracle(size, k):
    """(out, pad) gives the oracle's output shape, and the first and last outputs of a ramp image under an asymmetric integer
    kernel (exact in f32, so a pad on the wrong side or an output grid shifted by one shows as another integer)."""
    from tensorflow_ocr_amd import ops
    stride = 2
    out, pad = ops.conv2d_same_geometry(size, k, stride)
    x = np.arange(1, size * size + 1, dtype=np.float64).reshape(size, size)
    w = np.arange(1, k * k + 1, dtype=np.float64).reshape(k, k)
    ref = O.conv2d_same(torch.from_numpy(x.astype(np.float32))[None, :, :, None],
                        torch.from_numpy(w.astype(np.float32))[:, :, None, None], stride)
    assert tuple(ref.shape) == (1, out, out, 1)
    xp = np.zeros((size + 2 * k, size + 2 * k))
    xp[pad:pad + size, pad:pad + size] = x
    for o in (0, out - 1):
        got = float((xp[o * stride:o * stride + k, o * stride:o * stride + k] * w).sum())
        assert got == float(ref[0, o, o, 0]), (size, k, o)
    # stride 1 is TF SAME, and the strided form is the [::s] subsample of it
    assert ops.conv2d_same_geometry(size, k, 1) == ops.same_pad(size, k, 1)
    full = O.conv2d_same(torch.from_numpy(x.astype(np.float32))[None, :, :, None],
                         torch.from_numpy(w.astype(np.float32))[:, :, None, None], 1)
    assert torch.equal(full[:, ::stride, ::stride], ref)
    d = ops.conv2d_same_desc((1, size, size, 1), 8, k, stride)
    assert (d.oh, d.ow, d.pad_top, d.pad_left, d.stride) == (out, out, pad, pad, stride)


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", txt))


def test_epilogue_entry_points_are_declared_and_exported_by_both_product_libraries():
    from tensorflow_ocr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    names = ["ocr_conv2d_f32_mfma_ep", "ocr_conv2d_f32_split_ep", "ocr_subsample_f32"]
    assert set(names) <= _declared("ocr_hip.h") and not set(names) & _declared("ocr_verify.h")
    here = os.path.dirname(_lib.LIB_PATH)
    for lib in ("libocr_hip.so", "libocr_hip_bf16.so"):
        so = ctypes.CDLL(os.path.join(here, lib))
        assert not [n for n in names if not hasattr(so, n)], lib
        so.ocr_abi_version.restype = ctypes.c_int
        assert so.ocr_abi_version() == _lib.ABI_VERSION == 7            # new entry points do not bump it
    hdr = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    for name, val in (("OCR_CONV_AFFINE", 16), ("OCR_CONV_RESIDUAL", 32), ("OCR_CONV_ACCUM_IN", 64)):
        assert re.search(r"\b%s = %d\b" % (name, val), hdr), name
    assert (_lib.CONV_AFFINE, _lib.CONV_RESIDUAL, _lib.CONV_ACCUM_IN) == (16, 32, 64)


def _script():
    spec = importlib.util.spec_from_file_location("ocr_test_script", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_fold_bn_flag(monkeypatch):
    """--fold-bn / --no-fold-bn; with --precision f16 the flag is ignored and Graph gets no fold_bn at all."""
    T = _script()
    for argv, want in ((["--precision", "f16x2", "--fold-bn"], {"precision": "f16x2", "fold_bn": True}),
                       (["--precision", "f32", "--no-fold-bn"], {"precision": "f32", "fold_bn": False}),
                       (["--precision", "f16", "--fold-bn"], {"precision": "f16"}),
                       ([], {"precision": "f16"})):
        monkeypatch.setattr("sys.argv", ["test.py"] + argv)
        fl = T.parse()
        assert T.graph_kwargs(fl.precision, fl.fold_bn) == want, argv
    for prec in ("f32", "f16x2"):
        monkeypatch.setattr("sys.argv", ["test.py", "--precision", prec])
        fl = T.parse()
        assert fl.fold_bn is None and T.graph_kwargs(prec, fl.fold_bn) == {"precision": prec, "fold_bn": T.FOLD_BN_DEFAULT[prec]}
