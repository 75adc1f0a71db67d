"""CPU: host side of global-norm gradient clipping — `clip_norm` validation on both optimiser constructors, the training
scripts' `--clip_norm` flag, and the C ABI's declarations.  (The rule itself runs on the device:
tests/test_gpu_grad_clip.py.)"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ocr_grad_clip_init", "ocr_grad_clip_workspace", "ocr_grad_clip_f32", "ocr_grad_check_clip_f32",
               "ocr_adam_step_clip", "ocr_momentum_step_clip"]


def _tower(loss_scale=1024.0):
    from tensorflow_ocr_amd import graph as G
    g = G.Graph("cpu", loss_scale=loss_scale, seed=2)
    with g.variable_scope("feature_fusion"):
        g.get_variable("Conv/weights", (1, 1, 4, 3), G.xavier_uniform(g.rng), regularized=True)
        g.get_variable("Conv/biases", (3,), G.constant(0.5))
    return g


@pytest.mark.parametrize("which", ["adam", "momentum"])
def test_clip_norm_validation_on_the_optimiser_constructors(which):
    from tensorflow_ocr_amd import ops
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer
    cls = AdamOptimizer if which == "adam" else MomentumOptimizer
    off = cls(_tower())
    assert off.clip is None
    with pytest.raises(RuntimeError):
        off.grad_norm()
    for ok in (1.0, 5, np.float32(0.25), 1e30):
        opt = cls(_tower(), clip_norm=ok)
        assert opt.clip is not None and opt.clip.clip_norm == float(ok)
        # the block and the partials exist from the constructor on, the block zeroed
        assert opt.clip.state.numel() == ops.GRAD_CLIP_WORDS and int(opt.clip.state.abs().sum()) == 0
        assert opt.clip.ws.numel() * 8 >= ops.grad_clip_workspace(opt.g.store.flat_grad.numel()) >= 8
        assert opt.grad_norm() == 0.0 and opt.clipped_steps() == 0 and opt.nonfinite_steps() == 0
    for bad in (0, 0.0, -1.0, float("inf"), float("-inf"), float("nan"), "1.0", True, [1.0], 1e39):
        with pytest.raises(ValueError):
            cls(_tower(), clip_norm=bad)


@pytest.mark.parametrize("script", ["multigpu_train", "train_pixellink"])
def test_scripts_parse_the_clip_norm_flag(script):
    import importlib
    mod = importlib.import_module(script)
    assert mod.parse([]).clip_norm is None                                      # off by default
    v = mod.parse(["--clip_norm", "2.5"]).clip_norm
    assert isinstance(v, float) and v == 2.5
    assert mod.parse(["--clip_norm", "1e3", "--loss_scale", "dynamic"]).clip_norm == 1000.0
    for bad in ("0", "-1", "inf", "nan", "much"):
        with pytest.raises(SystemExit):
            mod.parse(["--clip_norm", bad])


def test_header_declares_every_new_symbol_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "ocr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ocr_[a-z0-9_]+)\s*\(", code))
    assert not [s for s in NEW_SYMBOLS if s not in declared]
    assert re.search(r"#define OCR_ABI_VERSION 7\b", txt)
    # the state block: eight 32-bit words in the order the host indexes them
    m = re.search(r"typedef struct \{([^}]*)\}\s*ocr_grad_clip_state;", code)
    assert m
    fields = re.findall(r"\b(?:float|uint32_t)\s+(\w+);", m.group(1))
    assert fields == ["g_mul", "norm", "coef", "skip", "clipped_total", "nonfinite_total", "ticket", "reserved"]
    from tensorflow_ocr_amd import ops
    assert [ops.GC_G_MUL, ops.GC_NORM, ops.GC_COEF, ops.GC_SKIP, ops.GC_CLIPPED_TOTAL, ops.GC_NONFINITE_TOTAL,
            ops.GC_TICKET] == [fields.index(f) for f in fields[:7]]


def test_both_product_libraries_export_the_new_symbols_and_size_the_workspace():
    import ctypes
    from tensorflow_ocr_amd import _lib
    for name in ("libocr_hip.so", "libocr_hip_bf16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)], name
        ws = lib.ocr_grad_clip_workspace
        ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int64]
        sizes = [ws(n) for n in (1, 4, 1027, 1028, 1 << 20, 1 << 40)]
        assert sizes[0] == sizes[1] == sizes[2] == 8                # one workgroup: one f64 partial
        assert sizes[3] == 16 and sizes == sorted(sizes)
        assert sizes[-1] == ws(1 << 50) and sizes[-1] % 8 == 0      # capped: the grid cap times 8 bytes
