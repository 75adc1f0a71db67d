"""GPU: the bfloat16 build (libocr_hip_bf16.so, OCR_STORAGE=bf16 — BASELINE.json configs[3] "EAST
ResNet-v1-50 ... bf16").  The storage type is a process-wide choice, so the bf16 checks run in ONE
child interpreter: the conv forward / input-gradient / weight-gradient sweep over every tile variant,
every single-layer parity test, the ResNet blocks and both ResNet graphs, the VGG model end to end,
PixelLinkNet and the train-step tests (replay == eager, Adam/EMA, two ranks in sync), all against the
oracle rounding to bfloat16 at the same storage points (tolerances in those tests: 8x the f16 bars =
the ratio of the two roundings; end to end: the net's own f32-vs-bf16 sensitivity)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bf16_build_layers_models_and_train_step(device):
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_conv_abi.py"),
                        os.path.join(ROOT, "tests", "test_gpu_layers.py"),
                        os.path.join(ROOT, "tests", "test_gpu_resnet.py"),
                        os.path.join(ROOT, "tests", "test_gpu_model_vgg.py"),
                        os.path.join(ROOT, "tests", "test_gpu_pixellink.py"),
                        os.path.join(ROOT, "tests", "test_gpu_train_step.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 45 and "failed" not in r.stdout, tail


def test_bf16_conv_epilogue_matrix(device):
    """tests/test_gpu_conv_epilogues.py (kernel family x epilogue mode against float64) on the bf16 library: every
    case of the matrix passes, at the bf16 bars stated in that file."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        from test_gpu_conv_epilogues import CASES
    finally:
        sys.path.pop(0)
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_conv_epilogues.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(CASES) and "failed" not in r.stdout, tail


def test_bf16_conv_fused_matrix(device):
    """tests/test_gpu_conv_fused_matrix.py (the fused loader, tail and pooled conv entries against float64) on the bf16
    library: every case passes, at the bf16 bounds derived in that file."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        from test_gpu_conv_fused_matrix import N_TESTS
    finally:
        sys.path.pop(0)
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_conv_fused_matrix.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == N_TESTS and "failed" not in r.stdout, tail


def test_bf16_wgrad_matrix(device):
    """tests/test_gpu_wgrad_matrix.py (every weight-gradient family and plan edge against float64) on the bf16 library:
    every case passes at the same bar (bf16 operands and their products are exact in f32 as well)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_wgrad_matrix as W
    finally:
        sys.path.pop(0)
    cases = 2 * len(W.ROWS) + len(W.UNSUPPORTED_SHAPES) + len(W.SLAB_SUM) + 1
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_wgrad_matrix.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    import re
    print("\n".join(re.findall(r"(?:wgrad|slab sum) .*", r.stdout)))
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == cases and "failed" not in r.stdout, tail


def test_bf16_image_conv_matrix(device):
    """tests/test_gpu_image_convs.py (every entry of the first-layer and stem convolutions against float64) on the bf16
    library: every case passes, at the bf16 bars stated in that file."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_image_convs as I
    finally:
        sys.path.pop(0)
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_image_convs.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    import re
    print("\n".join(re.findall(r"image conv .*", r.stdout)))
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == I.N_TESTS and "failed" not in r.stdout, tail


def test_bf16_bn_pool_matrix(device):
    """tests/test_gpu_bn_pool_matrix.py (every batch-norm, pool and unpool entry against float64) on the bf16 library:
    every case passes; the bars scale through the storage half-ulp only."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_bn_pool_matrix as B
    finally:
        sys.path.pop(0)
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_bn_pool_matrix.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    import re
    print("\n".join(re.findall(r"bn_pool .*", r.stdout)))
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == B.N_TESTS and "failed" not in r.stdout, tail


def test_bf16_optim_matrix(device):
    """tests/test_gpu_optim_matrix.py (every entry of optim.hip and s2d.hip against float64) on the bf16 library: every
    case passes; the pack and space-to-depth rows then round to bfloat16, the f32 rows are the same code."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_optim_matrix as P
    finally:
        sys.path.pop(0)
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_optim_matrix.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    import re
    print("\n".join(re.findall(r"optim .*", r.stdout)))
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == P.N_TESTS and "failed" not in r.stdout, tail


def test_bf16_resnet50_east_640_batch64_parity(device):
    """BASELINE configs[3] as quoted (bf16, batch 64, 640^2): n = 64 replicated == n = 2 in the bf16 library."""
    env = dict(os.environ, OCR_STORAGE="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_batch_parity.py"), "-k", "bf16_batch64"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("bf16 n=64")))
    assert r.returncode == 0 and "1 passed" in r.stdout, tail
