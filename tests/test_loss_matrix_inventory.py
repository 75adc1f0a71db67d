"""The kernel inventory in the docstring of tests/test_gpu_loss_matrix.py against the __global__ names and extern "C"
entries of csrc/loss_softmax.hip and csrc/loss_dice.hip: a kernel or an entry that no row names fails here."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_kernel_and_entry_of_the_loss_files_is_named():
    src = _read("tensorflow_ocr_amd", "csrc", "loss_softmax.hip") + _read("tensorflow_ocr_amd", "csrc", "loss_dice.hip")
    test = _read("tests", "test_gpu_loss_matrix.py")
    doc = ast.get_docstring(ast.parse(test))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    entries = set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', src))
    assert len(kernels) == 17 and len(entries) == 15, (sorted(kernels), sorted(entries))
    missing = sorted(k for k in kernels if not re.search(r"\b%s\b" % k, doc))
    assert not missing, "kernels of the loss files that the inventory does not name: %s" % missing
    uncalled = sorted(e for e in entries if '"%s"' % e not in test)
    assert not uncalled, "entries of the loss files that no test calls: %s" % uncalled
