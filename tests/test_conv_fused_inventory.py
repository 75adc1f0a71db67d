"""The launch entries of csrc/conv_igemm.hip against the two matrix files that call them directly
(tests/test_gpu_conv_epilogues.py through its ops wrappers, tests/test_gpu_conv_fused_matrix.py through the C ABI): an
entry that neither calls fails here, and so does a row of the fused matrix that its docstring does not list."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# checked bit-exactly and against a float64 dW in test_gpu_conv_abi.py; the conv1_1 fusions are in flux
EXEMPT = {"ocr_conv2d_bnred_first_f16", "ocr_conv2d_bnred_first_wgrad_f16"}
ROWS = ["a64", "a128r", "a480", "a256sw", "a256", "amax", "b128", "b128r", "b256o", "b256sw",
        "t_pw", "t_pw64", "t_ig1", "t_w4", "t_w4s", "t_16row", "t_c64"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_launch_entry_of_conv_igemm_is_called():
    src = _read("tensorflow_ocr_amd", "csrc", "conv_igemm.hip")
    epilogues = _read("tests", "test_gpu_conv_epilogues.py")
    fused = _read("tests", "test_gpu_conv_fused_matrix.py")
    entries = set(re.findall(r'extern "C" int (ocr_conv2d_(?:\w+_)?f16)\(', src))
    assert len(entries) >= 10 and EXEMPT <= entries, sorted(entries)
    uncalled = sorted(e for e in entries - EXEMPT
                      if '"%s"' % e not in fused and not re.search(r"\bops\.%s\(" % e[len("ocr_"):-len("_f16")], epilogues))
    assert not uncalled, "entries of conv_igemm.hip that neither matrix calls: %s" % uncalled


def test_every_row_is_listed_in_the_docstring():
    fused = _read("tests", "test_gpu_conv_fused_matrix.py")
    doc = ast.get_docstring(ast.parse(fused))
    missing = [r for r in ROWS if not re.search(r"(?<![\w])%s(?![\w])" % r, doc)]
    assert not missing, "rows the docstring does not list: %s" % missing
    # ... and the tables of the file hold exactly these rows
    for r in ROWS:
        assert re.search(r'^    "%s": \(' % r, fused, re.M), r
