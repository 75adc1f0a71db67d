"""GPU (for the CU count only: nothing is launched or allocated): the selection of csrc/conv_igemm.hip — which kernel
runs a descriptor, how many partial rows the caller must allocate, how many workgroups the conv1_2 weight-gradient
form leaves blocks for — pinned against tests/golden/conv_plan.json, the answers ocr_conv2d_variant,
ocr_conv2d_num_mtiles and ocr_conv2d_bnred_first_wgrad_blocks gave BEFORE the three became readers of one ConvPlan
(recorded by tests/golden/make_conv_plan.py on an MI355X, status codes included).  A name that drifts from the row
count is an out-of-bounds write of partial rows in the product, so every row must agree in all three.

The table: every shape of test_gpu_conv_abi.SHAPES and test_gpu_conv_epilogues.FAMILIES and the layers of the two
benchmark nets, forward and input-gradient form, and the edges of every rule — 127 / 128 pixel tiles, pointwise pixel
counts that are and are not multiples of 32, cin 32 / 64 / 96, cout 32 ... 256, 8 and 9 output rows, dilation 6,
stride 2, 2^31 bytes per image, null / zero / negative fields.  The persistent 64-channel kernel sizes its grid by
the CU count: on a device with another count than the recording's its row and block counts are not compared."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "conv_plan.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def answers(device):
    """[(recorded row, the library's answers now)]; the recording is the default selection's (no OCR_CONV_* switch set)."""
    import sys
    import torch
    from tensorflow_ocr_amd import _lib as L
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        from make_conv_plan import query
    finally:
        sys.path.pop(0)
    same_cus = torch.cuda.get_device_properties(device).multi_processor_count == GOLDEN["cus"]
    return same_cus, [(r, query(L, r["desc"])) for r in GOLDEN["rows"]]


def test_table_covers_the_conv_tests_shapes():
    """Every shape the ABI sweep and the epilogue matrix launch is a row, in both forms."""
    from tensorflow_ocr_amd import ops
    from test_gpu_conv_abi import SHAPES
    from test_gpu_conv_epilogues import FAMILIES
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        from make_conv_plan import forms
    finally:
        sys.path.pop(0)
    have = {tuple(r["desc"]) for r in GOLDEN["rows"] if r["desc"] is not None}
    for s in [s[:7] for s in SHAPES] + [s for _, s in FAMILIES.values()]:
        for d in forms(ops, *s):
            assert tuple(d) in have, s
    names = {r["variant"]: r["desc"] for r in GOLDEN["rows"]}
    for s in SHAPES:
        assert s[7] in names
    for name, _ in FAMILIES.values():
        assert name in names


def test_variant_names_and_status_codes(answers):
    _, rows = answers
    bad = [(r["desc"], (r["variant_rc"], r["variant"]), (g["variant_rc"], g["variant"])) for r, g in rows
           if (r["variant_rc"], r["variant"]) != (g["variant_rc"], g["variant"])]
    assert not bad, bad[:8]


def test_partial_row_and_block_counts(answers):
    same_cus, rows = answers
    compared = 0
    bad = []
    for r, g in rows:
        if r["variant"].startswith("conv_c64_persist_kernel") and not same_cus:
            continue
        compared += 1
        if (r["num_mtiles"], r["wgrad_blocks"]) != (g["num_mtiles"], g["wgrad_blocks"]):
            bad.append((r["desc"], (r["num_mtiles"], r["wgrad_blocks"]), (g["num_mtiles"], g["wgrad_blocks"])))
    assert compared >= 250 and not bad, bad[:8]
