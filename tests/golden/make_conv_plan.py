"""Records tests/golden/conv_plan.json: for a table of convolution descriptors, what the library's three selection
queries answer — ocr_conv2d_variant (status + name), ocr_conv2d_num_mtiles and ocr_conv2d_bnred_first_wgrad_blocks —
together with the device's CU count (the persistent 64-channel kernel sizes its grid, and so its partial rows, by it).
tests/test_gpu_conv_plan.py compares the library against the file: run this on the commit whose selection is to be
kept, BEFORE changing the host code below the kernels of csrc/conv_igemm.hip.  Needs the GPU (the CU count); launches
nothing and allocates nothing.

    python tests/golden/make_conv_plan.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

FIELDS = ("n", "h", "w", "cin", "oh", "ow", "cout", "kh", "kw", "stride", "dilation", "pad_top", "pad_left", "flip_taps", "flags")


def forms(ops, n, h, w, cin, cout, k, dil=1, stride=1):
    """The forward descriptor (SAME padding) and, at stride 1, the input-gradient one (layers._conv_dgrad's pads)."""
    d = ops.conv_desc((n, h, w, cin), cout, k, k, stride, dil)
    out = [[int(getattr(d, f)) for f in FIELDS]]
    if stride == 1:
        out.append([n, h, w, cout, h, w, cin, k, k, 1, dil, dil * (k - 1) - d.pad_top, dil * (k - 1) - d.pad_left, 1, 0])
    return out


def table(ops):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    import test_gpu_conv_abi as A
    import test_gpu_conv_epilogues as E
    import w4_layers
    from bench_configs import VGG_512_B8_LAYERS
    shapes = [s[:7] for s in A.SHAPES] + [s for _, s in E.FAMILIES.values()]
    # the headline step (model_vgg, 32 x 512^2) and the inference table (8 x 512^2); conv1_1 is conv_first.hip's
    shapes += [(w4_layers.N, hw, hw, ci, co, 3) for _, hw, ci, co in w4_layers.FWD]
    shapes += [(n, hw, hw, ci, co, k, rate) for n in (8, 32) for _, hw, ci, co, k, rate in VGG_512_B8_LAYERS if ci % 32 == 0]
    # ResNet-v1-50 at 64 x 640^2: per stage (map size, bottleneck width), the unit's 1x1 / 3x3 / 1x1, the next unit's
    # 1x1 on its output, the projection shortcut and the strided 3x3 that ends the stage
    for hw, c in ((160, 64), (80, 128), (40, 256), (20, 512)):
        shapes += [(64, hw, hw, c, c, 1), (64, hw, hw, c, c, 3), (64, hw, hw, c, 4 * c, 1), (64, hw, hw, 4 * c, c, 1),
                   (64, hw, hw, 2 * c, 4 * c, 1), (64, hw, hw, c, c, 3, 1, 2), (64, hw, hw, 2 * c, c, 1, 1, 2)]
    # edges: 127 / 128 pixel tiles (the persistent kernel's threshold)
    shapes += [(1, 1016, 32, 64, 64, 3), (1, 1024, 32, 64, 64, 3), (1, 1016, 32, 64, 192, 3), (1, 1024, 32, 64, 192, 3)]
    # pointwise pixel counts that are and are not multiples of 32
    shapes += [(1, 8, 8, 128, 128, 1), (1, 9, 7, 128, 128, 1), (3, 16, 10, 64, 256, 1), (3, 17, 11, 64, 256, 1)]
    # channel counts across every tile width and chunk size
    shapes += [(1, 16, 32, ci, co, k) for k in (1, 3) for ci in (32, 64, 96) for co in (32, 64, 128, 160, 256)]
    # 8 and 9 output rows (the 16-row candidates), a large map per tile width
    shapes += [(1, oh, 32, ci, 128, 3) for oh in (8, 9) for ci in (64, 96)] + [(2, 256, 256, ci, co, 3) for ci in (64, 96) for co in (64, 128)]
    # dilation 6: the halo of the 64-channel chunk does not fit beside a 256-cout ring
    shapes += [(8, 32, 32, 512, 1024, 3, 6), (1, 32, 32, 256, 256, 3, 6), (1, 32, 32, 128, 128, 3, 6), (1, 32, 32, 64, 64, 3, 6)]
    # stride 2
    shapes += [(2, 18, 36, 64, 64, 3, 1, 2), (2, 32, 32, 128, 128, 1, 1, 2)]
    # 2^31 bytes per image and one column either side (the persistent kernel's buffer descriptors)
    shapes += [(1, 4096, w, 64, 64, 3) for w in (4095, 4096, 4097)]
    rows, seen = [], set()
    for s in shapes:
        for d in forms(ops, *s):
            if tuple(d) not in seen:
                seen.add(tuple(d))
                rows.append(d)
    # refused descriptors: null, zero and negative extents, channel counts no tile divides
    base = forms(ops, 2, 16, 32, 64, 64, 3)[0]
    rows.append(None)
    for f, v in (("n", 0), ("n", -1), ("h", 0), ("w", -4), ("oh", 0), ("ow", -1), ("kh", 0), ("kw", -3), ("stride", 0),
                 ("stride", -1), ("dilation", 0), ("dilation", -2), ("cin", 16), ("cin", 48), ("cout", 16), ("cout", 80)):
        d = list(base)
        d[FIELDS.index(f)] = v
        rows.append(d)
    pw = forms(ops, 2, 16, 32, 64, 64, 1)[0]
    for f, v in (("n", 0), ("n", -1), ("dilation", 0), ("dilation", -1)):          # ... on a pointwise shape
        d = list(pw)
        d[FIELDS.index(f)] = v
        rows.append(d)
    return rows


def query(L, fields):
    """-> {"variant_rc", "variant", "num_mtiles", "wgrad_blocks"} of one descriptor (None: the null pointer)."""
    d = None if fields is None else ctypes.byref(L.ConvDesc(*fields))
    buf = ctypes.create_string_buffer(96)
    rc = int(L._fn("ocr_conv2d_variant", ctypes.c_int)(d, buf, ctypes.c_size_t(96)))
    return {"variant_rc": rc, "variant": buf.value.decode() if rc == 0 else "",
            "num_mtiles": int(L._fn("ocr_conv2d_num_mtiles", ctypes.c_int)(d)),
            "wgrad_blocks": int(L._fn("ocr_conv2d_bnred_first_wgrad_blocks", ctypes.c_int)(d))}


def main():
    sys.path.insert(0, ROOT)
    import torch
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd import ops
    rows = [{"desc": d, **query(L, d)} for d in table(ops)]
    out = {"fields": list(FIELDS), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "rows": rows}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_plan.json")
    with open(path, "w") as f:
        f.write('{"fields": %s,\n "cus": %d,\n "rows": [\n  %s\n ]}\n' % (
            json.dumps(out["fields"]), out["cus"], ",\n  ".join(json.dumps(r) for r in rows)))
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
