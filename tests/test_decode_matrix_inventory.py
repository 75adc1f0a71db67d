"""Host half of tests/test_gpu_decode_matrix.py, no device: the kernel inventory in its docstring against the __global__
names and extern "C" entries of csrc/decode.hip and csrc/boxes.hip; its breadth-first reference against O.link_cc_union
on every link row (labels, counts and the table); and what each row generator promises about its own map."""
import ast
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = {"ocr_py27_dict_order"}         # a host routine, pinned in tests/test_oracle.py


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def M():
    import test_gpu_decode_matrix as M
    return M


def test_every_kernel_and_entry_of_the_decode_files_is_named():
    src = _read("tensorflow_ocr_amd", "csrc", "decode.hip") + _read("tensorflow_ocr_amd", "csrc", "boxes.hip")
    test = _read("tests", "test_gpu_decode_matrix.py")
    doc = ast.get_docstring(ast.parse(test))
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    entries = set(re.findall(r'extern "C" (?:int|size_t) (ocr_\w+)\(', src))
    assert len(kernels) == 22 and len(entries) == 16, (sorted(kernels), sorted(entries))
    templates = set(re.findall(r"template <[^>]*>[^;{]*?__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert templates == {"cc_union_tile_kernel", "mar_border_kernel"} and templates <= kernels
    missing = sorted(k for k in kernels if not re.search(r"\b%s\b" % k, doc))
    assert not missing, "kernels of the decode files that the inventory does not name: %s" % missing
    uncalled = sorted(e for e in entries - HOST_ONLY if '"%s"' % e not in test)
    assert not uncalled, "entries of the decode files that no test calls: %s" % uncalled
    assert all(e in doc for e in HOST_ONLY) and "ocr_py27_dict_order" in _read("tests", "test_oracle.py")


def test_the_direction_table_is_the_kernel_s(M):
    from oracle import ocr_oracle as O
    src = _read("tensorflow_ocr_amd", "csrc", "decode.hip")
    for name, want in (("kDx", M.KDX), ("kDy", M.KDY)):
        got = re.search(r"%s\[8\] = \{([^}]*)\}" % name, src).group(1)
        assert tuple(int(v) for v in got.split(",")) == want
    assert list(zip(M.KDX, M.KDY)) == O.LINK_OFFSETS


def test_link_rows_are_the_ones_the_matrix_names(M):
    names = [r.name for r in M.LINK_ROWS]
    assert len(set(names)) == len(names) == 30
    assert [(r.h, r.w) for r in M.LINK_ROWS[:8]] == [(3, 3), (3, 70), (70, 3), (32, 32), (33, 31), (33, 65), (64, 96), (67, 70)]
    assert all(r.h <= 100 and r.w <= 100 for r in M.LINK_ROWS)
    assert all(m.mask.shape[1] <= 100 and m.mask.shape[2] <= 100 and m.mask.shape[0] <= 3 for m in M.MASK_ROWS)


def test_flood_fill_equals_the_union_find_oracle_on_every_link_row(M):
    from oracle import ocr_oracle as O
    for r in M.LINK_ROWS:
        labels, comps = M.ref_of(r)
        if r.h * r.w > 3000 and r.name.startswith(("singletons-1025", "singletons-16")):
            continue                        # the same map as singletons-4900
        olab, ocomps = O.link_cc_union(r.score, r.link, r.tp, r.tl, r.min_size)
        assert np.array_equal(labels, olab), r.name
        assert comps == ocomps, r.name
        assert labels.dtype == np.int32 and int(labels.max()) == len(comps)


def test_generators_keep_their_promises(M):
    R = {r.name: r for r in M.LINK_ROWS}
    ref = {k: M.ref_of(r) for k, r in R.items()}
    # serpentine: one component held together by one directed link per edge, crossing tile borders again and again
    s = R["serpentine"]
    assert s.crossings >= 20 and ref["serpentine"][1] == [(s.root, s.size)] and s.size == int((s.score > s.tp).sum())
    on = (s.link > s.tl).sum()
    assert on == s.size - 1, "one direction per snake edge"
    # late root: the tile of the smallest index holds under 5 % of the component, and no other tile's first pixel is it
    c = R["late_root"]
    assert c.share < 0.05 and ref["late_root"][1] == [(c.root, c.size)]
    ys, xs = np.nonzero(c.score > c.tp)
    tiles = {(y >> 5, x >> 5) for y, x in zip(ys, xs)}
    assert tiles == {(0, 1), (1, 0), (1, 1)}
    for t in tiles - {(c.root // c.w >> 5, c.root % c.w >> 5)}:
        first = min(y * c.w + x for y, x in zip(ys, xs) if (y >> 5, x >> 5) == t)
        assert first != c.root
    # tile corners: exactly one link joins the blobs, and it crosses both tile borders
    for kind in ("diag", "anti"):
        for way in ("down", "up"):
            r, none = R["corner_%s_%s" % (kind, way)], R["corner_%s_none" % kind]
            extra = np.argwhere((r.link > r.tl) & ~(none.link > none.tl))
            assert len(extra) == 1
            d, y, x = extra[0]
            ny, nx = y + M.KDY[d], x + M.KDX[d]
            assert (y >> 5) != (ny >> 5) and (x >> 5) != (nx >> 5) and M.KDX[d] != 0 and M.KDY[d] != 0
            assert len(ref[r.name][1]) == 1 and ref[r.name][1][0][1] == 18
        assert [c[1] for c in ref["corner_%s_none" % kind][1]] == [9, 9]
    # the border rule
    assert [c[1] for c in ref["border_edge_alone"][1]] == [1] * 8 and [c[1] for c in ref["border_corner_alone"][1]] == [1] * 8
    assert [c[1] for c in ref["border_edge_joined"][1]] == [2] * 4 and [c[1] for c in ref["border_corner_joined"][1]] == [2] * 4
    assert ref["3x3_one"][1] == [(0, 9)] and len(ref["3x3_singletons"][1]) == 9
    # thresholds: every special value occurs on both operands and is negative
    t = R["thresholds"]
    for v in t.values[0]:
        sel = np.isnan(t.score) if np.isnan(v) else t.score == v
        assert sel.any() and ((ref["thresholds"][0][sel] > 0).all() if v > t.tp else not ref["thresholds"][0][sel].any())
    inner = np.zeros(t.score.shape, bool)
    inner[1:-1, 1:-1] = True
    for v in t.values[1]:
        sel = np.isnan(t.link) if np.isnan(v) else t.link == v
        assert (sel & inner & (t.score > t.tp)).any()
    # min_size: k pixels are dropped, k + 1 kept; 0 and -1 keep everything
    assert R["min_size-5"].sizes == [5, 6, 6, 5, 1]
    assert [c[1] for c in ref["min_size-5"][1]] == [6, 6]
    assert [c[1] for c in ref["min_size-0"][1]] == [5, 6, 6, 5, 1] == [c[1] for c in ref["min_size--1"][1]]
    # numbering: kept roots in all five 1024-pixel blocks, the last one ragged, and tables shorter than the count
    for m in (4900, 1025, 16):
        r = R["singletons-%d" % m]
        assert r.max_comps == m and len(ref[r.name][1]) == 4900 and 4900 % 1024 != 0 and -(-4900 // 1024) == 5
    assert ref["fully_linked"][1] == [(0, 4900)]


def test_mask_reference_against_scipy(M):
    from scipy import ndimage
    for row in M.MASK_ROWS:
        for conn in (4, 8):
            st = np.ones((3, 3), int) if conn == 8 else [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
            for value in (0, 1):
                for m in row.mask:
                    labels, comps = M.mask_ref(m, value, conn)
                    slab, k = ndimage.label((m != 0) == (value != 0), structure=st)
                    assert k == len(comps)
                    # the same partition, numbered by first pixel (scipy's raster scan numbers the same way)
                    assert np.array_equal(labels, slab), (row.name, conn, value)
