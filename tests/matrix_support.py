"""What the matrix files (test_gpu_*_matrix.py, test_gpu_conv_epilogues.py, test_gpu_image_convs.py) share: a plain
module, no fixtures and no hooks.  A new matrix file gets from it the status codes and rounding units of the storage
type, the keyed generator its operands are drawn from, the comparisons against a float64 reference (_bits_equal,
_ratio, _note), guarded device buffers (Guard, Strided, or carve for a band sized in elements) and the ctypes plumbing
to call a C-ABI entry with them (_a, _rc, _raw, _p, _items).  Its rows, its float64 references and the derivation of
every bound stay in the file itself.

Two rules.  The key passed to _rng / _seed is part of the test: it selects the operands every recorded ratio was
measured on, so a call site's key tuple is never edited.  And the checks here are strict by default: where copies of a
helper once differed in what they asserted the shared one asserts both, and a row that needs the looser form asks for
it with an argument at its call site and says there why.
"""
import ctypes
import zlib

import numpy as np
import torch

from oracle import ocr_oracle as O

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
F16, BF16 = O.STORAGE == torch.float16, O.STORAGE == torch.bfloat16
U16 = 2.0 ** -11 if F16 else 2.0 ** -8
TINY = 2.0 ** -24 if F16 else 2.0 ** -133
U32 = 2.0 ** -24
f32, f64 = np.float32, np.float64
BAND = 512                              # bytes on each side of a Guard
SENT16, SENT32 = 0x5EED, 0x5EEDF00D     # the band words of carve
NAN16, NAN32 = 0x7FBE, 0x7FC0BEEF       # quiet NaNs with a payload in f16, bf16 and f32 (f64: NAN32 twice): "still what the test wrote"
SZ, FL, I64, DB = ctypes.c_size_t, ctypes.c_float, ctypes.c_int64, ctypes.c_double


# ------------------------------------------------------------------------------------------------ host helpers
def _h(a):
    """round to the library's 16-bit storage type"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(O.STORAGE).float().numpy()


def _z(a):
    """bit pattern with a zero's sign dropped"""
    return (np.asarray(a, f32) + f32(0)).view(np.int32)


def _g(m):
    m = np.asarray(m, f64)
    return m * U32 / (1.0 - m * U32)


def _cdiv(a, b):
    return -(-a // b)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _rng(*key):
    return np.random.default_rng(_seed(*key))


def _exact32(v):
    v32 = np.asarray(v, f64).astype(f32)
    assert np.array_equal(v32.astype(f64), np.asarray(v, f64)), "the reference itself must be exact in f32"
    return v32


def _bits_equal(got, ref, what, skip=None):
    bad = _z(got) != _z(ref)
    if skip is not None:
        bad &= ~skip
    assert not bad.any(), "%s: %d elements differ, first %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _ratio(err, bound, skip=None):
    """largest |err| / bound outside `skip`; the error there is finite and no ratio is NaN"""
    err, bound = np.broadcast_arrays(np.asarray(err, f64), np.asarray(bound, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    if skip is not None:
        r = np.where(skip, 0.0, r)
    assert not np.isnan(r).any()
    assert np.isfinite(err if skip is None else np.where(skip, 0.0, err)).all()
    if r.size and r.max() > 1:
        j = np.unravel_index(int(r.argmax()), r.shape)
        print("over the bound at %s: |err| %.6g, bound %.6g (%d elements over)" % (j, float(err[j]), float(bound[j]), int((r > 1).sum())))
    return float(r.max()) if r.size else 0.0


def _note(prefix, entry, row, ratio):
    print("%s %s %s ratio=%.3f" % (prefix, entry, row, ratio))
    assert ratio <= 1.0, (entry, row, ratio)


# ------------------------------------------------------------------------------------------------ device helpers
class Guard:
    """An output or scratch buffer carved out of a larger allocation: 0xFF-filled (NaN in every float type, 255 in
    bytes) between two sentinel bands."""

    def __init__(self, shape, dtype, device, init=None):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * item
        self.flat = torch.empty(2 * BAND + (self.nbytes + 15) // 16 * 16, dtype=torch.uint8, device=device)
        self.flat.fill_(0x5E)
        self.flat[BAND:BAND + self.nbytes].fill_(0xFF)
        self.t = self.flat[BAND:BAND + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))

    def ok(self):
        return bool((self.flat[:BAND] == 0x5E).all()) and bool((self.flat[BAND + self.nbytes:] == 0x5E).all())

    def untouched(self):
        return self.ok() and bool((self.flat[BAND:BAND + self.nbytes] == 0xFF).all())

    def raw(self):
        assert self.ok(), "written outside the buffer"
        t = self.t
        return (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).cpu().numpy()

    def np(self, finite=True):
        """the contents, every element written and finite; finite=False lets an infinity through, never a NaN"""
        a = self.raw()
        if a.dtype.kind == "f":
            assert not np.isnan(a).any(), "elements the kernel did not write"
            assert not finite or np.isfinite(a).all(), "an infinite element"
        return a


class Strided:
    """[P][ld] f32 with the live columns [off, off + width) NaN (an output) or data (an input) and every other column a
    sentinel that must come back bit for bit."""
    SENT = f32(-12345.5)

    def __init__(self, P, ld, off, width, device, data=None):
        self.P, self.ld, self.off, self.width = P, ld, off, width
        host = np.full((P, ld), self.SENT, f32)
        host[:, off:off + width] = np.nan if data is None else data
        self.host = host
        self.g = Guard((P, ld), torch.float32, device, host)

    def np(self):
        a = self.g.raw()
        live = np.zeros(self.ld, bool)
        live[self.off:self.off + self.width] = True
        assert np.array_equal(a[:, ~live].view(np.int32), self.host[:, ~live].view(np.int32)), "sentinel columns written"
        out = a[:, live]
        assert not np.isnan(out).any(), "elements the kernel did not write"
        return out


def _words(t):
    """(integer view, band word, NaN word) of a flat tensor: 32-bit words under f32 / f64, 16-bit under a storage type"""
    if t.dtype in (torch.float32, torch.float64):
        return t.view(torch.int32), SENT32, NAN32
    return t.view(torch.int16), SENT16, NAN16


def carve(shape, dtype, band, device, fill=None):
    """-> (guard, tensor): a tensor inside a larger flat allocation, `band` sentinel elements on each side, filled with
    the NaN words, or with `fill` (a float, or a tensor of the shape: a buffer the launch reads)."""
    numel = int(np.prod(shape))
    flat = torch.empty(2 * band + numel, dtype=dtype, device=device)
    iv, sent, nan = _words(flat)
    iv.fill_(sent)
    t = flat[band:band + numel]
    assert t.data_ptr() % 16 == 0
    if fill is None:
        _words(t)[0].fill_(nan)
    elif isinstance(fill, float):
        t.fill_(fill)
    else:
        t.view(shape).copy_(fill)
    return (flat, band), t.view(shape)


def bands_untouched(guard):
    flat, band = guard
    iv, sent, _ = _words(flat)
    band *= iv.numel() // flat.numel()
    return bool((iv[:band] == sent).all()) and bool((iv[-band:] == sent).all())


def untouched(t):
    """every word of a carved tensor is still the NaN word"""
    iv, _, nan = _words(t.reshape(-1))
    return bool((iv == nan).all())


def written(t):
    return not bool(torch.isnan(t.reshape(-1).float()).any())


def _dev(a, device, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dtype or O.STORAGE).to(device)


def _d32(a, device):
    return _dev(a, device, torch.float32)


def _a(L, v):
    if isinstance(v, Strided):
        v = v.g
    if isinstance(v, Guard):
        return L.ptr(v.t)
    if v is None or isinstance(v, torch.Tensor):
        return L.ptr(v)
    if isinstance(v, (int, np.integer)):
        return ctypes.c_int(int(v))
    return v


def _raw(L, name, *args):
    """the status of a C-ABI call, not raised"""
    return int(L._fn(name, ctypes.c_int)(*args))


def _rc(L, name, *args):
    """the same with tensors, guards and ints converted and the stream appended"""
    return _raw(L, name, *[_a(L, v) for v in args], L.stream_ptr())


def _p(v):
    if isinstance(v, Strided):
        v = v.g
    if isinstance(v, Guard):
        v = v.t
    return None if v is None else v.data_ptr()


def _items(cls, rows):
    return (cls * max(len(rows), 1))(*[cls(*[_p(v) if not isinstance(v, (int, np.integer)) else int(v) for v in r]) for r in rows])


def _lib():
    from tensorflow_ocr_amd import _lib as L
    from tensorflow_ocr_amd import ops
    return L, ops
