"""Training summaries: what the reference writes with tf.summary while it trains (multigpu_train.py:49-65,105-106,
135-145,189-194: scalars, images, a FileWriter event file; train_pixellink.py:179-194: a histogram of every variable
and of every summed gradient, mean(var), mean(grad) / mean(var)).

`TensorStats` computes every per-variable record in one segmented device pass over a flat buffer
(ocr_tensor_stats_f32, csrc/summary.hip), from the gradients the step just taken left in `store.flat_grad`: no second
train step as in the reference, and nothing joins the recorded step plan.  `FileWriter` writes a TensorBoard event
file (TFRecord framing, hand-encoded protobuf, PNG through zlib) and `read_events` reads one back.

Parity with an event file written by TensorFlow is NOT pinned by any test: neither TensorFlow nor TensorBoard was
available where this was written.  The framing, the field numbers and the histogram's run-length rule follow
tensorflow/core/lib/io/record_writer.cc, core/util/event.proto, core/framework/summary.proto and
core/lib/histogram/histogram.cc.  Non-finite elements are counted (`nonfinite`) and left out of the histogram, where
TensorFlow's histogram op raises."""
import os
import socket
import struct
import time
import zlib

import numpy as np

from ._lib import TENSOR_STATS_BUCKETS, TensorStatsRecord
from .tf_bundle import _pb_bytes, _pb_fields, _pb_varint, _put_varint, crc32c, mask_crc

NUM_BUCKETS = TENSOR_STATS_BUCKETS
RECORD_DTYPE = np.dtype(TensorStatsRecord)
_LIMITS = None


def bucket_limits():
    """TensorFlow's default histogram limits (histogram.cc, InitDefaultBucketsInner), 1551 float64 in rising order:
    `v = 1e-12; while v < 1e20: push(v); v *= 1.1`, then DBL_MAX, mirrored negative, with 0 between the halves.
    Python floats are IEEE doubles: the same bits as the library's table (ocr_tensor_stats_limits)."""
    global _LIMITS
    if _LIMITS is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(float(np.finfo(np.float64).max))
        lim = np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)
        assert lim.size == NUM_BUCKETS
        lim.setflags(write=False)
        _LIMITS = lim
    return _LIMITS


# --------------------------------------------------------------------------- device pass
class TensorStats:
    """Per-variable records of a buffer laid out like `store.flat` (the weights, the gradients, an optimiser slot).

    The segment table is built from `store.trainable()` once and uploaded; `run(flat_like, mul_host, mul_dev)`
    enqueues the pass on the current stream (one memset, two launches, no sync) and `read()` copies the records back
    (a sync) as {variable name: record}, a record being a dict with num, nonfinite, min, max, sum, sum_squares and
    bucket (uint32 [1551]).  For gradients pass `TrainStep.summary_factor()`.  Call it outside the step."""

    def __init__(self, store):
        import torch
        from . import ops
        if store.flat is None:
            raise RuntimeError("the variable store is not materialised yet (build the step first)")
        self.store = store
        base = store.flat.data_ptr()
        self.names, offs, sizes = [], [], []
        for v in store.trainable():
            off = (v.data.data_ptr() - base) // 4
            if off < 0 or off + v.size > store.flat.numel():
                raise ValueError("variable %s does not lie in the flat buffer" % v.name)
            self.names.append(v.name)
            offs.append(off)
            sizes.append(v.size)
        if not self.names:
            raise ValueError("the store holds no trainable variable")
        table, self.n_chunks = ops.tensor_stats_table(offs, sizes)
        dev = store.flat.device
        self.table = torch.from_numpy(table.view(np.int64)).to(dev)                   # (int64: an 8-byte aligned allocation)
        self.records = torch.zeros(len(self.names) * RECORD_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        self.ws = torch.empty(max(1, ops.tensor_stats_workspace(self.n_chunks) // 8), dtype=torch.float64, device=dev)

    def run(self, flat_like, mul_host=1.0, mul_dev=None):
        from . import ops
        if flat_like.numel() != self.store.flat.numel() or flat_like.dtype != self.store.flat.dtype:
            raise ValueError("the buffer is not laid out like the store's flat buffer")
        ops.tensor_stats(flat_like, self.table, len(self.names), float(mul_host), mul_dev, self.records, self.ws)
        return self

    def read(self):
        raw = self.records.cpu().numpy().view(RECORD_DTYPE)
        return {n: record_dict(raw[i]) for i, n in enumerate(self.names)}


def record_dict(r):
    """One element of a RECORD_DTYPE array as a dict of Python numbers and the bucket array."""
    if int(r["nonfinite"]) == 0xFFFFFFFF and int(r["num"]) == 0:
        raise RuntimeError("ocr_tensor_stats_f32 refused its table or workspace on the device")
    return {"num": int(r["num"]), "nonfinite": int(r["nonfinite"]), "min": float(r["min"]), "max": float(r["max"]),
            "sum": float(r["sum"]), "sum_squares": float(r["sum_squares"]), "bucket": np.array(r["bucket"], dtype=np.uint32)}


class ImageSummary:
    """tf.summary.image's float -> u8 rule on the device (ocr_summary_image_u8): `u8(image)` takes one [h, w, c] f32
    device tensor and returns the numpy uint8 array (a sync)."""

    def __init__(self, device):
        import torch
        from . import ops
        self.ws = torch.empty(max(1, ops.summary_image_workspace() // 4), dtype=torch.float32, device=device)

    def u8(self, image):
        import torch
        from . import ops
        x = image.detach().to(torch.float32).contiguous()
        if x.dim() == 2:
            x = x[..., None]
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        ops.summary_image_u8(x, out, self.ws)
        return out.cpu().numpy()


# --------------------------------------------------------------------------- protobuf pieces
def _pb_double(fn, v):
    return _put_varint((fn << 3) | 1) + struct.pack("<d", v)


def _pb_float(fn, v):
    return _put_varint((fn << 3) | 5) + struct.pack("<f", v)


def _pb_packed_doubles(fn, values):
    return _pb_bytes(fn, np.asarray(values, dtype="<f8").tobytes())


def histogram_proto(record, limits=None):
    """HistogramProto fields of a record as a dict (min, max, num, sum, sum_squares, bucket_limit, bucket), the buckets
    run-length encoded as Histogram::EncodeToProto does: a run of empty buckets collapses into ONE entry that carries the
    last limit of the run (and count 0); a non-empty bucket is an entry of its own."""
    limits = bucket_limits() if limits is None else np.asarray(limits, dtype=np.float64)
    counts = np.asarray(record["bucket"])
    if counts.shape != limits.shape:
        raise ValueError("bucket and limits differ in length")
    lim_out, cnt_out = [], []
    i, n = 0, counts.size
    while i < n:
        end, count = float(limits[i]), float(counts[i])
        i += 1
        if count <= 0.0:
            while i < n and counts[i] <= 0:
                end, count = float(limits[i]), float(counts[i])
                i += 1
        lim_out.append(end)
        cnt_out.append(count)
    if not lim_out:
        lim_out, cnt_out = [float(np.finfo(np.float64).max)], [0.0]
    return {"min": float(record["min"]), "max": float(record["max"]), "num": float(record["num"]),
            "sum": float(record["sum"]), "sum_squares": float(record["sum_squares"]),
            "bucket_limit": lim_out, "bucket": cnt_out}


def _encode_histogram(h):
    return (_pb_double(1, h["min"]) + _pb_double(2, h["max"]) + _pb_double(3, h["num"]) + _pb_double(4, h["sum"]) +
            _pb_double(5, h["sum_squares"]) + _pb_packed_doubles(6, h["bucket_limit"]) + _pb_packed_doubles(7, h["bucket"]))


def encode_png(pixels):
    """uint8 [h, w] or [h, w, c] (c = 1 grey, 3 RGB, 4 RGBA) -> PNG bytes; zlib only, filter 0 on every row."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    ctype = {1: 0, 3: 2, 4: 6}[c]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * c)], axis=1).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def decode_png(data):
    """Inverse of `encode_png` for the PNGs it writes (8 bit, no interlace, filter 0): uint8 [h, w, c]."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError("PNG chunk %r fails its CRC" % kind)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = head
    c = {0: 1, 2: 3, 6: 4}[ctype]
    if depth != 8 or interlace:
        raise ValueError("unsupported PNG form")
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
    if rows[:, 0].any():
        raise ValueError("unsupported PNG row filter")
    return rows[:, 1:].reshape(h, w, c).copy()


def scalar_value(tag, value):
    return _pb_bytes(1, tag.encode()) + _pb_float(2, float(value))


def histogram_value(tag, record):
    return _pb_bytes(1, tag.encode()) + _pb_bytes(5, _encode_histogram(histogram_proto(record)))


def image_value(tag, pixels):
    a = np.asarray(pixels)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    img = _pb_varint(1, h) + _pb_varint(2, w) + _pb_varint(3, c) + _pb_bytes(4, encode_png(a))
    return _pb_bytes(1, tag.encode()) + _pb_bytes(4, img)


# --------------------------------------------------------------------------- event file
def _frame(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + payload + struct.pack("<I", mask_crc(crc32c(payload)))


class FileWriter:
    """tf.summary.FileWriter: `logdir`/events.out.tfevents.<time>.<host>, one TFRecord per Event; the first says
    file_version "brain.Event:2".  add_scalar / add_histogram / add_image collect Summary values, `flush_step(step)`
    writes them as ONE event (as a merged summary op does) and flushes the file."""

    def __init__(self, logdir, wall_time=None):
        os.makedirs(logdir, exist_ok=True)
        t = time.time() if wall_time is None else wall_time
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(t), socket.gethostname()))
        self._f = open(self.path, "ab")
        self._values = []
        self._f.write(_frame(_pb_double(1, t) + _pb_bytes(3, b"brain.Event:2")))
        self._f.flush()

    def add_scalar(self, tag, value):
        self._values.append(scalar_value(tag, value))

    def add_histogram(self, tag, record):
        self._values.append(histogram_value(tag, record))

    def add_image(self, tag, pixels):
        self._values.append(image_value(tag, pixels))

    def flush_step(self, step, wall_time=None):
        summary = b"".join(_pb_bytes(1, v) for v in self._values)
        self._values = []
        t = time.time() if wall_time is None else wall_time
        self._f.write(_frame(_pb_double(1, t) + _pb_varint(2, int(step)) + _pb_bytes(5, summary)))
        self._f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _f64(b):
    return struct.unpack("<d", bytes(b))[0]


def _decode_histogram(buf):
    h = {"bucket_limit": [], "bucket": []}
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for fn, wt, v in _pb_fields(buf):
        if fn in names and wt == 1:
            h[names[fn]] = _f64(v)
        elif fn in (6, 7):
            key = "bucket_limit" if fn == 6 else "bucket"
            h[key].extend(np.frombuffer(bytes(v), "<f8").tolist() if wt == 2 else [_f64(v)])
    return h


def _decode_value(buf):
    out = {}
    for fn, wt, v in _pb_fields(buf):
        if fn == 1:
            out["tag"] = bytes(v).decode()
        elif fn == 2 and wt == 5:
            out["simple_value"] = struct.unpack("<f", bytes(v))[0]
        elif fn == 4:
            img = {}
            for f2, _, v2 in _pb_fields(v):
                if f2 in (1, 2, 3):
                    img[{1: "height", 2: "width", 3: "colorspace"}[f2]] = int(v2)
                elif f2 == 4:
                    img["encoded_image_string"] = bytes(v2)
            out["image"] = img
        elif fn == 5:
            out["histo"] = _decode_histogram(v)
    return out


def read_records(path):
    """The payloads of a TFRecord file; ValueError when a length or a payload fails its masked CRC-32C or the file ends
    inside a record."""
    with open(path, "rb") as f:
        data = f.read()
    pos, out = 0, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("%s: truncated record header at byte %d" % (path, pos))
        head = data[pos:pos + 8]
        n, = struct.unpack("<Q", head)
        if struct.unpack("<I", data[pos + 8:pos + 12])[0] != mask_crc(crc32c(head)):
            raise ValueError("%s: the length at byte %d fails its CRC" % (path, pos))
        if pos + 12 + n + 4 > len(data):
            raise ValueError("%s: truncated record at byte %d" % (path, pos))
        payload = data[pos + 12:pos + 12 + n]
        if struct.unpack("<I", data[pos + 12 + n:pos + 16 + n])[0] != mask_crc(crc32c(payload)):
            raise ValueError("%s: the record at byte %d fails its CRC" % (path, pos))
        out.append(payload)
        pos += 16 + n
    return out


def read_events(path):
    """Inverse of FileWriter: a list of {"wall_time", "step", "file_version"?, "values": [{"tag", "simple_value" |
    "histo" | "image"}]}; both CRCs of every record are checked."""
    events = []
    for payload in read_records(path):
        ev = {"wall_time": 0.0, "step": 0, "values": []}
        for fn, wt, v in _pb_fields(payload):
            if fn == 1 and wt == 1:
                ev["wall_time"] = _f64(v)
            elif fn == 2 and wt == 0:
                ev["step"] = int(v)
            elif fn == 3:
                ev["file_version"] = bytes(v).decode()
            elif fn == 5:
                ev["values"] = [_decode_value(v2) for f2, _, v2 in _pb_fields(v) if f2 == 1]
        events.append(ev)
    return events


# --------------------------------------------------------------------------- the training scripts' writer
def variable_tags(name):
    """The four tags train_pixellink.py:190-193 writes for a variable `name` (an op name: no ':0'), and ours for the
    count of non-finite gradient elements."""
    g = name + "_summed_gradients"
    p = "variables_and_gradients_"
    return {"grad_histogram": p + g, "var_histogram": p + name, "ratio": p + g + "_mean/var_mean",
            "var_mean": p + name + "_mean", "nonfinite": name + "/nonfinite"}


class TrainingSummaries:
    """What the training scripts write every `--save_summary_steps` optimiser steps (rank 0): scalars, the images of
    the batch's first sample and, with `variables=True`, the four per-variable summaries of the reference
    (`variable_tags`) plus `<name>/nonfinite`.  Everything the device computes is enqueued behind the step; the reads
    happen here, on summary steps only."""

    def __init__(self, logdir, step, variables=False):
        self.writer = FileWriter(logdir)
        self.step = step
        # one object per buffer: both passes are enqueued before the first read
        self.var_stats = TensorStats(step.g.store) if variables else None
        self.grad_stats = TensorStats(step.g.store) if variables else None
        self.images = ImageSummary(step.g.store.flat.device)

    def write(self, global_step, scalars, images=()):
        """scalars: {tag: number}; images: (tag, [h, w, c] device tensor) pairs.  Call it behind a call of the step
        that closed its window (the gradients of that optimiser step are then in store.flat_grad)."""
        w = self.writer
        st = self.step.g.store
        if self.var_stats is not None:
            self.var_stats.run(st.flat)
            self.grad_stats.run(st.flat_grad, *self.step.summary_factor())
            varis, grads = self.var_stats.read(), self.grad_stats.read()
        for tag, v in scalars.items():
            w.add_scalar(tag, v)
        for tag, im in images:
            w.add_image(tag, self.images.u8(im))
        if self.var_stats is not None:
            for name in self.var_stats.names:
                t, rv, rg = variable_tags(name.replace(":0", "")), varis[name], grads[name]
                w.add_histogram(t["grad_histogram"], rg)
                w.add_histogram(t["var_histogram"], rv)
                var_mean = rv["sum"] / rv["num"] if rv["num"] else float("nan")
                grad_mean = rg["sum"] / rg["num"] if rg["num"] else float("nan")
                w.add_scalar(t["ratio"], grad_mean / var_mean if var_mean else float("nan"))
                w.add_scalar(t["var_mean"], var_mean)
                w.add_scalar(t["nonfinite"], rg["nonfinite"])
        w.flush_step(global_step)

    def close(self):
        self.writer.close()
