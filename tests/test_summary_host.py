"""Host side of the training summaries (tensorflow_ocr_amd/summary.py, include/ocr_hip.h): no GPU needed.

The header's declarations, TensorFlow's default bucket limits, the histogram's run-length rule, the event file's framing
(both CRCs), the PNG encoder, an independent protobuf decoder where google.protobuf is installed, and the scripts' flags."""
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ocr_hip.h")


def _record(counts=None, **kw):
    from tensorflow_ocr_amd import summary
    r = {"num": 0, "nonfinite": 0, "min": 0.0, "max": 0.0, "sum": 0.0, "sum_squares": 0.0,
         "bucket": np.zeros(summary.NUM_BUCKETS, np.uint32)}
    for i, c in (counts or {}).items():
        r["bucket"][i] = c
    r["num"] = int(r["bucket"].sum())
    r.update(kw)
    return r


# ------------------------------------------------------------------------------------------------ header
def test_header_declares_the_summary_entry_points_and_keeps_abi_7():
    text = open(HEADER).read()
    assert re.search(r"#define\s+OCR_ABI_VERSION\s+7\b", text)
    for name in ("ocr_tensor_stats_f32", "ocr_tensor_stats_workspace", "ocr_tensor_stats_record_bytes",
                 "ocr_tensor_stats_num_buckets", "ocr_tensor_stats_table", "ocr_tensor_stats_table_bytes",
                 "ocr_tensor_stats_limits", "ocr_summary_image_u8", "ocr_summary_image_workspace"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    sig = re.search(r"int\s+ocr_tensor_stats_f32\s*\(([^;]*)\)\s*;", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in sig.replace("\n", " ").split(",")] == [
        "x", "segments_dev", "n_segments", "mul_host", "mul_dev", "records", "workspace", "ws_bytes", "stream"]
    assert re.search(r"#define\s+OCR_TENSOR_STATS_BUCKETS\s+1551\b", text)
    assert "ocr_tensor_stats_record" in text
    from tensorflow_ocr_amd import _lib, summary
    assert _lib.ABI_VERSION == 7
    assert summary.RECORD_DTYPE.itemsize == 32 + 4 * 1551 + 4 and summary.RECORD_DTYPE.fields["bucket"][1] == 32


def test_library_agrees_with_the_host_layer():
    """Host-only entry points of the built library (no device is touched)."""
    from tensorflow_ocr_amd import _lib, ops, summary
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libocr_hip.so is not built")
    assert ops.tensor_stats_num_buckets() == summary.NUM_BUCKETS == 1551
    assert ops.tensor_stats_record_bytes() == summary.RECORD_DTYPE.itemsize
    lim = ops.tensor_stats_limits()
    assert lim.tobytes() == summary.bucket_limits().tobytes()
    chunk = ops.tensor_stats_chunk()
    table, n_chunks = ops.tensor_stats_table([0, 4, 8, 12 + chunk], [1, 3, chunk + 1, 2 * chunk])
    assert n_chunks == 1 + 1 + 2 + 2 and ops.tensor_stats_workspace(n_chunks) == 32 * n_chunks
    head = table[:16].view(np.int32)
    assert head[0] == 4 and head[1] == n_chunks and head[2] == chunk
    assert table[16:16 + 8 * 775].view(np.float64).tobytes() == lim[776:].tobytes()
    segs = table[16 + 8 * 775:].view(np.int64).reshape(4, 3)
    assert segs[:, 0].tolist() == [0, 4, 8, 12 + chunk] and segs[:, 1].tolist() == [1, 3, chunk + 1, 2 * chunk]
    assert segs[:, 2].copy().view(np.int32).reshape(4, 2).tolist() == [[0, 1], [1, 1], [2, 2], [4, 2]]
    for bad in (([0], [0]), ([-1], [4]), ([0], [1 << 32])):
        with pytest.raises(_lib.OcrHipError):
            ops.tensor_stats_table(*bad)


# ------------------------------------------------------------------------------------------------ limits
def test_bucket_limits_obey_tensorflows_recurrence():
    from tensorflow_ocr_amd import summary
    lim = summary.bucket_limits()
    assert lim.dtype == np.float64 and lim.size == 1551 and (np.diff(lim) > 0).all()
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[-1] == np.finfo(np.float64).max
    pos = lim[776:]
    assert pos.size == 775
    v = 1e-12
    for k in range(774):
        assert pos[k] == v and v < 1e20
        v *= 1.1
    assert v >= 1e20                                           # the loop ends exactly there
    assert np.array_equal(lim[:775], -pos[::-1])
    # where the limits put a few values (upper_bound = searchsorted side='right')
    at = lambda x: int(np.searchsorted(lim, np.float64(x), side="right"))
    assert at(0.0) == at(-0.0) == at(1e-13) == 776 and at(1e-12) == 777 and at(-1e-13) == 775 and at(-1e-12) == 775
    assert at(np.float32(3.4028235e38)) == 1550 and at(-np.float32(3.4028235e38)) == 1


# ------------------------------------------------------------------------------------------------ run-length rule
def test_histogram_proto_collapses_empty_runs_to_their_last_limit():
    from tensorflow_ocr_amd import summary
    lim = summary.bucket_limits()
    h = summary.histogram_proto(_record({10: 2, 11: 1, 700: 5, 776: 7}, min=-3.0, max=0.0, sum=-9.0, sum_squares=27.0))
    # leading run 0..9 -> limit[9]; 10, 11 on their own; run 12..699 -> limit[699]; 700; run 701..775 -> limit[775];
    # 776; trailing run 777..1550 -> limit[1550] = DBL_MAX
    assert h["bucket_limit"] == [lim[9], lim[10], lim[11], lim[699], lim[700], lim[775], lim[776], lim[1550]]
    assert h["bucket"] == [0.0, 2.0, 1.0, 0.0, 5.0, 0.0, 7.0, 0.0]
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-3.0, 0.0, 15.0, -9.0, 27.0)


def test_histogram_proto_edges():
    from tensorflow_ocr_amd import summary
    lim = summary.bucket_limits()
    h = summary.histogram_proto(_record({0: 1, 1550: 2}))                  # no leading, no trailing run
    assert h["bucket_limit"] == [lim[0], lim[1549], lim[1550]] and h["bucket"] == [1.0, 0.0, 2.0]
    h = summary.histogram_proto(_record({1: 4}))                           # runs of one bucket
    assert h["bucket_limit"] == [lim[0], lim[1], lim[1550]] and h["bucket"] == [0.0, 4.0, 0.0]
    h = summary.histogram_proto(_record())                                 # all empty: one entry, the last limit
    assert h["bucket_limit"] == [lim[1550]] and h["bucket"] == [0.0] and h["num"] == 0.0
    h = summary.histogram_proto(_record({i: 1 for i in range(1551)}))      # nothing to collapse
    assert h["bucket_limit"] == lim.tolist() and h["bucket"] == [1.0] * 1551
    with pytest.raises(ValueError):
        summary.histogram_proto({**_record(), "bucket": np.zeros(5, np.uint32)})


# ------------------------------------------------------------------------------------------------ event file
def _write_sample(logdir):
    from tensorflow_ocr_amd import summary
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, size=(5, 7, 3)).astype(np.uint8)
    grey = rng.integers(0, 256, size=(4, 3, 1)).astype(np.uint8)
    rec = _record({3: 1, 776: 9, 800: 2}, min=-1e19, max=1.5e-10, sum=-1e19, sum_squares=1e38)
    with summary.FileWriter(logdir, wall_time=1234567890.25) as w:
        w.add_scalar("model_loss", 0.5)
        w.add_scalar("learning_rate", 1e-4)
        w.flush_step(1, wall_time=1234567891.5)
        w.add_histogram("variables_and_gradients_conv1/weights", rec)
        w.add_image("input", rgb)
        w.add_image("score_map", grey)
        w.flush_step(2 ** 40 + 3, wall_time=1234567892.0)
    return w.path, rgb, grey, rec


def test_event_file_round_trip(tmp_path):
    from tensorflow_ocr_amd import summary
    path, rgb, grey, rec = _write_sample(str(tmp_path))
    assert re.fullmatch(r"events\.out\.tfevents\.1234567890\..+", os.path.basename(path))
    ev = summary.read_events(path)
    assert len(ev) == 3
    assert ev[0] == {"wall_time": 1234567890.25, "step": 0, "values": [], "file_version": "brain.Event:2"}
    assert ev[1]["step"] == 1 and ev[1]["wall_time"] == 1234567891.5 and "file_version" not in ev[1]
    assert ev[1]["values"] == [{"tag": "model_loss", "simple_value": 0.5},
                               {"tag": "learning_rate", "simple_value": float(np.float32(1e-4))}]
    assert ev[2]["step"] == 2 ** 40 + 3
    hv, iv, gv = ev[2]["values"]
    assert hv["tag"] == "variables_and_gradients_conv1/weights" and hv["histo"] == summary.histogram_proto(rec)
    assert iv["tag"] == "input" and (iv["image"]["height"], iv["image"]["width"], iv["image"]["colorspace"]) == (5, 7, 3)
    assert np.array_equal(summary.decode_png(iv["image"]["encoded_image_string"]), rgb)
    assert (gv["image"]["height"], gv["image"]["width"], gv["image"]["colorspace"]) == (4, 3, 1)
    assert np.array_equal(summary.decode_png(gv["image"]["encoded_image_string"]), grey)


def test_record_framing_is_tfrecord(tmp_path):
    """u64 length, masked crc32c of the length, payload, masked crc32c of the payload — checked by hand on the first record."""
    from tensorflow_ocr_amd import tf_bundle
    path = _write_sample(str(tmp_path))[0]
    data = open(path, "rb").read()
    n, = struct.unpack("<Q", data[:8])
    assert struct.unpack("<I", data[8:12])[0] == tf_bundle.mask_crc(tf_bundle.crc32c(data[:8]))
    payload = data[12:12 + n]
    assert struct.unpack("<I", data[12 + n:16 + n])[0] == tf_bundle.mask_crc(tf_bundle.crc32c(payload))
    assert payload == b"\x09" + struct.pack("<d", 1234567890.25) + b"\x1a\x0dbrain.Event:2"
    assert tf_bundle.crc32c(b"123456789") == 0xE3069283          # the CRC-32C check value


def test_a_corrupted_byte_is_detected(tmp_path):
    from tensorflow_ocr_amd import summary
    path = _write_sample(str(tmp_path))[0]
    data = bytearray(open(path, "rb").read())
    n0, = struct.unpack("<Q", data[:8])
    second = 16 + n0
    for at in (3, 9, 12 + 2, 12 + n0 + 1, second + 1, second + 12 + 5, len(data) - 1, len(data) - 30):
        bad = bytearray(data)
        bad[at] ^= 0x10
        p = os.path.join(str(tmp_path), "bad_%d" % at)
        open(p, "wb").write(bad)
        with pytest.raises(ValueError):
            summary.read_events(p)
    p = os.path.join(str(tmp_path), "short")
    open(p, "wb").write(data[:-3])
    with pytest.raises(ValueError):
        summary.read_events(p)


def test_png_inflates_back_to_the_same_pixels():
    """Decoded by hand with zlib only, not through summary.decode_png."""
    from tensorflow_ocr_amd import summary
    rng = np.random.default_rng(4)
    for shape, ctype in (((6, 5, 3), 2), ((3, 9, 1), 0), ((2, 2, 4), 6), ((7, 4), 0)):
        px = rng.integers(0, 256, size=shape).astype(np.uint8)
        png = summary.encode_png(px)
        assert png[:8] == b"\x89PNG\r\n\x1a\n"
        pos, chunks = 8, []
        while pos < len(png):
            n, = struct.unpack(">I", png[pos:pos + 4])
            kind, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
            assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
            chunks.append((kind, body))
            pos += 12 + n
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        h, w = shape[:2]
        c = shape[2] if len(shape) == 3 else 1
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (w, h, 8, ctype, 0, 0, 0)
        rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * c)
        assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, c), px.reshape(h, w, c))
        assert np.array_equal(summary.decode_png(png), px.reshape(h, w, c))


def test_event_file_decodes_with_google_protobuf(tmp_path):
    """An independent decoder: message types built here from descriptor_pb2 with the field numbers of TensorFlow's
    event.proto / summary.proto."""
    try:
        from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    except ImportError:
        pytest.skip("google.protobuf is not installed")
    from tensorflow_ocr_amd import summary
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="ocr_summary_test.proto", package="ocrtest", syntax="proto3")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, num, ftype, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=ftype, label=label)
            if tname:
                f.type_name = ".ocrtest." + tname
    OPT, REP = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg("HistogramProto", [("min", 1, F.TYPE_DOUBLE, OPT, None), ("max", 2, F.TYPE_DOUBLE, OPT, None),
                           ("num", 3, F.TYPE_DOUBLE, OPT, None), ("sum", 4, F.TYPE_DOUBLE, OPT, None),
                           ("sum_squares", 5, F.TYPE_DOUBLE, OPT, None), ("bucket_limit", 6, F.TYPE_DOUBLE, REP, None),
                           ("bucket", 7, F.TYPE_DOUBLE, REP, None)])
    msg("Image", [("height", 1, F.TYPE_INT32, OPT, None), ("width", 2, F.TYPE_INT32, OPT, None),
                  ("colorspace", 3, F.TYPE_INT32, OPT, None), ("encoded_image_string", 4, F.TYPE_BYTES, OPT, None)])
    msg("Value", [("tag", 1, F.TYPE_STRING, OPT, None), ("simple_value", 2, F.TYPE_FLOAT, OPT, None),
                  ("image", 4, F.TYPE_MESSAGE, OPT, "Image"), ("histo", 5, F.TYPE_MESSAGE, OPT, "HistogramProto")])
    msg("Summary", [("value", 1, F.TYPE_MESSAGE, REP, "Value")])
    msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, OPT, None), ("step", 2, F.TYPE_INT64, OPT, None),
                  ("file_version", 3, F.TYPE_STRING, OPT, None), ("summary", 5, F.TYPE_MESSAGE, OPT, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName("ocrtest.Event")
    if hasattr(message_factory, "GetMessageClass"):
        Event = message_factory.GetMessageClass(desc)
    else:
        Event = message_factory.MessageFactory(pool).GetPrototype(desc)
    path, rgb, grey, rec = _write_sample(str(tmp_path))
    events = []
    for payload in summary.read_records(path):
        e = Event()
        e.ParseFromString(payload)
        events.append(e)
    assert events[0].file_version == "brain.Event:2" and events[0].wall_time == 1234567890.25
    assert events[1].step == 1 and [(v.tag, v.simple_value) for v in events[1].summary.value] == [
        ("model_loss", 0.5), ("learning_rate", float(np.float32(1e-4)))]
    assert events[2].step == 2 ** 40 + 3
    hv, iv, gv = events[2].summary.value
    want = summary.histogram_proto(rec)
    assert (hv.histo.min, hv.histo.max, hv.histo.num, hv.histo.sum, hv.histo.sum_squares) == (
        want["min"], want["max"], want["num"], want["sum"], want["sum_squares"])
    assert list(hv.histo.bucket_limit) == want["bucket_limit"] and list(hv.histo.bucket) == want["bucket"]
    assert (iv.image.height, iv.image.width, iv.image.colorspace) == (5, 7, 3)
    assert np.array_equal(summary.decode_png(iv.image.encoded_image_string), rgb)
    assert gv.tag == "score_map" and np.array_equal(summary.decode_png(gv.image.encoded_image_string), grey)


# ------------------------------------------------------------------------------------------------ tags and flags
def test_variable_tags_follow_the_reference_pattern():
    from tensorflow_ocr_amd import summary
    t = summary.variable_tags("conv1/conv1_1/weights")
    assert t == {"grad_histogram": "variables_and_gradients_conv1/conv1_1/weights_summed_gradients",
                 "var_histogram": "variables_and_gradients_conv1/conv1_1/weights",
                 "ratio": "variables_and_gradients_conv1/conv1_1/weights_summed_gradients_mean/var_mean",
                 "var_mean": "variables_and_gradients_conv1/conv1_1/weights_mean",
                 "nonfinite": "conv1/conv1_1/weights/nonfinite"}


def test_cli_flags_parse():
    sys.path.insert(0, ROOT)
    import multigpu_train
    import train_pixellink
    f = multigpu_train.parse([])
    assert f.save_summary_steps == 20 and f.summary_variables is False             # the reference's default interval
    f = multigpu_train.parse(["--save_summary_steps", "0", "--summary_variables"])
    assert f.save_summary_steps == 0 and f.summary_variables is True
    f = train_pixellink.parse([])
    assert f.save_summary_steps == 0 and f.summary_variables is False              # off by default
    f = train_pixellink.parse(["--save_summary_steps", "50", "--summary_variables"])
    assert f.save_summary_steps == 50 and f.summary_variables is True


def test_summaries_off_creates_no_file(tmp_path, monkeypatch):
    """--save_summary_steps 0: the loop never builds a writer (the step functions are stand-ins: no device)."""
    sys.path.insert(0, ROOT)
    import multigpu_train
    from tensorflow_ocr_amd import summary
    made = []
    monkeypatch.setattr(summary, "TrainingSummaries", lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError))
    monkeypatch.setattr(multigpu_train, "_steps", lambda FLAGS, g, step, opt, K, nb, last, summaries, *a: made.append(summaries))

    class _Step:
        opt = object()

        def build(self, *batch):
            return self
    ck = os.path.join(str(tmp_path), "ckpt")
    os.makedirs(ck)
    FLAGS = multigpu_train.parse(["--save_summary_steps", "0", "--checkpoint_path", ck, "--max_steps", "1"])
    monkeypatch.setattr(multigpu_train, "_next_batch", lambda *a: [None])
    multigpu_train._train_loop(FLAGS, None, _Step(), None, None, 0, 1, None, 0.0)
    assert made == [None] and os.listdir(ck) == []
    # and a FileWriter, once made, does create its file at once (what "on" means)
    w = summary.FileWriter(ck)
    w.close()
    assert len(os.listdir(ck)) == 1 and os.listdir(ck)[0].startswith("events.out.tfevents.")
