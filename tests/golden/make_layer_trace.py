"""Records tests/golden/layer_trace.json: what the Python layer modules (tensorflow_ocr_amd/layers.py, resnet_layers.py,
head_layers.py) LAUNCH for a table of small builds — the flat list of C-ABI calls of one eager step under `_lib.Recorder`, made
independent of addresses — and, for the training builds, the bits of two training steps.  tests/test_gpu_layer_trace.py
re-records every build and requires the same list and the same bits: run this on the commit whose launches are to be
kept, BEFORE changing the host code above the C ABI.  Needs the GPU.

    python tests/golden/make_layer_trace.py [out.json] [--text DIR]

The file keeps a digest of every list (`digest` below), not its text — 5000 entries of a hundred characters each are
no reading matter; `--text DIR` writes the lists themselves, to be compared between two commits with `diff`.

One entry of the list is `name|tag|arguments`:
  * integers and floats by value, a ConvDesc (or another by-reference struct) by its fields, an array of item structs
    by the fields of every item;
  * a pointer as `p<k>+<offset>`: the step's tensors are all alive while it is recorded (graph.keepalive), so an
    address names one tensor; k numbers the allocations in the order in which the trace first passes a pointer into
    them (that is: it names the first entry argument that points into the same allocation), the offset is in bytes;
  * the stream (the last argument of every entry) dropped.
Host callbacks stay as `py:<label>` position markers.

Every build runs in a child interpreter of its own (the layer switches are read at import).  A training build's child
takes two eager steps (loss bits, CRC-32 of the parameters after the second) and records the third; this script runs
it twice and keeps the bits only where the two runs agree.  The shape is the smallest of CANDIDATES at which the default
model_vgg trace names every entry point of profiles/r06_step_calls.json (the headline step at 32 x 512^2)."""
import bisect
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "layer_trace.json")
MARK = "LAYER_TRACE_JSON "
CHILD_TIMEOUT = 240          # seconds, per build

CANDIDATES = [(2, 64), (2, 128), (2, 256)]          # (batch, image size)
SWITCHES = ["OCR_GUEST_BN", "OCR_FUSE_BN", "OCR_BATCH_HEADS", "OCR_FIRST_DROP_Y", "OCR_RESNET_FUSE_TAIL",
            "OCR_RESNET_FUSE_BWD", "OCR_RESNET_S2D"]
# name -> (net, mode, environment); mode: "train" | "infer" (is_training=False forward) | "f32" (precision="f32" forward)
BUILDS = {"vgg": ("vgg", "train", {}), "pixellink": ("pixellink", "train", {}), "resnet": ("resnet", "train", {}),
          "vgg_infer": ("vgg", "infer", {}), "pixellink_infer": ("pixellink", "infer", {}),
          "resnet_infer": ("resnet", "infer", {}), "vgg_f32": ("vgg", "f32", {})}
for _net in ("vgg", "resnet"):
    for _sw in SWITCHES:
        BUILDS["%s,%s=0" % (_net, _sw)] = (_net, "train", {_sw: "0"})
# head paths that the table above does not reach: the per-source bias forms, the two single sigmoid heads, the merge
# convolution on the upsampled tensor, and the RBOX heads' forward (their backward: tests/test_gpu_rbox.py)
MERGE_SWITCHES = ["OCR_RESNET_MERGE_HEADS", "OCR_RESNET_MERGE_REORDER"]
BUILDS["pixellink,OCR_BATCH_HEADS=0"] = ("pixellink", "train", {"OCR_BATCH_HEADS": "0"})
for _sw in MERGE_SWITCHES:
    BUILDS["resnet,%s=0" % _sw] = ("resnet", "train", {_sw: "0"})
BUILDS["rbox"] = ("rbox", "infer", {})


# ------------------------------------------------------------------------------------------------ canonical form
def _blocks():
    """Sorted (address, size) of every block of torch's caching allocator."""
    import torch
    out = []
    for seg in torch.cuda.memory_snapshot():
        a = seg["address"]
        for b in seg["blocks"]:
            a = b.get("address", a)
            out.append((a, b["size"]))
            a += b["size"]
    out.sort()
    return out


class _Pointers:
    def __init__(self):
        self.blocks = _blocks()
        self.starts = [b[0] for b in self.blocks]
        self.ids = {}

    def name(self, v):
        if not v:
            return "null"
        i = bisect.bisect_right(self.starts, v) - 1
        base = v
        if i >= 0 and v < self.blocks[i][0] + self.blocks[i][1]:
            base = self.blocks[i][0]
        k = self.ids.setdefault(base, len(self.ids))
        return "p%d+%d" % (k, v - base)


def _num(v):
    return repr(float(v)) if isinstance(v, float) else str(int(v))


def _struct(s, ptrs):
    out = []
    for f in s._fields_:
        v = getattr(s, f[0])
        out.append(ptrs.name(v) if f[1] is ctypes.c_void_p else _num(v))
    return "{" + ",".join(out) + "}"


def _arg(a, ptrs):
    if isinstance(a, ctypes.c_void_p):
        return ptrs.name(a.value)
    if isinstance(a, ctypes.Array):
        return "[" + ",".join(_struct(s, ptrs) for s in a) + "]"
    if isinstance(a, ctypes.Structure):
        return _struct(a, ptrs)
    obj = getattr(a, "_obj", None)            # byref(struct)
    if isinstance(obj, ctypes.Structure):
        return _struct(obj, ptrs)
    if hasattr(a, "value"):
        return _num(a.value)
    raise TypeError("unexpected argument %r" % (a,))


def canonical(entries):
    """The recorded entries (`_lib.Recorder.entries`) as a list of strings; call it while the step's tensors are alive."""
    from tensorflow_ocr_amd import _lib
    stream = _lib.stream_ptr().value
    ptrs = _Pointers()
    out = []
    for e in entries:
        if e[0] != "c":
            out.append("py:" + (e[2] if len(e) > 2 and isinstance(e[2], str) else "hook"))
            continue
        args = e[2]
        if isinstance(args[-1], ctypes.c_void_p) and args[-1].value == stream:
            args = args[:-1]                   # (the stream)
        tag = "" if e[4] is None else ",".join(_num(t) if isinstance(t, (int, float)) else str(t) for t in e[4])
        out.append("%s|%s|%s" % (e[3], tag, " ".join(_arg(a, ptrs) for a in args)))
    return out


# ------------------------------------------------------------------------------------------------ one build (child)
def _forward_loss(net, M):
    if net == "vgg":
        def fl(gr, im, px, lk, mk):
            a, b = M.model_vgg(im, is_training=True, graph=gr)
            return M.loss(px, a, lk, b, mk, graph=gr)
    elif net == "resnet":
        def fl(gr, im, px, lk, mk):
            a, b = M.model(im, is_training=True, graph=gr)
            return M.loss(px, a, lk, b, mk, graph=gr)
    else:
        from tensorflow_ocr_amd.nets import pixellink

        def fl(gr, im, px, lk, mk):
            return pixellink.PixelLinkNet(im, graph=gr).build_loss(px[..., 0], lk)
    return fl


def child(name, batch, size):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tensorflow_ocr_amd import _lib, synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, MomentumOptimizer, TrainStep
    net, mode, _ = BUILDS[name]
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    data = [torch.from_numpy(a).to(device) for a in synthetic.make_batch(np.random.default_rng(100), batch, size)]
    if net == "pixellink":
        data = [(data[0] - 120.0) / 60.0] + data[1:]
    out = {"name": name, "storage": _lib.STORAGE, "csrc": _lib.csrc_fingerprint()}
    if mode == "train":
        g = Graph(device, loss_scale=1024.0, seed=1)
        opt = (lambda gr: MomentumOptimizer(gr)) if net == "pixellink" else (lambda gr: AdamOptimizer(gr, learning_rate=1e-4))
        step = TrainStep(g, _forward_loss(net, M), opt, world_size=1)
        losses = [float(step(*data).item()) for _ in range(2)]
        torch.cuda.synchronize()
        out["loss"] = [np.float32(v).tobytes().hex() for v in losses]
        out["flat_crc32"] = "%08x" % zlib.crc32(g.store.flat.detach().cpu().numpy().tobytes())
        t0 = time.perf_counter()
        step(*data)
        torch.cuda.synchronize()
        out["record_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert step.plan is not None, "the third step was not recorded"
        out["trace"] = canonical(step.recorded)
    else:
        g = Graph(device, seed=1, **({"precision": "f32"} if mode == "f32" else {}))

        def forward():
            g.reset_tape()
            if net == "vgg":
                M.model_vgg(data[0], is_training=False, graph=g)
            elif net == "resnet":
                M.model(data[0], is_training=False, graph=g)
            elif net == "rbox":
                M.model_rbox(data[0], is_training=False, graph=g)
            else:
                # (PixelLinkNet has no is_training argument — its layers have no batch norm: the forward alone)
                from tensorflow_ocr_amd.nets import pixellink
                pixellink.PixelLinkNet(data[0], graph=g)
        forward()                               # creates the variables and the operand packs
        torch.cuda.synchronize()
        rec = _lib.Recorder()
        g.keepalive = []
        _lib.RECORDER = rec
        try:
            forward()
        finally:
            _lib.RECORDER = None
        torch.cuda.synchronize()
        out["trace"] = canonical(rec.entries)
    print(MARK + json.dumps(out), flush=True)


def run_build(name, batch, size, storage="f16"):
    """One build in a fresh interpreter -> the child's dict."""
    env = dict(os.environ, OCR_STORAGE=storage)
    for sw in SWITCHES + MERGE_SWITCHES:
        env.pop(sw, None)
    env.update(BUILDS[name][2])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(batch), str(size)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(MARK)]
    if r.returncode != 0 or not lines:
        raise RuntimeError("build %s failed (exit %d):\n%s" % (name, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads(lines[-1][len(MARK):])


# ------------------------------------------------------------------------------------------------ the recording
def profile_entry_points():
    with open(os.path.join(ROOT, "profiles", "r06_step_calls.json")) as f:
        prof = json.load(f)
    assert prof["which"] == "vgg"
    return sorted({r["call"] for r in prof["timeline"] if not r["call"].startswith("py:")})


def digest(trace):
    """What the golden keeps of one trace: a SHA-256 over the whole list (equal digest = equal list) and, so that a
    mismatch names its first entry, one CRC-32 per entry (8 hex digits each, 32 entries per line)."""
    crcs = "".join("%08x" % zlib.crc32(t.encode()) for t in trace)
    return {"sha256": hashlib.sha256("\n".join(trace).encode()).hexdigest(),
            "entries": [crcs[i:i + 256] for i in range(0, len(crcs), 256)]}


def write_golden(path, shape, csrc, builds):
    """builds: name -> {"trace": [...], "numbers": {...} | None (training builds only)}"""
    rows = []
    for name, row in builds.items():
        d = digest(row["trace"])
        head = '  %s: {' % json.dumps(name)
        if "numbers" in row:
            head += '"numbers": %s, ' % json.dumps(row["numbers"])
        rows.append(head + '"sha256": "%s", "entries": [\n   %s]}' % (d["sha256"], ",\n   ".join(json.dumps(e) for e in d["entries"])))
    with open(path, "w") as f:
        f.write('{"batch": %d, "size": %d, "storage": "f16", "csrc": "%s",\n "builds": {\n' % (shape + (csrc,)))
        f.write(",\n".join(rows) + "\n }}\n")


def main():
    """[out.json] [--text DIR]: DIR receives every build's list as text, one entry per line — what to `diff` between two
    commits when the test names an entry that changed."""
    argv = sys.argv[1:]
    text_dir = None
    if "--text" in argv:
        i = argv.index("--text")
        text_dir = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(text_dir, exist_ok=True)
    want = profile_entry_points()
    shape = first = None
    for batch, size in CANDIDATES:
        first = run_build("vgg", batch, size)
        missing = [c for c in want if c not in {t.split("|")[0] for t in first["trace"]}]
        print("vgg at %d x %d^2: %d entries, entry points of the profile not reached: %s" % (
            batch, size, len(first["trace"]), missing or "none"), flush=True)
        if not missing:
            shape = (batch, size)
            break
    assert shape is not None, "no candidate shape reaches every entry point of profiles/r06_step_calls.json"
    builds = {}
    for name, (net, mode, _) in BUILDS.items():
        a = first if name == "vgg" else run_build(name, *shape)
        row = {"trace": a["trace"]}
        if mode == "train":
            b = run_build(name, *shape)
            assert b["trace"] == a["trace"], "the trace of %s does not reproduce itself" % name
            same = a["loss"] == b["loss"] and a["flat_crc32"] == b["flat_crc32"]
            row["numbers"] = {"loss": a["loss"], "flat_crc32": a["flat_crc32"]} if same else None
            print("%-32s %4d entries, record step %.1f / %.1f ms, numbers %s" % (
                name, len(a["trace"]), a["record_ms"], b["record_ms"],
                "reproduce" if same else "DO NOT reproduce: %s %s | %s %s" % (a["loss"], a["flat_crc32"], b["loss"], b["flat_crc32"])),
                flush=True)
        else:
            print("%-32s %4d entries" % (name, len(a["trace"])), flush=True)
        builds[name] = row
        if text_dir is not None:
            with open(os.path.join(text_dir, name + ".txt"), "w") as f:
                f.write("\n".join(a["trace"]) + "\n")
    path = argv[0] if argv else GOLDEN
    write_golden(path, shape, first["csrc"], builds)
    print("%d builds -> %s (%d bytes)" % (len(builds), path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
