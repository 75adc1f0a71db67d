"""What the evaluation-chain files (test_gpu_eval_chain.py, test_gpu_link_eval_chain.py, test_gpu_eval_ic15.py,
test_gpu_eval_sweep.py, test_gpu_map_fuse.py) share: a plain module, no fixtures and no hooks.  The ground-truth writer,
the spies of a pass (every device read; every chain's `last`), the two synthetic evaluation directories with the stub
forwards that go with them (a file wraps a builder in a fixture of its own), and the body of the training runs with an
evaluation between the steps.  What a test asserts stays in its file."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32


def rect(x0, y0, x1, y1):
    """axis-aligned quad"""
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def write_gt(path, quads, tags):
    with open(path, "w") as f:
        for q, t in zip(quads, tags):
            f.write(",".join(str(int(v)) for v in np.asarray(q).reshape(-1)) + "," + t + "\r\n")


def write_training_eval_dir(d):
    """the directory the training tests evaluate on: two random 64 x 64 images, a word and an ignored one each"""
    rng = np.random.default_rng(5)
    for name in ("img_1", "img_2"):
        np.save(os.path.join(d, name + ".npy"), rng.integers(0, 256, (64, 64, 3)).astype(np.uint8))
        write_gt(os.path.join(d, "gt_%s.txt" % name), [rect(8, 8, 40, 24), rect(30, 40, 60, 56)], ["text", "###"])


# ------------------------------------------------------------------------------------------------ spies
def spy_reads(monkeypatch, calls):
    """every read of the device from here on (undo with monkeypatch.undo()), each with the number of forwards launched
    before it -> the list they are appended to"""
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                reads.append((_name, len(calls)))
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, spy)
    return reads


def keep_lasts(ev):
    """every chain's `last` of the passes that follow (device tensors, no read) -> the list they are appended to"""
    chains, match = [], ev._match

    def keeping(*a, **kw):
        out = match(*a, **kw)
        chains.append(dict(ev.last))
        return out
    ev._match = keeping
    return chains


# ------------------------------------------------------------------------------------------------ the RBOX directory
def rbox_eval_dir(graph, d):
    """3 images (two 64 x 64, one 96 wide x 64 high) with label maps from synthetic.rbox_labels and ground truths made from
    what the detector finds on them: the best detection exactly, an ignored quad, and one nothing matches."""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.tool import rbox
    rng = np.random.default_rng(77)
    s64, g64, _ = synthetic.rbox_labels(2, 64, rng, rects=2)
    s96, g96, _ = synthetic.rbox_labels(1, 96, rng, rects=3)
    maps = {"img_a": (s64[0], g64[0]), "img_b": (s64[1], g64[1]), "img_c": (s96[0, :16], g96[0, :16])}      # [16,24] for 64 x 96
    shapes = {"img_a": (64, 64), "img_b": (64, 64), "img_c": (64, 96)}
    for name, (h, w) in shapes.items():
        np.save(os.path.join(d, name + ".npy"), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        quads = rbox.detect(maps[name][0][None], maps[name][1][None], graph=graph)[0]
        assert len(quads) >= 1, name
        best = quads[np.argsort(-quads[:, 8], kind="stable")[0], :8].astype(i32)
        write_gt(os.path.join(d, "gt_%s.txt" % name), [best, rect(1, 1, 9, 6), rect(50, 2, 62, 9)], ["text", "###", "far"])
    return d, maps, shapes


def rbox_stub_forward(device, maps):
    """the maps of the images a batch holds, by its shape: (2, 64, 64) = img_a, img_b in name order; (1, 64, 96) = img_c"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    calls = []

    def forward(x):
        calls.append(tuple(x.shape))
        names = {(2, 64, 64, 3): ["img_a", "img_b"], (1, 64, 96, 3): ["img_c"]}[tuple(x.shape)]
        return up(np.stack([maps[k][0] for k in names])), up(np.stack([maps[k][1] for k in names]))
    return forward, calls


# ------------------------------------------------------------------------------------------------ the link directory
EVAL = 128                                       # the eval size of the link tests: maps of 32 x 32
SHAPES = {"img_a": (96, 128), "img_b": (96, 128), "img_c": (96, 160)}      # (h, w) of the originals
REGIONS = {"img_a": [(9, 8, 6, 2, 0), (20, 22, 8, 2, 35)],                 # per image: (cx, cy, a, b, deg) of `rot`
           "img_b": [(16, 10, 9, 3, -20), (8, 25, 5, 2, 0), (25, 25, 3, 3, 0)],
           "img_c": [(16, 16, 10, 3, 60), (5, 5, 3, 2, 0)]}


def rot(h, w, cx, cy, a, b, deg):
    ys, xs = np.mgrid[0:h, 0:w]
    th = np.deg2rad(deg)
    u = (xs - cx) * np.cos(th) + (ys - cy) * np.sin(th)
    v = -(xs - cx) * np.sin(th) + (ys - cy) * np.cos(th)
    return (np.abs(u) <= a) & (np.abs(v) <= b)


def link_logits(rng, regions, text=(2.0, 4.5)):
    """(pixel_cls [32,32,2], link_cls [32,32,16]) whose softmaxes paint the regions: the text logit uniform in `text` inside
    (P(text) in (0.88, 0.99) for the default), P(text) below 0.12 outside; every link 0.993"""
    inside = np.zeros((32, 32), bool)
    for m in regions:
        inside |= m
    px = np.zeros((32, 32, 2), f32)
    px[..., 1] = np.where(inside, rng.uniform(text[0], text[1], (32, 32)), rng.uniform(-4.5, -2.0, (32, 32)))
    lk = np.zeros((32, 32, 16), f32)
    lk[..., 1::2] = 5.0
    return px, lk


def host_detections(graph, pixel_score, link_score, scale_x, scale_y, min_size, max_comps=64):
    """The host path, per image: link_cc_decode -> min_area_rect_boxes (host formatting), the NumPy mean score of every
    component, ordered by a stable descending sort -> [(boxes int32 [k,4,2], scores f32 [k])]"""
    from test_link_eval_host import component_scores_ref
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    labels, ncomp, _ = P.link_cc_decode(pixel_score, link_score, 0.8, 0.9, min_size=min_size, max_comps=max_comps, graph=graph)
    boxes = P.min_area_rect_boxes(labels, ncomp, scale_x, scale_y, max_comps=max_comps, graph=graph)
    ps = pixel_score.cpu().numpy() if isinstance(pixel_score, torch.Tensor) else pixel_score
    scores = component_scores_ref(labels.cpu().numpy(), ps, ncomp.cpu().numpy(), max_comps)
    out = []
    for b, (_, bx) in enumerate(boxes):
        sc = scores[b, :len(bx)]
        order = np.argsort(-sc.astype(np.float64), kind="stable")
        out.append((bx[order].astype(i32), sc[order]))
    return out


def host_image(graph, device, px, lk, h, w):
    """the host path for ONE image of original size h x w: boxes in original pixels and scores, in matching order"""
    from tensorflow_ocr_amd.tool import pixellink_fn as P
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    pixel_score = P.pixel_scores(up(px[None]), graph=graph)[..., 1].contiguous()
    link_score = P.link_scores(up(lk[None]), graph=graph)
    return host_detections(graph, pixel_score, link_score, w / 32.0, h / 32.0, 10)[0]


def host_best_box(graph, device):
    """link_eval_dir's `best_box`: the best detection of the host path, which finds every planted region"""
    def best_box(name, px, lk, h, w, n_regions):
        boxes, _ = host_image(graph, device, px, lk, h, w)
        assert len(boxes) == n_regions, name
        return boxes[0]
    return best_box


def link_eval_dir(d, best_box, text=(2.0, 4.5)):
    """3 images of two original shapes with the logits a stub forward returns for them, and per image three ground truths:
    best_box(name, px, lk, h, w, n_regions) — the best detection, exactly — an ignored quad, and one nothing matches."""
    rng = np.random.default_rng(78)
    maps = {k: link_logits(rng, [rot(32, 32, *r) for r in regions], text) for k, regions in REGIONS.items()}
    for name, (h, w) in SHAPES.items():
        np.save(os.path.join(d, name + ".npy"), rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        best = best_box(name, maps[name][0], maps[name][1], h, w, len(REGIONS[name]))
        write_gt(os.path.join(d, "gt_%s.txt" % name), [best, rect(1, 1, 9, 6), rect(w - 14, 2, w - 2, 9)], ["text", "###", "far"])
    return d, maps


def link_stub_forward(device, maps):
    """the logits of the images a batch holds, by its size: 2 = img_a, img_b (one original shape, name order); 1 = img_c"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    calls = []

    def forward(x):
        calls.append(tuple(x.shape))
        names = {2: ["img_a", "img_b"], 1: ["img_c"]}[x.shape[0]]
        return up(np.stack([maps[k][0] for k in names])), up(np.stack([maps[k][1] for k in names]))
    return forward, calls


# ------------------------------------------------------------------------------------------------ training
def run_training(script, g, step, te, batch, steps, slots=()):
    """`steps` steps of `step` on `batch`, with the evaluation `te` of the training script (or None) between them -> (the
    recorded step's C entry names and host entry tags, its plan kinds, clones of the weights, the auxiliaries, the EMA and
    the optimiser's `slots`, the evaluation results, te)"""
    results = []
    for it in range(steps):
        step(*batch)
        if te is not None and te.due(it + 1):
            script._evaluate(te, None, step.opt)
            results.append(te.last)
    torch.cuda.synchronize()
    assert step.plan is not None
    calls = [(e[0], e[3] if e[0] == "c" else (e[2] if len(e) > 2 else None)) for e in step.recorded]
    state = [t.clone() for t in (g.store.flat, g.store.flat_aux, step.opt.ema) + tuple(getattr(step.opt, k) for k in slots)]
    return calls, list(step.plan_kinds), state, results, te


def train_pixellink(device, eval_dir_path, eval_flags, steps=4):
    """train_pixellink.py's step at 2 x 64^2; eval_flags: None = no evaluation, or the flags that follow --eval_data_path"""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import pixellink
    from tensorflow_ocr_amd.train import MomentumOptimizer, TrainStep
    sys.path.insert(0, ROOT)
    T = importlib.import_module("train_pixellink")
    argv = ["--batch_size", "2", "--train_image_height", "64", "--train_image_width", "64", "--using_moving_average",
            "--eval_image_height", "64", "--eval_image_width", "64"]
    if eval_flags is not None:
        argv += ["--eval_steps", "1", "--eval_data_path", eval_dir_path] + eval_flags
    FLAGS = T.parse(argv)
    rng = np.random.default_rng(52)
    im, px, lk, _ = synthetic.make_batch(rng, 2, 64)
    batch = [torch.from_numpy(a).to(device) for a in (im, px[..., 0], lk)]

    def fl(gr, images, pixel_labels, link_labels):
        net = pixellink.PixelLinkNet(images, graph=gr, input_norm=T.INPUT_NORM)
        return net.build_loss(pixel_labels, link_labels)
    g = Graph(device, loss_scale=1024.0, seed=6)
    step = TrainStep(g, fl, lambda gr: MomentumOptimizer(gr, base_lr=1e-3, momentum=0.9, weight_decay=5e-4,
                                                         moving_average_decay=FLAGS.moving_average_decay))
    te = T.make_train_eval(FLAGS, g, step)
    assert (te is not None) == (eval_flags is not None)
    return run_training(T, g, step, te, batch, steps)


SMALL = [("block1", [(128, 64, 1), (128, 64, 2)]), ("block2", [(256, 64, 1), (256, 64, 2)]),
         ("block3", [(256, 128, 1), (256, 128, 2)]), ("block4", [(512, 128, 1)])]


def train_east_rbox(device, eval_dir_path, with_eval, steps=5):
    """multigpu_train.py's RBOX step at 2 x 64^2 on the narrow blocks SMALL, with or without an evaluation every step"""
    from tensorflow_ocr_amd import synthetic
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    from tensorflow_ocr_amd.train import AdamOptimizer, TrainStep
    sys.path.insert(0, ROOT)
    T = importlib.import_module("multigpu_train")
    argv = ["--net", "east", "--geometry", "RBOX", "--input_size", "64", "--batch_size_per_gpu", "2"]
    if with_eval:
        argv += ["--eval_steps", "1", "--eval_data_path", eval_dir_path]
    FLAGS = T.parse(argv)
    rng = np.random.default_rng(51)
    images = rng.uniform(0, 255, (2, 64, 64, 3)).astype(f32)
    batch = [torch.from_numpy(a).to(device) for a in (images,) + tuple(synthetic.rbox_labels(2, 64, rng))]

    def fl(gr, im, yy, gg, mm):
        a, b = M.model_rbox(im, text_scale=FLAGS.text_scale, graph=gr, blocks=SMALL)
        return M.loss_rbox(yy, a, gg, b, mm, graph=gr)
    g = Graph(device, loss_scale=1024.0, seed=6)
    step = TrainStep(g, fl, lambda gr: AdamOptimizer(gr, learning_rate=1e-3))
    te = T.make_train_eval(FLAGS, g, step, blocks=SMALL)
    assert (te is not None) == with_eval
    return run_training(T, g, step, te, batch, steps, slots=("m", "v"))
