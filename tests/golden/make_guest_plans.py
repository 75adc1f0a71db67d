"""Records tests/golden/guest_plans.json: what `train.schedule_guests` makes of the corpus of synthetic recordings in
tests/test_step_plan_host.py (every recording under every setting, one SHA-256 per plan) and of one real recording,
model_vgg's step at 2 x 128^2.  The tests require the same plans: run this on the commit whose scheduler is to be kept
(with this file and the test file copied onto it), BEFORE changing the scheduler — never on the rewritten one.

    python tests/golden/make_guest_plans.py [--parent HASH]          the corpus; no GPU needed
    python tests/golden/make_guest_plans.py --vgg OUT.json           the real recording's plan alone, on the GPU
    python tests/golden/make_guest_plans.py --merge OUT.json         puts that plan into the golden

HASH is the commit the scheduler is taken from (default: `git rev-parse HEAD`)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "guest_plans.json")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_step_plan_host as T                      # noqa: E402


def write(gold):
    with open(GOLDEN, "w") as f:
        f.write('{"parent": %s, "recordings": %d, "settings": %s,\n "traits": %s,\n "vgg_2x128": %s,\n "plans": {\n' % (
            json.dumps(gold["parent"]), gold["recordings"], json.dumps(gold["settings"]), json.dumps(gold["traits"]),
            json.dumps(gold.get("vgg_2x128"))))
        f.write(",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in gold["plans"].items()) + "\n }}\n")


def corpus(parent):
    from tensorflow_ocr_amd.train import schedule_guests
    n = T.RECORDINGS * len(T.SETTINGS)
    plans, count, differ = {}, dict.fromkeys(("fork", "multi", "over12", "scarce", "deferred"), 0), 0
    for seed in range(T.RECORDINGS):
        rec = T.recording(seed)
        out = [T.schedule(schedule_guests, rec, s) for s in T.SETTINGS]
        plans[str(seed)] = [T.digest(p) for p in out]
        for s, p in zip(T.SETTINGS, out):
            for k, v in T.traits(rec, p, s).items():
                count[k] += v
        differ += sum(plans[str(seed)][k] != plans[str(seed)][k + 6] for k in range(6))
    print("%d plans; " % n + ", ".join("%s %.1f %%" % (k, 100.0 * v / n) for k, v in count.items())
          + "; balance changes %d plans" % differ)
    assert count["fork"] >= 0.30 * n and count["multi"] >= 0.10 * n and differ >= 1
    assert min(count["over12"], count["scarce"], count["deferred"]) >= 0.05 * n
    old = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    write({"parent": parent, "recordings": T.RECORDINGS, "settings": [list(s) for s in T.SETTINGS], "traits": count,
           "vgg_2x128": old.get("vgg_2x128") if old.get("parent") == parent else None, "plans": plans})
    print("-> %s (%d bytes)" % (GOLDEN, os.path.getsize(GOLDEN)))


def vgg_plan():
    """The scheduled plan of model_vgg's recorded step at 2 x 128^2 with GUEST_MIN_US = 0 (at this size every pass is
    shorter than the pairing threshold), in the test's canonical form: tests/test_gpu_guests.py records the same step."""
    import numpy as np
    import torch
    from oracle import ocr_oracle as O
    from tensorflow_ocr_amd import train
    from tensorflow_ocr_amd.graph import Graph
    from tensorflow_ocr_amd.nets import model_vgg_16 as M
    train.GUEST_MIN_US = 0.0
    batch = [torch.from_numpy(a).to("cuda:0") for a in O.synthetic_batch(np.random.default_rng(0), 2, 128)]

    def fl(g, im, px, lk, mk):
        p, l = M.model_vgg(im, graph=g)
        return M.loss(px, p, lk, l, mk, graph=g)
    step = train.TrainStep(Graph("cuda:0", loss_scale=1024.0, seed=3), fl, lambda gg: train.AdamOptimizer(gg), replay=True)
    for _ in range(3):
        step(*batch)
    torch.cuda.synchronize()
    assert step.plan is not None
    return T.canonical(step.plan)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--vgg"]:
        with open(argv[1], "w") as f:
            json.dump(vgg_plan(), f)
    elif argv[:1] == ["--merge"]:
        gold = json.load(open(GOLDEN))
        gold["vgg_2x128"] = json.load(open(argv[1]))
        write(gold)
    else:
        corpus(argv[1] if argv[:1] == ["--parent"] else
               subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip())
