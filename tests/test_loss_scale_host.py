"""CPU: host side of dynamic loss scaling — argument validation of graph.DynamicLossScale, the precisions it is refused
for, the training scripts' `--loss_scale` flag, and the checkpoint round trip of its two scalars.  (Everything that moves
the scale runs on the device: tests/test_gpu_loss_scale.py.)"""
import numpy as np
import pytest
import torch


def test_defaults_and_argument_validation():
    from tensorflow_ocr_amd.graph import DynamicLossScale
    d = DynamicLossScale()
    assert (d.init_scale, d.growth_factor, d.backoff_factor, d.growth_interval, d.min_scale, d.max_scale) == \
        (2.0 ** 16, 2.0, 0.5, 2000, 1.0, 2.0 ** 24)
    DynamicLossScale(init_scale=1.0, min_scale=1.0, max_scale=1.0)              # min == init == max is a (degenerate) range
    bad = [dict(init_scale=0.0), dict(init_scale=-4.0), dict(growth_factor=-2.0), dict(backoff_factor=0.0),
           dict(min_scale=0.0), dict(max_scale=float("inf")), dict(init_scale=float("nan")),
           dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=1.0), dict(backoff_factor=2.0),
           dict(init_scale=0.5), dict(init_scale=2.0 ** 25), dict(min_scale=8.0, max_scale=4.0, init_scale=6.0),
           dict(growth_interval=0), dict(growth_interval=-3), dict(growth_interval=2.5), dict(init_scale="big")]
    for kw in bad:
        with pytest.raises(ValueError):
            DynamicLossScale(**kw)


def test_only_the_f16_training_precision_takes_a_dynamic_scale():
    from tensorflow_ocr_amd.graph import DynamicLossScale, Graph
    for precision in ("f32", "f16x2"):
        with pytest.raises(ValueError, match="f16"):
            Graph("cpu", precision=precision, loss_scale=DynamicLossScale())
    with pytest.raises(ValueError):
        Graph(precision="f32", loss_scale=DynamicLossScale())
    cfg = DynamicLossScale(init_scale=4096.0)
    g, g2 = Graph("cpu", loss_scale=cfg), Graph("cpu", loss_scale=cfg)
    assert g.loss_scaler is not None and g.loss_scaler is not g2.loss_scaler is not cfg      # each graph binds its own state
    assert g.loss_scale == 4096.0 and g.loss_scaler.scale() == 4096.0
    assert g.loss_scaler.skipped_steps() == 0 and g.loss_scaler.good_steps() == 0
    # a number keeps the static path
    gs = Graph("cpu", loss_scale=512)
    assert gs.loss_scaler is None and gs.loss_scale == 512.0 and gs.seed_scale() == 512.0
    assert Graph("cpu").loss_scaler is None and Graph("cpu").loss_scale == 1024.0


@pytest.mark.parametrize("script", ["multigpu_train", "train_pixellink"])
def test_scripts_parse_the_loss_scale_flag(script):
    import importlib
    from tensorflow_ocr_amd.graph import DynamicLossScale
    mod = importlib.import_module(script)
    assert mod.parse([]).loss_scale == 1024.0                                   # the default is what it was
    v = mod.parse(["--loss_scale", "512"]).loss_scale
    assert isinstance(v, float) and v == 512.0
    d = mod.parse(["--loss_scale", "dynamic"]).loss_scale
    assert isinstance(d, DynamicLossScale) and d.init_scale == 2.0 ** 16
    for bad in ("sometimes", "-8", "0", "nan"):
        with pytest.raises(SystemExit):
            mod.parse(["--loss_scale", bad])


def _tower(loss_scale):
    from tensorflow_ocr_amd import graph as G
    from tensorflow_ocr_amd.train import AdamOptimizer
    g = G.Graph("cpu", loss_scale=loss_scale, seed=2)
    with g.variable_scope("feature_fusion"):
        g.get_variable("Conv/weights", (1, 1, 4, 3), G.xavier_uniform(g.rng), regularized=True)
        g.get_variable("Conv/biases", (3,), G.constant(0.5))
    return g, AdamOptimizer(g)


def test_checkpoint_round_trip_of_scale_and_good_steps(tmp_path):
    from tensorflow_ocr_amd import checkpoint
    from tensorflow_ocr_amd.graph import DynamicLossScale
    cfg = DynamicLossScale(init_scale=2.0 ** 12, growth_interval=100)
    g, opt = _tower(cfg)
    g.loss_scaler.load_state_dict({"scale": 2.0 ** 9, "good_steps": 37})
    assert g.loss_scaler.state_dict() == {"scale": np.float32(512.0), "good_steps": np.int64(37)}
    opt.global_step = 11
    checkpoint.save_training_state(str(tmp_path / "dyn"), g, opt)
    g2, opt2 = _tower(cfg)
    assert g2.loss_scaler.scale() == 2.0 ** 12
    assert checkpoint.restore_training_state(str(tmp_path / "dyn"), g2, opt2) == 11
    assert g2.loss_scaler.scale() == 512.0 and g2.loss_scaler.good_steps() == 37
    assert torch.equal(g2.store.flat, g.store.flat)
    # the two scalars are no model variables
    sd, step = checkpoint.load_tf_checkpoint(str(tmp_path / "dyn"))
    assert step == 11 and not [k for k in sd if k.startswith("loss_scale")]
    # a checkpoint of a static run has neither: a dynamic graph restores to init_scale, whatever it held before
    gs, opts = _tower(1024.0)
    checkpoint.save_training_state(str(tmp_path / "static"), gs, opts)
    g2.loss_scaler.load_state_dict({"scale": 2.0, "good_steps": 5})
    checkpoint.restore_training_state(str(tmp_path / "static"), g2, opt2)
    assert g2.loss_scaler.scale() == 2.0 ** 12 and g2.loss_scaler.good_steps() == 0
    # and a static graph reads a dynamic run's checkpoint as before
    assert checkpoint.restore_training_state(str(tmp_path / "dyn"), gs, opts) == 11
    assert gs.loss_scaler is None
    # restored values are held to the configured range
    g2.loss_scaler.load_state_dict({"scale": 2.0 ** 30, "good_steps": 1000})
    assert g2.loss_scaler.scale() == cfg.max_scale and g2.loss_scaler.good_steps() == 99
