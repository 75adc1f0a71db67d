"""CPU: the four drivers' flags against tests/golden/train_tail_trace.json (key "cli") — recorded by
tests/golden/make_train_tail_trace.py from THIS file on the commit from before the drivers' shared flag code moved into
tensorflow_ocr_amd/cli.py.  Per driver: `vars(parse([]))`, `vars(parse(argv))` for one argv with every flag set, and for every
`ap.error` rule of its `parse` (and every argparse type function of a flag) an argv that triggers it, with the message
argparse printed."""
import importlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_tail_trace.json")
DRIVERS = ("multigpu_train", "train_pixellink", "test", "eval_pixellink_fast")

EVAL_ON = ["--eval_data_path", "d", "--eval_steps", "5"]
RBOX = ["--net", "east", "--geometry", "RBOX"]
FULL = {
    "multigpu_train": [
        "--input_size", "256", "--batch_size_per_gpu", "3", "--num_readers", "2", "--learning_rate", "0.01", "--max_steps", "7",
        "--moving_average_decay", "0.9", "--gpu_list", "0,1", "--checkpoint_path", "/c/", "--restore", "--save_checkpoint_steps", "11",
        "--save_summary_steps", "13", "--pretrained_model_path", "/p", "--training_data_path", "/t/", "--net", "east",
        "--loss_scale", "dynamic", "--clip_norm", "2.5", "--accumulate_steps", "4", "--augment", "east,max_rotate_deg=10",
        "--summary_variables", "--geometry", "RBOX", "--text_scale", "256", "--eval_data_path", "/e", "--eval_steps", "9",
        "--eval_max_images", "17", "--eval_weights", "raw", "--eval_protocol", "icdar15", "--eval_sweep", "0.1:0.9:5",
        "--eval_scales", "0.5,1,2", "--eval_fuse", "vote"],
    "train_pixellink": [
        "--train_with_ignored", "--train_dir", "/t", "--checkpoint_path", "/c", "--batch_size", "8", "--num_gpus", "2",
        "--max_number_of_steps", "7", "--log_every_n_steps", "3", "--learning_rate", "0.1", "--lr_policy", "staircase",
        "--lr_breakpoints", "1,2", "--lr_decays", "0.5,0.25", "--momentum", "0.8", "--weight_decay", "0.001",
        "--using_moving_average", "--moving_average_decay", "0.99", "--num_readers", "4", "--dataset_dir", "/d",
        "--train_image_width", "256", "--train_image_height", "256", "--loss_scale", "512", "--clip_norm", "1",
        "--accumulate_steps", "2", "--save_summary_steps", "5", "--summary_variables", "--pixel_loss", "instance_balanced",
        "--max_neg_pos_ratio", "2", "--eval_data_path", "/e", "--eval_steps", "9", "--eval_max_images", "17", "--eval_weights", "ema",
        "--eval_image_width", "640", "--eval_image_height", "384", "--eval_protocol", "icdar15", "--eval_sweep", "0.5,0.7",
        "--eval_map_scales", "0.5,1,2", "--eval_flip"],
    "test": [
        "--input_size", "256", "--gpu_list", "0", "--test_data_path", "/t", "--checkpoint_path", "/c/", "--output_dir", "/o/",
        "--precision", "f16x2", "--no-fold-bn", "--geometry", "RBOX", "--text_scale", "256", "--box_thresh", "0.1", "--gt_path", "/g",
        "--eval_protocol", "icdar15", "--eval_sweep", "0.1:0.9:5", "--scales", "0.5,1,2", "--fuse", "vote"],
    "eval_pixellink_fast": [
        "--checkpoint_path", "/c", "--test_data_path", "/t/", "--gt_path", "/g", "--pixel_conf_threshold", "0.7",
        "--link_conf_threshold", "0.6", "--eval_image_width", "640", "--eval_image_height", "384", "--min_side", "4", "--min_area", "30",
        "--batch_size", "2", "--synthetic", "3", "--precision", "f32", "--eval_protocol", "icdar15", "--eval_sweep", "0.5,0.7",
        "--map_scales", "0.5,1,2", "--flip"],
}
TRAIN_TYPE_ERRORS = [["--loss_scale", "much"], ["--loss_scale", "-1"], ["--clip_norm", "0"], ["--clip_norm", "nan"],
                     ["--clip_norm", "much"], ["--accumulate_steps", "0"], ["--accumulate_steps", "1.5"],
                     ["--eval_sweep", "much"], ["--eval_sweep", "0.9:0.1:0"]]
# every ap.error rule of the four `parse` functions, in source order (a rule with two arms: one argv per arm), then the
# type functions of the flags
ERRORS = {
    "multigpu_train": [
        RBOX + ["--eval_scales", "0.5,1"],
        ["--eval_fuse", "vote"],
        ["--eval_sweep", "0.5,0.7"],
        ["--eval_protocol", "icdar15"],
        ["--geometry", "RBOX"],
        ["--eval_steps", "-1"],
        RBOX + EVAL_ON + ["--eval_max_images", "0"],
        ["--eval_steps", "5"],
        EVAL_ON,
        ["--eval_data_path", "d"],
        RBOX + EVAL_ON + ["--moving_average_decay", "0"],
    ] + TRAIN_TYPE_ERRORS + [["--eval_scales", "much"], ["--eval_scales", "0"], ["--augment", "much"], ["--net", "much"]],
    "train_pixellink": [
        ["--eval_map_scales", "0.5,1"],
        ["--eval_flip"],
        ["--eval_sweep", "0.5,0.7"],
        ["--eval_steps", "-1"],
        EVAL_ON + ["--eval_max_images", "0"],
        ["--eval_steps", "5"],
        EVAL_ON,
    ] + TRAIN_TYPE_ERRORS + [["--eval_map_scales", "much"], ["--eval_map_scales", "0"], ["--max_neg_pos_ratio", "-1"],
                             ["--pixel_loss", "much"]],
    "test": [
        ["--scales", "0.5,1"],
        ["--fuse", "vote"],
        ["--eval_sweep", "0.5,0.7"],
        ["--gt_path", "g"],
        ["--eval_protocol", "icdar15"],
        ["--eval_sweep", "much"], ["--scales", "much"], ["--scales", "0"],
    ],
    "eval_pixellink_fast": [
        ["--min_side", "-1"],
        ["--min_area", "-1"],
        ["--batch_size", "0"],
        ["--synthetic", "2"],
        ["--eval_sweep", "much"], ["--map_scales", "much"], ["--map_scales", "0"],
    ],
}


def render(v):
    from tensorflow_ocr_amd.graph import DynamicLossScale
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [render(x) for x in v]
    if isinstance(v, DynamicLossScale):
        return ["DynamicLossScale", v.init_scale, v.growth_factor, v.backoff_factor, v.growth_interval, v.min_scale, v.max_scale]
    return [type(v).__name__] + [[k, render(x)] for k, x in sorted(vars(v).items()) if not k.startswith("_") and k != "log"]


def flags(driver, argv):
    return {k: render(v) for k, v in vars(importlib.import_module(driver).parse(list(argv))).items()}


def error_text(driver, argv, capsys):
    with pytest.raises(SystemExit) as e:
        importlib.import_module(driver).parse(list(argv))
    assert e.value.code == 2
    return capsys.readouterr().err.split(": error: ", 1)[1].strip()


def record_all(capsys):
    return json.loads(json.dumps({d: {"defaults": flags(d, []), "full": flags(d, FULL[d]),
                                      "errors": [[argv, error_text(d, argv, capsys)] for argv in ERRORS[d]]} for d in DRIVERS}))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cli"]


@pytest.mark.parametrize("driver", DRIVERS)
def test_golden_holds_every_rule_of_the_parent(golden, driver):
    want = golden[driver]
    assert [argv for argv, _ in want["errors"]] == ERRORS[driver]
    # one fully populated argv: no flag of the driver is left at its default
    assert sorted(want["defaults"]) == sorted(want["full"])
    left = [k for k in want["full"] if want["full"][k] == want["defaults"][k]]
    assert left == {"multigpu_train": [], "train_pixellink": ["lr_policy", "eval_weights"], "test": [],
                    "eval_pixellink_fast": []}[driver]       # (a flag with one legal value; `ema` is the legal one here)
    rules = {"multigpu_train": 9, "train_pixellink": 5, "test": 5, "eval_pixellink_fast": 3}[driver]
    assert len({msg for _, msg in want["errors"] if not msg.startswith("argument ")}) == rules


@pytest.mark.parametrize("which", ["defaults", "full"])
@pytest.mark.parametrize("driver", DRIVERS)
def test_flags_parse_to_what_the_parent_parsed(golden, driver, which):
    got = json.loads(json.dumps(flags(driver, [] if which == "defaults" else FULL[driver])))
    assert got == golden[driver][which]


@pytest.mark.parametrize("driver", DRIVERS)
def test_every_error_rule_says_what_the_parent_said(golden, driver, capsys):
    for argv, want in golden[driver]["errors"]:
        assert error_text(driver, argv, capsys) == want, argv
