"""What the four drivers (multigpu_train.py, train_pixellink.py, test.py, eval_pixellink_fast.py) share: the argparse type
functions, the training flags that are not the reference's, the between-steps evaluation flags with their cross-checks, the
accumulation window and the log lines of the gradient factor.  Nothing here imports torch at module level: a driver parses
its flags before anything touches HIP, and `launch.self_launch` depends on that."""
import argparse


def _typed(fn, text):
    """`fn(text)` with its ValueError as argparse's."""
    try:
        return fn(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def loss_scale_arg(text):
    from .graph import parse_loss_scale
    return _typed(parse_loss_scale, text)


def clip_norm_arg(text):
    from .train import check_clip_norm
    return _typed(lambda t: check_clip_norm(float(t)), text)


def accumulate_steps_arg(text):
    from .train import check_accumulate_steps
    return _typed(lambda t: check_accumulate_steps(int(t)), text)


def sweep_arg(text):
    from .evaluate import sweep_arg as arg
    return arg(text)


def sweep_help(order_key):
    from .evaluate import SWEEP_HELP
    return SWEEP_HELP % order_key


def scales_arg(text):
    from .tool.rbox import scales_arg as arg
    return arg(text)


def map_scales_arg(text):
    from .tool.pixellink_fn import map_scales_arg as arg
    return arg(text)


def grid_axis_arg(text):
    """one axis of the decode-threshold grid: the sweep's syntax, LO:HI:N or a comma list"""
    return sweep_arg(text)


def add_grid_flags(ap):
    """--eval_grid_pixel / --eval_grid_link: the decode-threshold grid of the link geometry (evaluate.LinkEvaluator's grid)"""
    from .evaluate import GRID_HELP
    # (no attribute without the flag: a run that does not ask for a grid parses to the namespace it always parsed to;
    # read them with `grid_option`)
    ap.add_argument('--eval_grid_pixel', type=grid_axis_arg, default=argparse.SUPPRESS, metavar='LO:HI:N',
                    help=GRID_HELP % 'eval_')
    ap.add_argument('--eval_grid_link', type=grid_axis_arg, default=argparse.SUPPRESS, metavar='LO:HI:N',
                    help='the link thresholds of --eval_grid_pixel')


def grid_option(FLAGS):
    """the `grid=` option of evaluate.LinkEvaluator the flags ask for: (pixel thresholds, link thresholds), or None"""
    pixel_list, link_list = getattr(FLAGS, 'eval_grid_pixel', None), getattr(FLAGS, 'eval_grid_link', None)
    return None if pixel_list is None or link_list is None else (pixel_list, link_list)


def check_grid_flags(ap, FLAGS):
    """one grid flag without the other, a grid with --eval_sweep, more than 64 pairs: argparse errors -> `grid_option`"""
    from .evaluate import check_grid_flags as check
    return check(ap, getattr(FLAGS, 'eval_grid_pixel', None), getattr(FLAGS, 'eval_grid_link', None), FLAGS.eval_sweep,
                 prefix='eval_')


def add_step_flags(ap, batch_flag_name):
    """The training flags that are not the reference's (TF-1.4 trains in f32, unclipped, one batch per step)."""
    # the f16 loss scale, a number or "dynamic" (graph.DynamicLossScale: a step whose gradients overflow is skipped and the
    # scale backs off; it grows again after a run of clean steps)
    ap.add_argument('--loss_scale', type=loss_scale_arg, default=1024.0)
    # clip the un-scaled gradients to this global L2 norm on the device (train.GradClip); a step whose norm is not finite is
    # skipped.  Off by default.
    ap.add_argument('--clip_norm', type=clip_norm_arg, default=None)
    # gradient accumulation (train.TrainStep(accumulate_steps=K)): one optimiser step on the mean gradient of K micro-batches
    # of `batch_flag_name`, so one card reaches the effective batch of K.  Every step counter of the script (maximum,
    # checkpoint, summary and log intervals, the learning-rate staircase) counts OPTIMISER steps.  1 = off.
    ap.add_argument('--accumulate_steps', type=accumulate_steps_arg, default=1,
                    help='one optimiser step per this many micro-batches of %s' % batch_flag_name)
    # with the scalars and images the script's --save_summary_steps writes (0: no event file), the four per-variable
    # summaries of train_pixellink.py:179-194 (histograms of every variable and gradient, their means) from one device pass
    # over the flat buffers (summary.TensorStats)
    ap.add_argument('--summary_variables', action='store_true')


def add_train_eval_flags(ap):
    """Held-out evaluation between steps (evaluate.TrainEval; not reference flags).  Every --eval_steps optimiser steps
    (0 = off) rank 0 runs the images of --eval_data_path (images + gt_*.txt, at most --eval_max_images of them) through
    forward -> decode -> matching on the device and reports precision / recall / hmean; --eval_weights: ema = the moving
    averages, raw = the weights being trained; --eval_protocol: raster = the reference's matching rule, icdar15 = the
    official ICDAR-2015 protocol (polygon IoU); --eval_sweep LO:HI:N (or a comma list): every pass also reports the
    precision / recall curve over the matcher's order key, its best row and AP, from the one matching pass."""
    ap.add_argument('--eval_data_path', type=str, default=None, metavar='DIR')
    ap.add_argument('--eval_steps', type=int, default=0, metavar='N')
    ap.add_argument('--eval_max_images', type=int, default=None, metavar='M')
    ap.add_argument('--eval_weights', choices=['ema', 'raw'], default='ema')
    ap.add_argument('--eval_protocol', choices=['raster', 'icdar15'], default='raster')
    ap.add_argument('--eval_sweep', type=sweep_arg, default=None, metavar='LO:HI:N')


def eval_on(FLAGS):
    return bool(FLAGS.eval_steps > 0 and FLAGS.eval_data_path)


def check_train_eval_flags(ap, FLAGS, ema_available, ema_message, after_sweep=(), before_ema=()):
    """The cross-checks of `add_train_eval_flags`, first failure reported.  `after_sweep` / `before_ema`: a script's own
    (failed, message) rules that stand at these places of the order."""
    rules = [(FLAGS.eval_sweep is not None and not eval_on(FLAGS), '--eval_sweep needs --eval_data_path and --eval_steps')]
    rules += after_sweep
    rules += [(FLAGS.eval_steps < 0 or (FLAGS.eval_max_images is not None and FLAGS.eval_max_images < 1),
               '--eval_steps must not be negative and --eval_max_images must be positive'),
              (FLAGS.eval_steps > 0 and not FLAGS.eval_data_path, '--eval_steps needs --eval_data_path')]
    rules += before_ema
    rules += [(FLAGS.eval_weights == 'ema' and FLAGS.eval_steps > 0 and not ema_available, ema_message)]
    for failed, message in rules:
        if failed:
            ap.error(message)


def window(step, K, next_batch):
    """One optimiser step: K calls of `step`, each on a batch of its own.  Returns the mean of the micro-step losses as a
    device tensor (summed on the device: no read here)."""
    total = None
    for _ in range(K):
        loss = step(*next_batch())
        if K > 1:
            total = loss.clone() if total is None else total + loss
    return loss if K == 1 else total / K


def report_eval(train_eval, summaries, opt, prefix):
    """One pass between two steps (rank 0; the other ranks meet it at the next exchange): behind `prefix` (formatted with
    the optimiser step) the line the script's inference counterpart prints, and eval/precision, eval/recall, eval/hmean
    (with --eval_sweep also eval/ap, eval/best_hmean, eval/best_threshold; with the grid flags the grid's lines and
    eval/grid_best_hmean, eval/grid_best_pixel_threshold, eval/grid_best_link_threshold) in the event file where one is
    open."""
    from . import evaluate
    res = train_eval.run()
    print(prefix.format(opt.global_step) + evaluate.format_line(res), flush=True)
    if 'sweep' in res:
        print(evaluate.format_sweep(res), flush=True)
    if 'grid' in res:
        print(evaluate.format_grid(res), flush=True)
    if summaries is not None:
        train_eval.write(summaries.writer, opt.global_step)


def log_grad_factor(opt):
    """The loss-scale and gradient-norm lines of the optimiser's gradient factor policy (train.grad_factor), behind a loss
    line: the loss was just read, so a few more device reads cost nothing there."""
    for line in opt.factor.log_lines():
        print(line, flush=True)


def grad_factor_scalars(opt):
    """The same policy's summary scalars: loss_scale, grad_norm."""
    return opt.factor.scalars()
