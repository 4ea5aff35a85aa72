"""What train() decides from its test pass: the stopping rule, the monitored quantity and the checks of the keywords that go with
them.  Host code only: nothing here touches a device, so every refusal comes before any launch.

    best_and_wait(history, min_delta, mode)    the one rule: where the best epoch of a history is and how long ago
    Monitor(products, value, mode)             select on a verification product instead of on the loss
    check_*                                    the keywords of train(), each refused under its own name
"""
import math
import numbers
import os

import numpy as np

MODES = ('min', 'max')


def best_and_wait(history, min_delta=0.0, mode='min'):
    """The stopping rule of train(), over a whole history (one value per epoch, in order) ->
    (best_epoch, best_value, epochs_since_best).

    Going through the epochs in order, an epoch IMPROVES when its value is better than the best so far by more than min_delta:
    value < best - min_delta (mode 'min'), value > best + min_delta ('max').  The first value that is no NaN always improves; a
    tie (a difference of exactly min_delta included) does not, and a NaN never does.  best_epoch is the last improving epoch's
    index into `history`, best_value its value, and epochs_since_best the number of epochs after it: len(history) - 1 -
    best_epoch.  Before any improving epoch -- an empty history, NaNs only -- the result is (None, None, len(history)).

    Note that best_value is the last IMPROVING value, not the smallest one: with min_delta > 0 a later epoch may be smaller by
    less than min_delta, and the weights kept are then still the earlier epoch's."""
    if mode not in MODES:
        raise ValueError(f'mode: one of {MODES} is needed, got {mode!r}')
    best_epoch = best = None
    for epoch, value in enumerate(history):
        value = float(value)
        if math.isnan(value):
            continue
        if best is None or (value < best - min_delta if mode == 'min' else value > best + min_delta):
            best_epoch, best = epoch, value
    return best_epoch, best, len(history) - (0 if best_epoch is None else 1 + best_epoch)


class Monitor:
    """train(monitor=Monitor(products, value, mode)): select the model on a verification product.

    products   what verify(products=) takes: names of the products, or a mapping name -> that product's keywords
    value      a callable Verification -> float, e.g.  lambda v: v.extent.by_lead('model')['iiee'].mean()
    mode       'min' (smaller is better: errors) or 'max' (scores, skill)

    The test pass of every epoch then makes these products beside the loss, on the same rollout, and value(...) of the epoch's
    qtmpnn.verify.Verification is what patience, restore_best and keep_best read.  mode and value are checked here and again by
    train(): a mode outside ('min', 'max') is a ValueError, a value that cannot be called a TypeError, both naming `monitor`."""

    def __init__(self, products, value, mode='min'):
        self.products, self.value, self.mode = products, value, mode
        check_monitor(self)

    def __repr__(self):
        return f'Monitor(products={self.products!r}, value={self.value!r}, mode={self.mode!r})'


def check_patience(patience):
    """patience as None or an integer >= 1, or a refusal that names it."""
    if patience is None:
        return None
    if isinstance(patience, bool) or not isinstance(patience, (int, np.integer)):
        raise TypeError(f'patience: None or an integer >= 1 is needed (the epochs without improvement after which training stops), '
                        f'got {patience!r}')
    if patience < 1:
        raise ValueError(f'patience: an integer >= 1 is needed (the epochs without improvement after which training stops), got '
                         f'{patience!r}')
    return int(patience)


def check_min_delta(min_delta):
    """min_delta as one finite float >= 0, or a refusal that names it."""
    if isinstance(min_delta, bool) or not isinstance(min_delta, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f'min_delta: one finite number >= 0 is needed (by how much an epoch has to improve on the best), got '
                        f'{min_delta!r}')
    if not (math.isfinite(min_delta) and min_delta >= 0):
        raise ValueError(f'min_delta: one finite number >= 0 is needed (by how much an epoch has to improve on the best), got '
                         f'{min_delta!r}')
    return float(min_delta)


def check_flag(name, flag):
    """A keyword that is True or False and nothing else (1, 'yes', None are refused: they are usually another argument that
    slipped into this place)."""
    if not isinstance(flag, (bool, np.bool_)):
        raise TypeError(f'{name}: True or False is needed, got {flag!r}')
    return bool(flag)


def check_keep_best(keep_best):
    """keep_best as None or a path (str or os.PathLike; not empty), or a refusal that names it."""
    if keep_best is None:
        return None
    if not isinstance(keep_best, (str, os.PathLike)):
        raise TypeError(f'keep_best: None or a path (str or os.PathLike) for save_checkpoint() is needed, got {keep_best!r}')
    if not os.fspath(keep_best):
        raise ValueError('keep_best: the path is empty')
    return keep_best


def check_monitor(monitor):
    """monitor as 'loss' or a Monitor whose mode and value hold, or a refusal that names it."""
    if isinstance(monitor, str) and monitor == 'loss':
        return monitor
    if not isinstance(monitor, Monitor):
        raise TypeError(f"monitor: 'loss' or a qtmpnn.validation.Monitor is needed, got {monitor!r}")
    if not (isinstance(monitor.mode, str) and monitor.mode in MODES):
        raise ValueError(f'monitor: mode must be one of {MODES}, got {monitor.mode!r}')
    if not callable(monitor.value):
        raise TypeError(f'monitor: value must be a callable Verification -> float, got {monitor.value!r}')
    return monitor


def monitored_value(value, epoch):
    """What Monitor.value returned as a float, or a refusal that names `monitor`: one finite real number is needed (a Python or
    numpy scalar, or an array of one element)."""
    v = value
    if isinstance(v, np.ndarray) and v.size == 1:
        v = v.reshape(()).item()
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f'monitor: value(...) must return one finite float, got {value!r} after the test pass of epoch {epoch}')
    if not math.isfinite(v):
        raise ValueError(f'monitor: value(...) must return one finite float, got {value!r} after the test pass of epoch {epoch}')
    return float(v)
