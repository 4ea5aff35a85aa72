"""The rollout horizon: how many output steps a call rolls out, as a setting of the call and not of the constructor
(NextFramePredictorS2S.set_horizon, horizon(k), train(horizon=)).  Host code only: nothing here touches a device, so every refusal
comes before any launch, and every one names `horizon`.

    check_horizon(k, where='')                              one horizon: an integer >= 1
    resolve_schedule(horizon, first_epoch, n_epochs, limit) train(horizon=): the horizons of a call's epochs, all checked at once
    first_steps(t, k, what)                                 the first k output steps of a target or a climatology, as a view
"""
import collections.abc

import numpy as np


def check_horizon(k, where=''):
    """k as a Python int >= 1, or a refusal that names `horizon` (and `where`, e.g. 'epoch 3: '): a TypeError for what is no
    integer -- True and floats included: 2.0 is usually another argument that slipped into this place --, a ValueError below 1."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError(f'horizon: {where}an integer >= 1 is needed (the output steps of the rollout), got {k!r}')
    if k < 1:
        raise ValueError(f'horizon: {where}an integer >= 1 is needed (the output steps of the rollout), got {k!r}')
    return int(k)


def resolve_schedule(horizon, first_epoch, n_epochs, limit=None):
    """The horizons of the epochs first_epoch .. first_epoch + n_epochs - 1 as a list of n_epochs ints, from what
    train(horizon=) was given:

        one integer      every epoch
        a sequence       entry e for epoch e, the last entry for every later epoch
        a callable       horizon(e)

    The epoch index is the index into the predictor's whole history, so a resumed run continues the schedule where the
    interrupted one stood.  A pure function: the whole list is made and checked here, before anything else happens.  Every entry
    that is used is held to check_horizon under its epoch's index, and to `limit` (None: none), the output steps the training
    targets hold; an empty sequence, and anything that is none of the three, are refused as well."""
    if isinstance(first_epoch, bool) or not isinstance(first_epoch, (int, np.integer)) or first_epoch < 0:
        raise ValueError(f'horizon: the first epoch must be an index >= 0 into the history, got {first_epoch!r}')
    epochs = range(int(first_epoch), int(first_epoch) + int(n_epochs))
    if callable(horizon):
        entry = horizon
    elif isinstance(horizon, (str, bytes)):
        raise TypeError(f'horizon: an integer, a sequence of integers (one per epoch) or a callable epoch -> integer is needed, '
                        f'got {horizon!r}')
    elif isinstance(horizon, collections.abc.Sequence) or (isinstance(horizon, np.ndarray) and horizon.ndim == 1):
        entries = list(horizon)
        if not entries:
            raise ValueError('horizon: the sequence is empty: one entry per epoch is needed, the last one holding for every later '
                             'epoch')
        entry = lambda e: entries[min(e, len(entries) - 1)]
    else:
        k = check_horizon(horizon)
        entry = lambda e: k
    schedule = [check_horizon(entry(e), f'epoch {e}: ') for e in epochs]
    if limit is not None:
        for e, k in zip(epochs, schedule):
            if k > limit:
                raise ValueError(f'horizon: epoch {e}: y holds {limit} output steps, horizon={k} needs {k}')
    return schedule


def first_steps(t, k, what='y', strict=True):
    """The first k output steps of `t`, (T, W, H, C) or (B, T, W, H, C) -- targets, or the climatology of the output days -- as
    a view: nothing is copied, the kernels read it through its clip stride.  None, and what has exactly k steps, is returned as it
    is; fewer than k steps are refused.  strict=False (no horizon was set: k is the built step count) returns a short `t` as it
    is instead, for the shape checks that were there before to refuse it in their own words."""
    if t is None or not hasattr(t, 'dim') or t.dim() not in (4, 5):
        return t
    have = t.shape[-4]
    if have < k:
        if not strict:
            return t
        raise ValueError(f'horizon: {what} holds {have} output steps, horizon={k} needs {k}')
    return t if have == k else t.narrow(t.dim() - 4, 0, k)
