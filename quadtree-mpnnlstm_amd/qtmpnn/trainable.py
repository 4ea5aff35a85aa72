"""Which parameters an optimiser step updates (NextFramePredictorS2S.set_trainable, training_only(patterns), train(trainable=)):
the pure parts.  Host code, apart from flat_mask's one upload: every refusal comes before any launch, and every one names
`trainable`.

    check_patterns(patterns)              None, or the patterns as a tuple of strings
    resolve_trainable(names, patterns)    one bool per name: some pattern matches it
    encoder_frozen(names, flags)          whether the encoder cut applies: no parameter under `encoder.` is trainable
    flat_mask(table, flags, device)       the 0/1 fp32 mask over the flat parameter vector

THE ORACLE is torch's own rule for requires_grad=False parameters, stated on this project's step: forward, loss and backward as
ever; the frozen entries of the gradient are zero before the (all-reduced) gradient is used; the clipping norm is the norm of
the trainable gradients; Adam updates the trainable entries; frozen parameters keep their bits.
"""
import collections.abc
import fnmatch

import torch


def check_patterns(patterns):
    """None (everything is trainable) as it is, else the fnmatch patterns as a tuple of strings.  TypeError for one plain string
    ('decoder.*' is usually a forgotten pair of brackets: it would be read letter by letter), for what is no sequence, and for an
    entry that is no string; ValueError for an empty sequence."""
    if patterns is None:
        return None
    if isinstance(patterns, (str, bytes)):
        raise TypeError(f'trainable: None or a sequence of fnmatch patterns is needed, got the plain string {patterns!r} '
                        f'(write ({patterns!r},))')
    if not isinstance(patterns, collections.abc.Sequence):
        raise TypeError(f'trainable: None or a sequence of fnmatch patterns over the state-dict names is needed, got {patterns!r}')
    patterns = tuple(patterns)
    if not patterns:
        raise ValueError('trainable: the sequence of patterns is empty: None makes every parameter trainable, a selection names '
                         'at least one pattern')
    for p in patterns:
        if not isinstance(p, str):
            raise TypeError(f'trainable: every pattern must be a string, got {p!r}')
    return patterns


def resolve_trainable(names, patterns):
    """One bool per entry of `names` (the state-dict names, in their order): True iff some pattern matches the name
    (fnmatch.fnmatchcase: * ? [seq], case-sensitive); None: all True.  A pure function: nothing is changed, and everything that
    is wrong with a selection is said here -- what check_patterns refuses, a pattern that matches no name (ValueError: the
    pattern and the top-level names, a misspelt `decode.*` would otherwise freeze the whole model without a word) and a
    selection that leaves nothing trainable (ValueError; with fnmatch patterns the refusal before it already covers that case,
    the check states the contract for whatever the matching rule becomes)."""
    names = list(names)
    patterns = check_patterns(patterns)
    if patterns is None:
        return tuple(True for _ in names)
    for p in patterns:
        if not any(fnmatch.fnmatchcase(n, p) for n in names):
            tops = tuple(dict.fromkeys(n.split('.')[0] for n in names))
            raise ValueError(f'trainable: the pattern {p!r} matches no parameter name; the names start with {tops} '
                             "(named_parameters() lists them, e.g. 'decoder.fc_out1.lins.0.weight')")
    flags = tuple(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in names)
    if not any(flags):
        raise ValueError(f'trainable: the patterns {patterns} leave nothing trainable')
    return flags


def encoder_frozen(names, flags):
    """True when the model has parameters under `encoder.` and none of them is trainable: the rollout's encoder phase then
    needs no autograd graph (Seq2Seq.set_encoder_cut)."""
    enc = [f for n, f in zip(names, flags, strict=True) if n.startswith('encoder.')]
    return bool(enc) and not any(enc)


def flat_mask(table, flags, device=None):
    """The fp32 mask over the flat parameter vector of `table` (qtmpnn.flat.name_table: [(name, offset, shape)]): 1.0 on the
    elements of a trainable parameter, 0.0 on those of a frozen one.  g.mul_(mask) is then exact: g * 1 is g, g * 0 is 0."""
    n = 0
    for _, off, shape in table:
        n = max(n, off + int(torch.Size(shape).numel()))
    mask = torch.zeros(n, dtype=torch.float32)
    for (_, off, shape), f in zip(table, flags, strict=True):
        if f:
            mask[off:off + int(torch.Size(shape).numel())] = 1.0
    return mask if device is None else mask.to(device)
