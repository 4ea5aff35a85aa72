"""Activation recomputation: one rollout step as ONE autograd node that keeps its inputs and re-runs the step in the backward.

segment(fn, *args) returns fn(*args).  With autograd on and a gradient wanted, fn's first run happens without autograd (the
forward-only launches where ops has them), only the tensors among `args` are saved, and the node's backward runs fn once more
on them with autograd on and differentiates that run: the step's activations live from its replay to the end of its own
backward instead of from the forward pass to it.  The replay issues the launches of the plain step on the same operands, so
outputs and gradients are the plain step's bits.

What a step shares with the other steps of its pass is kept consistent by hand:
- ops.GradAcc (the deferred parameter gradients of a packed weight): the first run counts the uses, the replay takes the same
  use indices (GradAcc.cursor) and counts nothing, so the pass's first use still emits the sum, once, after all the others;
- the attention-dropout call counter (ops._ATTN_CALLS): the replay starts from the first run's value and leaves the counter
  where it found it -- the replayed masks are the first run's, the next pass draws what it would have drawn;
- a recording of attention weights (Seq2Seq.record_attention) sees the first run only (replaying()).
Nothing here reads or sets a torch generator, and nothing synchronises: a captured step replays inside its capture.

Mode 'stream' is 'step' with one difference, which is the accumulators' and not this module's: the GradAccs of the pass are marked
(stream_accs) and then reduce every use's weight-gradient operands inside that use's backward instead of keeping them for one
grouped launch at the end.  The sum is taken in another order, so the weight gradients are the plain step's up to rounding.
"""
import copy

import torch
from torch.autograd import Function

from . import ops
from .mesh import Mesh

MODES = (None, 'step', 'stream')
_REPLAYING = [0]
_RECORDS = []           # the classes of packed-weight records (register_record)


def register_record(cls):
    """Declare a slotted class whose instances hold packed weights of a pass (tensors, GradAccs, plain values in its __slots__):
    a segment takes such a record apart and rebuilds it around the replay's leaves.  Usable as a class decorator."""
    assert getattr(cls, '__slots__', None), cls
    _RECORDS.append(cls)
    return cls


def check_mode(mode, who='set_recompute'):
    """`mode` as it is kept: one of MODES (ValueError otherwise; True and 1 are no modes)."""
    if mode is None or (isinstance(mode, str) and mode in MODES):
        return mode
    raise ValueError(f"{who}: mode must be None, 'step' or 'stream', got {mode!r}")


def stream_accs(pack):
    """Every GradAcc in the packed weights `pack` of one pass (dicts / lists / records, as segment takes them) streams from here on:
    the pass's weight gradients are summed use by use (ops.GradAcc.keep).  Returns `pack`."""
    accs = []
    _split(pack, [], accs, {})
    for a in accs:
        a.stream = True
    return pack


def replaying():
    """True while a segment's backward re-runs its forward."""
    return _REPLAYING[0] > 0


class _Slot:
    __slots__ = ('i',)

    def __init__(self, i):
        self.i = i


class _Record:
    """A slotted record that carries gradient accumulators (PackedCell, PackedConv, PackedMHConv): rebuilt as a shallow copy with
    its tensors replaced; the accumulators stay the pass's own."""
    __slots__ = ('obj', 'fields')

    def __init__(self, obj, fields):
        self.obj, self.fields = obj, fields


def _is_record(obj):
    return type(obj) in _RECORDS


def _carries_tensors(obj):
    """True for an object that is none of the kinds _split knows and holds a tensor or a GradAcc in an attribute: passed through
    as it is, its tensors would be no leaves of the replay and their gradients would be dropped."""
    names = list(getattr(obj, '__dict__', ())) + [s for s in getattr(type(obj), '__slots__', ()) if hasattr(obj, s)]
    return any(torch.is_tensor(getattr(obj, n)) or isinstance(getattr(obj, n), ops.GradAcc) for n in names)


def _split(obj, tensors, accs, seen):
    """A template of `obj` (dicts, lists, tuples, packed records) with every tensor replaced by its slot in `tensors` (one slot
    per tensor object) and every GradAcc noted in `accs`; a Mesh (constants of the pass), a number, None stay as they are; any
    other object that holds tensors is a TypeError (register_record is the way to let one in)."""
    if torch.is_tensor(obj):
        i = seen.get(id(obj))
        if i is None:
            i = seen[id(obj)] = len(tensors)
            tensors.append(obj)
        return _Slot(i)
    if isinstance(obj, ops.GradAcc):
        if all(a is not obj for a in accs):
            accs.append(obj)
        return obj
    if isinstance(obj, dict):
        return {k: _split(v, tensors, accs, seen) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_split(v, tensors, accs, seen) for v in obj)
    if _is_record(obj):
        return _Record(obj, {s: _split(getattr(obj, s), tensors, accs, seen) for s in type(obj).__slots__ if hasattr(obj, s)})
    if not isinstance(obj, Mesh) and _carries_tensors(obj):
        raise TypeError(f'recompute: a {type(obj).__name__} holds tensors and is no registered record (recompute.register_record): '
                        'its tensors would get no gradient from a replayed step')
    return obj


def _join(tpl, tensors):
    if isinstance(tpl, _Slot):
        return tensors[tpl.i]
    if isinstance(tpl, dict):
        return {k: _join(v, tensors) for k, v in tpl.items()}
    if isinstance(tpl, (list, tuple)):
        return type(tpl)(_join(v, tensors) for v in tpl)
    if isinstance(tpl, _Record):
        obj = copy.copy(tpl.obj)
        for s, v in tpl.fields.items():
            setattr(obj, s, _join(v, tensors))
        return obj
    return tpl


class _Segment(Function):
    @staticmethod
    def forward(ctx, fn, tpl, accs, wants, box, *tensors):
        lo = [a.uses for a in accs]
        calls = ops._ATTN_CALLS[0]
        ops._SEGMENT_PASS[0] += 1
        try:
            out = fn(*_join(tpl, tensors))          # autograd is off in here
        finally:
            ops._SEGMENT_PASS[0] -= 1
        outs = []
        box.append(_split(out, outs, [], {}))
        ctx.fn, ctx.tpl, ctx.accs, ctx.wants, ctx.calls = fn, tpl, accs, wants, calls
        ctx.lo, ctx.hi = lo, [a.uses for a in accs]
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        accs = ctx.accs
        leaves = [t.detach().requires_grad_(w) for t, w in zip(ctx.saved_tensors, ctx.wants)]
        calls, ops._ATTN_CALLS[0] = ops._ATTN_CALLS[0], ctx.calls
        for a, lo in zip(accs, ctx.lo):
            a.cursor = lo
        _REPLAYING[0] += 1
        try:
            with torch.enable_grad():
                out = ctx.fn(*_join(ctx.tpl, leaves))
            took = [a.cursor for a in accs]
        finally:
            _REPLAYING[0] -= 1
            ops._ATTN_CALLS[0] = calls
            for a in accs:
                a.cursor = None
        if took != ctx.hi:
            raise RuntimeError('recompute: the replay of a step used its packed weights another number of times than its first run')
        outs = []
        _split(out, outs, [], {})
        assert len(outs) == len(gouts)
        pairs = [(o, g) for o, g in zip(outs, gouts) if g is not None and o.requires_grad]
        ins = [t for t in leaves if t.requires_grad]
        grads = [None] * len(leaves)
        if pairs and ins:
            got = iter(torch.autograd.grad([o for o, _ in pairs], ins, [g for _, g in pairs], allow_unused=True))
            grads = [next(got) if t.requires_grad else None for t in leaves]
        return (None,) * 5 + tuple(grads)


def segment(fn, *args):
    """fn(*args), recomputed in the backward (see the module's text).  args: tensors, None, numbers, meshes and the packed weights
    of the pass (dicts / lists / records of tensors and GradAccs); fn returns tensors, None, or lists / tuples of them.  Without
    autograd, or when no tensor among args wants a gradient, this IS fn(*args)."""
    tensors, accs = [], []
    tpl = _split(args, tensors, accs, {})
    wants = tuple(t.is_floating_point() and t.requires_grad for t in tensors)
    if not (torch.is_grad_enabled() and any(wants)):
        return fn(*args)
    box = []
    outs = _Segment.apply(fn, tpl, accs, wants, box, *tensors)
    return _join(box[0], outs)
