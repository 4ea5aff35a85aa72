"""An exponential moving average of the weights: the shadow that validation, prediction and checkpoints read (beyond the
reference).  It holds the averaged weights and nothing else; the trainer (model/mpnnlstm.py: set_ema, averaged_weights,
train(ema=)) decides when it is updated and who reads it.  No kernel of the library is involved: the update is two element-wise
torch ops over ~1e5 floats, short enough to sit in the captured step beside clip + Adam.

    check_decay(decay)                  the decay as a float in [0, 1), or a refusal that names `ema`
    WeightEMA(params, decay)            the shadow of one flat tensor or of a list of parameters
    check_state(state, table)           a stored state held to the parameters of a name table, by field name
"""
import numbers

import numpy as np
import torch

from .flat import join_flat, name_table, split_flat


def check_decay(decay):
    """decay as a float in [0, 1), or a refusal that names `ema`: TypeError for what is no real number (True and False included),
    ValueError for a number outside [0, 1) or a NaN.  Host code: nothing is launched."""
    if isinstance(decay, (bool, np.bool_)) or not isinstance(decay, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f'ema: None or one decay in [0, 1) is needed (s <- decay * s + (1 - decay) * p after every optimiser '
                        f'step), got {decay!r}')
    decay = float(decay)
    if not 0.0 <= decay < 1.0:              # (a NaN fails both comparisons)
        raise ValueError(f'ema: the decay must lie in [0, 1), got {decay!r}')
    return decay


class WeightEMA:
    """The exponential moving average of `params`: ONE tensor (FlatParams.param, the ChebConv / GCNConv path) or a list of
    tensors (the parameter list of the attention stacks).  The shadow `s` has the shapes of the parameters, fp32, on their
    device, and starts at ZERO; `updates` (t) is a host integer.

    THE ARITHMETIC, stated once.  With d = decay, both constants Python floats that the ops round to fp32:

        update()       s.mul_(d);  s.add_(p, alpha=1 - d)               (a list: torch._foreach_mul_, torch._foreach_add_)
                       t += 1
        averaged(out)  out = s / c,  c = fp32(1 - d ** t), formed in float64 on the host and rounded once

    update() is two in-place launches, fixed: no host read, no allocation, no value that differs from call to call, so a graph
    capture holds it as it stands and the host count advances once per replay (the caller's to do: advance()).  s / c is the
    bias-corrected average: s_t = (1 - d) sum_i d^(t - i) p_i has the weights sum 1 - d^t, so s_t / (1 - d^t) is a proper
    weighted mean of the iterates p_1..p_t from the first update on -- a constant p gives p, and the start weights never enter.
    d = 0 is the last iterate, exactly.  averaged() before any update is refused by name (the mean of nothing)."""

    def __init__(self, params, decay):
        self.decay = check_decay(decay)
        self.flat = torch.is_tensor(params)
        self.params = params if self.flat else list(params)
        tensors = [self.params] if self.flat else self.params
        if not tensors or any(p.dtype != torch.float32 for p in tensors):
            raise ValueError('ema: the parameters must be fp32 tensors, at least one')
        shadow = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in tensors]
        self.shadow = shadow[0] if self.flat else shadow
        self.updates = 0

    @torch.no_grad()
    def update(self):
        """s <- d s + (1 - d) p on the parameters as they are now (after the optimiser step), then t += 1."""
        d = self.decay
        if self.flat:
            self.shadow.mul_(d)
            self.shadow.add_(self.params, alpha=1.0 - d)
        else:
            torch._foreach_mul_(self.shadow, d)
            torch._foreach_add_(self.shadow, self.params, alpha=1.0 - d)
        self.updates += 1

    def advance(self, j=1):
        """t += j: a replay of a capture that holds update()'s launches has run them j times without the host's knowing."""
        self.updates += j

    def divisor(self):
        """c = fp32(1 - d ** t) as a Python float, or the refusal of t == 0."""
        if self.updates < 1:
            raise ValueError('ema: no optimiser step has been averaged yet')
        return float(np.float32(1.0 - self.decay ** self.updates))

    @torch.no_grad()
    def averaged(self, out):
        """out = s / c in place: `out` is one tensor or a list shaped like the shadow (the parameters themselves, for one).  -> out"""
        c = self.divisor()
        if self.flat:
            torch.div(self.shadow, c, out=out)
        else:
            torch._foreach_copy_(out, self.shadow)
            torch._foreach_div_(out, c)
        return out

    def state(self, module):
        """The host copy {'shadow': {name: tensor in the parameter's shape}, 'decay': float, 'updates': int} over
        module.named_parameters(): the layout of qtmpnn.optim.adam_state, one for both kinds of shadow."""
        table = name_table(module)
        if self.flat:
            shadow = split_flat(self.shadow.detach().cpu(), table)
        else:
            shadow = {name: s.detach().cpu().clone() for (name, _, _), s in zip(table, self.shadow, strict=True)}
        return {'shadow': shadow, 'decay': self.decay, 'updates': int(self.updates)}

    @torch.no_grad()
    def load_state(self, state):
        """Write a checked state (check_state: its names are the parameters', in their order) into the shadow IN PLACE, by
        copy_: a step captured earlier holds pointers into this storage and goes on from the loaded values.  The decay is the
        caller's to compare; the count is taken."""
        named = state['shadow']
        if self.flat:
            table, off = [], 0
            for name, t in named.items():
                table.append((name, off, tuple(t.shape)))
                off += t.numel()
            if off != self.shadow.numel():
                raise ValueError(f'shadow: {off} elements in the state, {self.shadow.numel()} here')
            join_flat(named, table, self.shadow)
        else:
            for s, t in zip(self.shadow, named.values(), strict=True):
                s.copy_(t)
        self.updates = int(state['updates'])


def check_state(state, table):
    """Refuse, by field name and on the host, a stored EMA state that does not fit the parameters of `table` (name_table) or
    that no run could have left: ValueError, before a caller changes anything."""
    for k in ('shadow', 'decay', 'updates'):
        if not isinstance(state, dict) or k not in state:
            raise ValueError(f'ema: no {k!r}')
    decay, updates, have = state['decay'], state['updates'], state['shadow']
    if isinstance(decay, bool) or not isinstance(decay, float) or not 0.0 <= decay < 1.0:
        raise ValueError(f'decay: a float in [0, 1) is needed, the state has {decay!r}')
    if isinstance(updates, bool) or not isinstance(updates, int) or updates < 0:
        raise ValueError(f'updates: an update count >= 0 is needed, the state has {updates!r}')
    if not isinstance(have, dict):
        raise ValueError(f'shadow: a dict name -> tensor is needed, the state has {type(have).__name__}')
    want = {name: shape for name, _, shape in table}
    missing, extra = [n for n in want if n not in have], [n for n in have if n not in want]
    if missing or extra or list(have) != list(want):
        raise ValueError(f'shadow: parameter names differ: missing in the state {missing}, not in this model {extra}'
                         + ('' if missing or extra else ' (same names, another order)'))
    for name, shape in want.items():
        t = have[name]
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError(f'shadow[{name!r}]: shape {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} '
                             f'{t.dtype if torch.is_tensor(t) else ""} in the state, fp32 {shape} here')
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f'shadow[{name!r}]: NaN or infinite entries')
    if updates == 0 and any(bool(t.any()) for t in have.values()):
        raise ValueError('updates: 0 updates with a shadow that is not zero')


WeightEMA.check_state = staticmethod(check_state)
