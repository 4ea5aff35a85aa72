"""Adam + gradient clipping on the model's flat parameter vector (qtmpnn.flat) in two launches (qt_flat_adam).

Same update as the reference's `clip_grad_norm_(params, 10)` + `torch.optim.Adam(params, lr)` (model/mpnnlstm.py:174, 251-257):
Adam is elementwise and the clipping norm is the norm over all parameters, so one flat tensor gives the reference's numbers.
Keeps the torch.optim.Optimizer surface (`param_groups[0]['lr']`, `state`, `zero_grad`, StepLR works on it); with
capturable=True the learning rate lives in a device tensor and the step counter on the device, so the step can be captured
in a hipGraph and a scheduler's in-place update is seen by every replay.
"""
import torch

from . import _lib
from ._lib import ptr
from .flat import join_flat, name_table, split_flat


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False):
        if not (torch.is_tensor(flat_param) and flat_param.dim() == 1 and flat_param.is_cuda and flat_param.dtype == torch.float32):
            raise ValueError('FlatAdam takes ONE flat fp32 CUDA parameter vector (qtmpnn.flat.FlatParams.param)')
        if capturable and not torch.is_tensor(lr):
            lr = torch.tensor(float(lr), device=flat_param.device)
        super().__init__([flat_param], dict(lr=lr, betas=betas, eps=eps, capturable=capturable, fused=True))
        self.last_norm = torch.zeros(2, device=flat_param.device)       # [|g| before clipping, -]

    def _state(self, p):
        st = self.state[p]
        if not st:
            st['step'] = torch.zeros(1, dtype=torch.int32, device=p.device)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        """One update; max_norm: clip the gradient to this total norm first (in place, like clip_grad_norm_), None = no
        clipping.  The gradient norm before clipping is left in `self.last_norm[0]` (device)."""
        loss = closure() if closure is not None else None
        group = self.param_groups[0]
        p = group['params'][0]
        if p.grad is None:
            return loss
        g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
        st = self._state(p)
        lr = group['lr']
        b1, b2 = group['betas']
        _lib.call('qt_flat_adam', ptr(p), ptr(g), ptr(st['exp_avg']), ptr(st['exp_avg_sq']), p.numel(), ptr(st['step']),
                  ptr(lr) if torch.is_tensor(lr) else None, 0.0 if torch.is_tensor(lr) else float(lr), float(b1), float(b2),
                  float(group['eps']), float(max_norm) if max_norm is not None else 0.0, ptr(self.last_norm))
        if g is not p.grad:
            p.grad.copy_(g)
        return loss


# ------------------------------------------------------------------------------ Adam state by parameter name (checkpoints)
# One layout for FlatAdam (one flat tensor) and torch.optim.Adam (a state per parameter): host copies of exp_avg / exp_avg_sq per
# state-dict name in the parameter's shape, ONE integer step, lr as a float, betas, eps.  What one optimiser wrote the other reads.
def adam_state(optimizer, module):
    """The host copy of `optimizer`'s Adam state over module.named_parameters(), in the shared layout.  A parameter that has no
    state yet (no step taken, or never a gradient) has zero moments; parameters that stepped must agree on the step count."""
    group, table = optimizer.param_groups[0], name_table(module)
    zeros = lambda: {name: torch.zeros(shape) for name, _, shape in table}
    step = 0
    if isinstance(optimizer, FlatAdam):
        st = optimizer.state.get(group['params'][0])
        if st:
            m, v = (split_flat(st[k].detach().cpu(), table) for k in ('exp_avg', 'exp_avg_sq'))
            step = int(st['step'].item())
        else:
            m, v = zeros(), zeros()
    else:
        m, v, steps = zeros(), zeros(), set()
        for name, p in module.named_parameters():
            st = optimizer.state.get(p)
            if st:
                m[name], v[name] = (st[k].detach().cpu().clone() for k in ('exp_avg', 'exp_avg_sq'))
                steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError(f'step: the parameters have taken different numbers of steps {sorted(steps)}; one step count is stored')
        step = steps.pop() if steps else 0
    return {'exp_avg': m, 'exp_avg_sq': v, 'step': step, 'lr': float(group['lr']),
            'betas': tuple(float(b) for b in group['betas']), 'eps': float(group['eps'])}


def check_adam_state(state, table):
    """Refuse, by field name and on the host, a stored Adam state that does not fit the parameters of `table` (name_table) or
    that no run of Adam could have left: ValueError, before a caller changes anything."""
    for k in ('exp_avg', 'exp_avg_sq', 'step', 'lr', 'betas', 'eps'):
        if not isinstance(state, dict) or k not in state:
            raise ValueError(f'optimizer: no {k!r}')
    step, lr = state['step'], state['lr']
    if isinstance(step, bool) or not isinstance(step, int) or step < 0:
        raise ValueError(f'step: a step count >= 0 is needed, the file has {step!r}')
    if not isinstance(lr, float) or not lr == lr or lr in (float('inf'), -float('inf')):
        raise ValueError(f'lr: a finite float is needed, the file has {lr!r}')
    want = {name: shape for name, _, shape in table}
    for k in ('exp_avg', 'exp_avg_sq'):
        have = state[k]
        missing, extra = [n for n in want if n not in have], [n for n in have if n not in want]
        if missing or extra:
            raise ValueError(f'{k}: parameter names differ: missing in the file {missing}, not in this model {extra}')
        for name, shape in want.items():
            t = have[name]
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f'{k}[{name!r}]: shape {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} in the file, '
                                 f'{shape} here')
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f'{k}[{name!r}]: NaN or infinite entries')
        if k == 'exp_avg_sq' and any(bool((t < 0).any()) for t in have.values()):
            raise ValueError(f'exp_avg_sq: negative entries in {[n for n, t in have.items() if bool((t < 0).any())]}')


@torch.no_grad()
def load_adam_state(optimizer, module, state):
    """Write a checked state (check_adam_state) into `optimizer`, IN PLACE wherever the optimiser has storage already: moments and
    step counters by copy_ / fill_, a device learning rate by fill_ (a captured step reads these buffers through the pointers
    it was captured with), a float learning rate by assignment.  State that does not exist yet is made as the optimiser's own
    first step would make it."""
    group, table = optimizer.param_groups[0], name_table(module)
    if isinstance(optimizer, FlatAdam):
        st = optimizer._state(group['params'][0])
        for k in ('exp_avg', 'exp_avg_sq'):
            join_flat(state[k], table, st[k])
        st['step'].fill_(state['step'])
    else:
        on_dev = group.get('capturable') or group.get('fused')
        for name, p in module.named_parameters():
            st = optimizer.state[p]
            if not st:          # (as Adam._init_group)
                st['step'] = torch.zeros((), dtype=torch.float32, device=p.device) if on_dev else torch.tensor(0.0, dtype=torch.float32)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg'].copy_(state['exp_avg'][name])
            st['exp_avg_sq'].copy_(state['exp_avg_sq'][name])
            st['step'].fill_(state['step'])
    set_lr(group, 'lr', state['lr'])
    group['betas'], group['eps'] = tuple(state['betas']), state['eps']


def set_lr(group, key, value):
    """group[key] = value where it is a float, fill_ where it is a device tensor (the capturable learning rate keeps its storage)."""
    if torch.is_tensor(group.get(key)):
        group[key].fill_(float(value))
    else:
        group[key] = float(value)
