"""Parameter groups: a learning-rate scale and a decoupled weight decay per parameter (NextFramePredictorS2S.set_param_groups,
train(param_groups=), param_group_table).  The pure parts and the device mechanism; every refusal comes before any launch and
names `param_groups`.

    check_groups(groups)               None, or the setting as a tuple of (pattern, (lr_scale, weight_decay))
    resolve_groups(names, groups)      {name: (lr_scale, weight_decay)}: the FIRST matching pattern decides, else (1, 0)
    GroupedStep(params, table)         the vectors of a setting and the launches around the optimiser's own step

THE RULE is torch's AdamW with a learning rate lr * s_i and a decay lam_i per entry i, lr the optimiser's current learning rate:

    p_i <- p_i * (1 - lr * s_i * lam_i)
    p_i <- p_i - lr * s_i * mhat_i / (sqrt(vhat_i) + eps)

with the moments and the one step count updated as ever, for every entry, also where s_i = 0.  THE MECHANISM leaves the
optimiser's step (qt_flat_adam, torch's fused Adam) as it is and works around it, in fp32 element-wise launches over the parameter
vector that sit in the graph that holds clip + Adam:

    before()   D  = fl(1 + fl(nsl * lr)),  nsl = -fp32(s * lam)         two launches into the work vector
               p  = fl(p * D)                                           D is exactly 1 where s * lam = 0: those bits stay
               p0 = p                                                   the stash, allocated once
    (the optimiser's step at the learning rate lr: p = p0 - lr * mhat / (sqrt(vhat) + eps))
    after()    w  = fl(p - p0);  w = fl(w * s);  w = fl(w + p0)         the blend p0 + s (p - p0), on the entries with s != 1
               p  = w where s != 1                                      s = 0 gives fl(0 + p0) = p0: those bits stay

A flat-vector model runs them as plain tensor ops on the flat buffer's parameter range (its views and its zero pad tail are not
touched) and selects with one torch.where; a parameter-list model runs torch._foreach_* on the sub-lists that need them -- the
scale is one number per parameter there -- so unit parameters are never written.  Nothing reads the host, nothing is allocated
per step, and the learning rate is read where it lives (a device tensor when capturable: StepLR is followed by replays).
"""
import collections.abc
import fnmatch
import math
import numbers

import numpy as np
import torch

OPTIONS = ('lr_scale', 'weight_decay')
UNIT = (1.0, 0.0)


def _number(key, value, pattern):
    """value as a float, or the refusal: TypeError for what is no real number (True and False included), ValueError for a
    negative number, a NaN or an infinity."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f'param_groups: {key} of the pattern {pattern!r} must be a finite number >= 0, got {value!r}')
    value = float(value)
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError(f'param_groups: {key} of the pattern {pattern!r} must be a finite number >= 0, got {value!r}')
    return value


def check_groups(groups):
    """None (no setting) as it is, else the setting as a tuple of (pattern, (lr_scale, weight_decay)) with the defaults filled
    in: the form two settings are compared in.  A dict is read in its insertion order.  TypeError for a plain string, for what
    is neither a sequence nor a dict, for a pair that is no (str, dict) and for an option that is no number; ValueError for an
    empty sequence, an unknown option key and a number that is negative or not finite."""
    if groups is None:
        return None
    if isinstance(groups, (str, bytes)):
        raise TypeError(f'param_groups: None or a sequence of (pattern, options) pairs is needed, got the plain string {groups!r} '
                        f"(write [({groups!r}, dict(lr_scale=..., weight_decay=...))])")
    if isinstance(groups, collections.abc.Mapping):
        groups = list(groups.items())
    if not isinstance(groups, collections.abc.Sequence):
        raise TypeError(f'param_groups: None or a sequence of (pattern, options) pairs is needed, got {groups!r}')
    if not len(groups):
        raise ValueError('param_groups: the sequence of pairs is empty: None is no setting, a setting names at least one pattern')
    out = []
    for pair in groups:
        if (isinstance(pair, (str, bytes)) or not isinstance(pair, collections.abc.Sequence) or len(pair) != 2
                or not isinstance(pair[0], str) or not isinstance(pair[1], collections.abc.Mapping)):
            raise TypeError(f'param_groups: every entry must be a pair (pattern: str, options: dict), got {pair!r}')
        pattern, options = pair
        for key in options:
            if key not in OPTIONS:
                raise ValueError(f'param_groups: unknown option {key!r} of the pattern {pattern!r}; the options are {OPTIONS}')
        out.append((pattern, (_number('lr_scale', options.get('lr_scale', UNIT[0]), pattern),
                              _number('weight_decay', options.get('weight_decay', UNIT[1]), pattern))))
    return tuple(out)


def as_pairs(setting):
    """check_groups' tuple back as (pattern, options) pairs (None stays None): what set_param_groups takes."""
    return None if setting is None else [(p, dict(lr_scale=s, weight_decay=lam)) for p, (s, lam) in setting]


def resolve_groups(names, groups):
    """{name: (lr_scale, weight_decay)} over `names` (the state-dict names, in their order): the FIRST pair whose pattern
    matches the name (fnmatch.fnmatchcase: * ? [seq], case-sensitive) decides it; a name that nothing matches, and every name
    under None, has (1.0, 0.0).  A pure function, the counterpart of qtmpnn.trainable.resolve_trainable: nothing is changed, and
    everything that is wrong with a setting is said here -- what check_groups refuses, and a pattern that is the first match of
    no name (ValueError: a misspelt `decode.*` would otherwise leave its parameters at the defaults without a word; the message
    lists the top-level names, and where the pattern does match names that an earlier pattern has taken it names that one)."""
    names = list(names)
    groups = check_groups(groups)
    table = {n: UNIT for n in names}
    if groups is None:
        return table
    taken = {}
    for i, (pattern, _) in enumerate(groups):
        for n in names:
            if n not in taken and fnmatch.fnmatchcase(n, pattern):
                taken[n] = i
    for i, (pattern, _) in enumerate(groups):
        if i in taken.values():
            continue
        tops = tuple(dict.fromkeys(n.split('.')[0] for n in names))
        matched = [n for n in names if fnmatch.fnmatchcase(n, pattern)]
        if matched:
            earlier = tuple(dict.fromkeys(groups[taken[n]][0] for n in matched))
            raise ValueError(f'param_groups: the pattern {pattern!r} is the first match of no parameter: it is shadowed, every one '
                             f'of the {len(matched)} names it matches is decided by an earlier pattern {earlier} (the first '
                             f'matching pair decides; put the narrower pattern first); the names start with {tops}')
        raise ValueError(f'param_groups: the pattern {pattern!r} is the first match of no parameter: it matches no name; the names '
                         f"start with {tops} (named_parameters() lists them, e.g. 'decoder.fc_out1.lins.0.weight')")
    for n, i in taken.items():
        table[n] = groups[i][1]
    return table


def fp32(x):
    return float(np.float32(x))


class GroupedStep:
    """The vectors of one setting over `params` -- ONE flat fp32 tensor (FlatParams.param) or the list of parameters, in the order
    of `table` (qtmpnn.flat.name_table) -- and the launches around the optimiser's step (the module docstring has the rule).
    Five buffers of the parameter count, allocated here, once: s, nsl, the work vector, the stash, and the bool selector of the
    blend.  set() fills them IN PLACE (a captured step reads them by pointer) and decides on the host, once, which launches a
    step issues: none at all for a setting that is (1, 0) everywhere."""

    def __init__(self, params, table):
        self.flat = torch.is_tensor(params)
        self.params = params.detach() if self.flat else [p.detach() for p in params]       # (the same storage, no autograd)
        self.table = list(table)
        self.sizes = [int(torch.Size(shape).numel()) for _, _, shape in self.table]
        self.n = sum(self.sizes)
        first = self.params if self.flat else self.params[0]
        if self.flat and self.params.numel() != self.n:
            raise ValueError(f'param_groups: the flat vector has {self.params.numel()} elements, the names cover {self.n}')
        new = lambda dtype=torch.float32: torch.zeros(self.n, dtype=dtype, device=first.device)
        self.s, self.nsl, self.work, self.stash, self.blended = new(), new(), new(), new(), new(torch.bool)
        self.decay = self.blend = False
        self._decay_lists = self._blend_lists = None

    def _views(self, vec, which):
        return [vec[off:off + n].view(shape) for j, ((_, off, shape), n) in enumerate(zip(self.table, self.sizes)) if j in which]

    @torch.no_grad()
    def set(self, resolved, trainable=None):
        """Take the setting `resolved` (resolve_groups' dict over the table's names) under the trainable flags `trainable` (one
        bool per name, None: all): a frozen entry gets neither decay nor blend -- its update is exactly zero already."""
        trainable = [True] * len(self.table) if trainable is None else list(trainable)
        s, nsl, blended = np.ones(self.n, np.float32), np.zeros(self.n, np.float32), np.zeros(self.n, bool)
        decayed, scaled, scales = set(), set(), []
        for j, ((name, off, _), n, live) in enumerate(zip(self.table, self.sizes, trainable, strict=True)):
            scale, lam = (fp32(v) for v in resolved[name])
            s[off:off + n] = scale
            if live and scale * lam != 0.0:
                nsl[off:off + n] = -np.float32(scale * lam)
                decayed.add(j)
            if live and scale != 1.0:
                blended[off:off + n] = True
                scaled.add(j)
                scales.append(scale)
        self.s.copy_(torch.from_numpy(s))
        self.nsl.copy_(torch.from_numpy(nsl))
        self.blended.copy_(torch.from_numpy(blended))
        self.decay, self.blend = bool(decayed), bool(scaled)
        if not self.flat:
            pick = lambda which: [p for j, p in enumerate(self.params) if j in which]
            self._decay_lists = (pick(decayed), self._views(self.work, decayed))
            self._blend_lists = (pick(scaled), self._views(self.work, scaled), self._views(self.stash, scaled), scales)

    @torch.no_grad()
    def before(self, lr):
        """The decay and the stash, ahead of the optimiser's step.  lr: the optimiser's learning rate as it holds it, a float or
        a 0-dim device tensor."""
        if self.decay:
            torch.mul(self.nsl, lr, out=self.work)
            self.work.add_(1.0)
            if self.flat:
                self.params.mul_(self.work)
            else:
                torch._foreach_mul_(*self._decay_lists)
        if self.blend:
            if self.flat:
                self.stash.copy_(self.params)
            else:
                torch._foreach_copy_(self._blend_lists[2], self._blend_lists[0])

    @torch.no_grad()
    def after(self):
        """The blend p0 + s (p - p0), behind the optimiser's step, on the entries with s != 1."""
        if not self.blend:
            return
        if self.flat:
            torch.sub(self.params, self.stash, out=self.work)
            self.work.mul_(self.s)
            self.work.add_(self.stash)
            torch.where(self.blended, self.work, self.params, out=self.params)
        else:
            params, work, stash, scales = self._blend_lists
            torch._foreach_copy_(work, params)
            torch._foreach_sub_(work, stash)
            torch._foreach_mul_(work, scales)
            torch._foreach_add_(work, stash)
            torch._foreach_copy_(params, work)
