"""Input attribution maps of a forecast as NextFramePredictorS2S.sensitivity() returns them (numpy only).

For every clip b and requested lead time t the forecast is summarised by one number,

    J[b, t] = sum_p w_p y_hat[b, t, p] / sum_p w_p        over the unmasked pixels p, w = `target`,

and `maps[b, l]` is an array shaped like the clip's input frames (T_in, W, H, C) that says where that number comes from: its
gradient ('gradient'), the gradient times (x - baseline) ('gradient_x_input') or integrated gradients along the straight path
from the baseline to x ('integrated').  The device leaves the maps and the values of J; every reduction a user reads -- by
input day, by channel, per pixel, the completeness residual of integrated gradients -- is formed here.  check_request() holds
the argument checks of the call: host only, before any launch, every refusal a ValueError that names the argument."""
import numbers

import numpy as np

METHODS = ('gradient', 'gradient_x_input', 'integrated')
DEFAULT_STEPS = 16      # path points of 'integrated' when the caller names none
MAX_STEPS = 256
CHUNK = 32              # clips per batched rollout of the integrated-gradients path


def _host(a):
    """numpy view of an array-like or a torch tensor (detached, on the host) without importing torch here."""
    if hasattr(a, 'detach') and hasattr(a, 'cpu'):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


class Request:
    """The checked arguments of one sensitivity() call for inputs of shape `x_shape` ((T_in, W, H, C) or (B, T_in, W, H, C)) and
    a model of `T_out` output steps:

        target    (W, H) float32 weights, zero under the mask; sum_w their float64 sum (> 0)
        leads     tuple of output steps, strictly increasing, in [0, T_out)
        method    one of METHODS
        steps     path points of 'integrated' (None for the other methods)
        baseline  None (zeros) or a float32 array of shape (T_in, W, H, C) or x's own shape

    mask: the host bool mask of the call (True = not counted) or None."""

    def __init__(self, x_shape, T_out, mask=None, target=None, leads=None, method='gradient', baseline=None, steps=DEFAULT_STEPS):
        x_shape = tuple(int(v) for v in x_shape)
        if len(x_shape) not in (4, 5):
            raise ValueError(f'x: shape {x_shape}, expected (T_in, W, H, C) or (B, T_in, W, H, C)')
        clip = x_shape[-4:]
        frame = clip[1:3]
        if mask is not None:
            mask = np.asarray(mask) != 0
            if mask.shape != frame:
                raise ValueError(f'mask: shape {mask.shape} for frames of {frame}')
        if not isinstance(method, str) or method not in METHODS:
            raise ValueError(f'method: {method!r} is not one of {METHODS}')
        self.method = method
        # leads
        if leads is None:
            leads = range(int(T_out))
        try:
            leads = list(leads)
        except TypeError:
            raise ValueError(f'leads: a sequence of output steps is needed, got {leads!r}') from None
        if not leads:
            raise ValueError('leads: empty -- name at least one output step')
        for t in leads:
            if isinstance(t, (bool, np.bool_)) or not isinstance(t, (numbers.Integral, np.integer)):
                raise ValueError(f'leads: output steps are integers, got {t!r}')
            if not 0 <= int(t) < int(T_out):
                raise ValueError(f'leads: step {int(t)} is outside [0, {int(T_out)}) (the output steps)')
        leads = tuple(int(t) for t in leads)
        if any(b <= a for a, b in zip(leads, leads[1:])):
            raise ValueError(f'leads: the steps must be strictly increasing, got {leads}')
        self.leads = leads
        # steps
        if method == 'integrated':
            if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (numbers.Integral, np.integer)) \
                    or not 1 <= int(steps) <= MAX_STEPS:
                raise ValueError(f'steps: the number of path points must be an integer in 1..{MAX_STEPS}, got {steps!r}')
            self.steps = int(steps)
        else:
            if not (isinstance(steps, (numbers.Integral, np.integer)) and not isinstance(steps, (bool, np.bool_))
                    and int(steps) == DEFAULT_STEPS):
                raise ValueError(f"steps: path points belong to method='integrated', not to {method!r} (got steps={steps!r})")
            self.steps = None
        # baseline
        if baseline is not None and method == 'gradient':
            raise ValueError("baseline: method='gradient' is the raw gradient and takes no baseline ('gradient_x_input' and "
                             "'integrated' do)")
        if baseline is not None:
            baseline = _host(baseline)
            if baseline.dtype == object or baseline.dtype.kind not in 'fiub':
                raise ValueError(f'baseline: a numeric array is needed, got dtype {baseline.dtype}')
            if tuple(baseline.shape) not in (clip, x_shape):
                raise ValueError(f'baseline: shape {tuple(baseline.shape)}, expected {clip}' + (f' or {x_shape}' if x_shape != clip else ''))
            baseline = np.ascontiguousarray(baseline, dtype=np.float32)
            if not np.isfinite(baseline).all():
                raise ValueError('baseline: NaN or infinite entries')
        self.baseline = baseline
        # target
        if target is None:
            w = np.ones(frame, np.float32)
        else:
            w = _host(target)
            if w.dtype == object or w.dtype.kind not in 'fiub':
                raise ValueError(f'target: a numeric array is needed, got dtype {w.dtype}')
            if tuple(w.shape) != frame:
                raise ValueError(f'target: shape {tuple(w.shape)}, expected {frame}')
            w = np.array(w, dtype=np.float32)
            if not np.isfinite(w).all():
                raise ValueError('target: NaN or infinite entries')
            if (w < 0).any():
                raise ValueError('target: negative entries')
        if mask is not None:
            w[mask] = 0.0
        self.target = w
        self.sum_w = float(w.astype(np.float64).sum())
        if not self.sum_w > 0:
            raise ValueError('target: the weights of the unmasked pixels sum to 0')


class Sensitivity:
    """maps (B, L, T_in, W, H, C) float32: per clip and requested lead the attribution of J over the clip's input frames;
    leads (L,) the output steps; method one of METHODS; target (W, H) the weights of J (zero under the mask); J (B, L) float64
    the values of the functional; J_baseline (B, L) float64, its values at the baseline -- 'integrated' only, else None.
    The constructor checks shapes and dtypes and raises ValueError by field name."""

    def __init__(self, maps, leads, method, target, J, J_baseline=None):
        if not isinstance(method, str) or method not in METHODS:
            raise ValueError(f'method: {method!r} is not one of {METHODS}')
        maps = np.asarray(maps)
        if maps.dtype != np.float32:
            raise ValueError(f'maps: float32 is needed, got {maps.dtype}')
        if maps.ndim != 6:
            raise ValueError(f'maps: shape {maps.shape}, expected (B, L, T_in, W, H, C)')
        B, L = maps.shape[:2]
        leads = tuple(leads)
        if len(leads) != L or any(isinstance(t, (bool, np.bool_)) or not isinstance(t, (numbers.Integral, np.integer)) for t in leads) \
                or any(b <= a for a, b in zip(leads, leads[1:])) or (leads and leads[0] < 0):
            raise ValueError(f'leads: {leads} for maps of {L} lead(s): expected {L} strictly increasing output steps >= 0')
        target = np.asarray(target)
        if target.dtype.kind != 'f' or target.shape != maps.shape[3:5]:
            raise ValueError(f'target: {target.dtype} of shape {target.shape}, expected a float array of shape {maps.shape[3:5]}')
        J = np.asarray(J)
        if J.dtype != np.float64 or J.shape != (B, L):
            raise ValueError(f'J: {J.dtype} of shape {J.shape}, expected float64 of shape {(B, L)}')
        if (J_baseline is not None) != (method == 'integrated'):
            raise ValueError(f"J_baseline: belongs to method='integrated' and to no other (method={method!r}, J_baseline "
                             f"{'given' if J_baseline is not None else 'missing'})")
        if J_baseline is not None:
            J_baseline = np.asarray(J_baseline)
            if J_baseline.dtype != np.float64 or J_baseline.shape != (B, L):
                raise ValueError(f'J_baseline: {J_baseline.dtype} of shape {J_baseline.shape}, expected float64 of shape {(B, L)}')
        self.maps, self.leads, self.method, self.target, self.J, self.J_baseline = maps, tuple(int(t) for t in leads), method, target, J, J_baseline

    def _lead(self, lead):
        if lead not in self.leads:
            raise KeyError(f'no lead {lead!r} in these maps (have {self.leads})')
        return self.leads.index(lead)

    def _reduced(self, axes, lead, absolute):
        m = self.maps.astype(np.float64)
        out = (np.abs(m) if absolute else m).sum(axis=axes)
        return out if lead is None else out[:, self._lead(lead)]

    def by_day(self, lead=None, absolute=True):
        """(B, L, T_in), or (B, T_in) for one lead: the sum of |map| (absolute=False: of map) over pixels and channels."""
        return self._reduced((3, 4, 5), lead, absolute)

    def by_channel(self, lead=None, absolute=True):
        """(B, L, C), or (B, C) for one lead: the sum of |map| (absolute=False: of map) over days and pixels."""
        return self._reduced((2, 3, 4), lead, absolute)

    def pixel_map(self, lead, day=None, channel=None, absolute=False):
        """(B, W, H) for one lead: the map (absolute=True: |map|) summed over the input days and channels, or at the one `day`
        / `channel` given."""
        m = self.maps[:, self._lead(lead)].astype(np.float64)              # (B, T_in, W, H, C)
        if absolute:
            m = np.abs(m)
        m = m.sum(axis=1) if day is None else m[:, day]                     # (B, W, H, C)
        return m.sum(axis=-1) if channel is None else m[..., channel]

    def completeness(self):
        """(B, L): sum of the map - (J - J_baseline), the residual of the completeness axiom of integrated gradients (zero in
        the limit of many path points: what is left is the midpoint rule's error).  'integrated' only."""
        if self.method != 'integrated':
            raise ValueError(f"completeness: defined for method='integrated' only (these maps are {self.method!r})")
        return self.maps.astype(np.float64).sum(axis=(2, 3, 4, 5)) - (self.J - self.J_baseline)

    def pooled(self):
        """The mean over the clips, as a Sensitivity of one clip (maps, J and J_baseline averaged)."""
        return Sensitivity(self.maps.astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32), self.leads, self.method,
                           self.target, self.J.mean(axis=0, keepdims=True),
                           None if self.J_baseline is None else self.J_baseline.mean(axis=0, keepdims=True))
