"""What a reference forecast of the verification products is, stated once (beyond the reference).

`references=` of score, score_maps, reliability, fss, edge_distance, extent, event_dates and verify is a sequence of specs:

    'persistence'           channel 0 of the last input frame at every lead time
    'climatology'           the daily normals of the output days (the concat_layers the decoder gets)
    'anomaly_persistence'   AnomalyPersistence()
    AnomalyPersistence(damping=None, name=None, clip=(0.0, 1.0))

The anomaly-persistence field of clip b, output step t (0-based) and pixel p is

    f[b, t, p] = clamp(c[b, t, p] + r[t, p] * (x0[b, p] - c0[b, p]), lo, hi)

c: the climatology of the clip's output days, x0: channel 0 of the last input frame, c0: the climatology of the launch-state
day (the day before the first output day, model.utils.launch_day_index), r: the damping.  The arithmetic is fp32 in a fixed
order: d = x0 - c0, then r * d as its own rounded product (torch.mul, never a fused multiply-add), then c + that, then the
clamp; damping=None is r = 1 and leaves the product out (1 * d is d), clip=None leaves the clamp out.

No kernel and no entry point of the library is involved: the field is a few element-wise torch ops per batch (captured with
the rollout where the rollout is captured) and goes to the verification launches as one of their two dense fields; more
than two references take one more launch of the same kernels per pair (reference_launches)."""
import collections.abc

import numpy as np
import torch

PERSISTENCE, CLIMATOLOGY, ANOMALY = 'persistence', 'climatology', 'anomaly_persistence'
RESERVED = ('model', 'observed')        # the names the result classes give the forecast itself and the truth


class AnomalyPersistence:
    """The (damped) anomaly-persistence reference.  damping: None (r = 1, default name 'anomaly_persistence') or an array
    (T_out,) or (T_out, W, H), numeric, finite, every entry in [-1, 1] (default name 'damped_anomaly_persistence'), e.g.
    ClipBank.anomaly_autocorrelation(T_out)[0]; held as float32 and uploaded once per call.  clip: (lo, hi), lo < hi, both
    finite, or None for no clamp.  Nothing is checked here: check_references does it, for the call the spec is part of."""

    def __init__(self, damping=None, name=None, clip=(0.0, 1.0)):
        self.damping, self.clip = damping, clip
        self.name = name if name is not None else (ANOMALY if damping is None else 'damped_' + ANOMALY)
        self._dev = None

    def __repr__(self):
        shape = None if self.damping is None else tuple(np.shape(self.damping))
        return f'AnomalyPersistence(name={self.name!r}, damping={shape}, clip={self.clip!r})'

    def checked(self, who, T_out, frame):
        """A copy with the damping as a float32 host array and the clip as two floats, or a ValueError under `who` that names
        `references`.  frame: (W, H), or None where the call does not know it (a per-pixel damping is then held to its first
        axis here and to the batch when the field is built)."""
        what = f'{who}: references: {self.name!r}'
        if not isinstance(self.name, str) or not self.name:
            raise ValueError(f'{who}: references: a name must be a non-empty string, got {self.name!r}')
        damping = self.damping
        if damping is not None:
            a = damping.detach().cpu().numpy() if torch.is_tensor(damping) else np.asarray(damping)
            if a.dtype == object or a.dtype.kind not in 'fiu':
                raise ValueError(f'{what}: damping must be a numeric array, got dtype {a.dtype}')
            shapes = [(T_out,)] + ([(T_out, *frame)] if frame is not None else [])
            if tuple(a.shape) not in shapes and not (frame is None and a.ndim == 3 and a.shape[0] == T_out):
                raise ValueError(f'{what}: damping of shape {tuple(a.shape)}, expected {" or ".join(str(s) for s in shapes)}'
                                 + (f' or ({T_out}, W, H)' if frame is None else ''))
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(a).all():
                raise ValueError(f'{what}: damping has NaN or infinite entries')
            if (np.abs(a) > 1).any():
                raise ValueError(f'{what}: damping must lie in [-1, 1], got values in [{float(a.min())!r}, {float(a.max())!r}]')
            damping = a
        clip = self.clip
        if clip is not None:
            try:
                lo, hi = (float(v) for v in clip)
            except (TypeError, ValueError):
                raise ValueError(f'{what}: clip must be (lo, hi) or None, got {clip!r}') from None
            if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
                raise ValueError(f'{what}: clip must be lo < hi, both finite, got {clip!r}')
            clip = (lo, hi)
        return AnomalyPersistence(damping, self.name, clip)

    def damping_on(self, device):
        """The checked damping on `device`, (T_out, 1) or (T_out, P): uploaded on first use and kept."""
        if self._dev is None or self._dev.device != torch.device(device):
            self._dev = torch.from_numpy(self.damping.reshape(self.damping.shape[0], -1)).to(device)
        return self._dev


def spec_name(spec):
    return spec if isinstance(spec, str) else spec.name


def default_references(with_clim):
    """What references=None means: ('persistence',) and, with a climatology, 'climatology'."""
    return (PERSISTENCE,) + ((CLIMATOLOGY,) if with_clim else ())


def forecast_sources(with_clim, references=None):
    """The sources of a verification call: 'model', then the references' names in the order asked for (None: the default)."""
    refs = default_references(with_clim) if references is None else references
    return ('model',) + tuple(spec_name(s) for s in refs)


def check_references(who, references, with_clim, T_out, frame):
    """`references` of a verification call -> the tuple of normalised specs ('persistence', 'climatology', or a checked
    AnomalyPersistence), or a refusal under `who` that names `references`, on the host and before any launch.  TypeError for
    what is no sequence of specs; ValueError for an empty sequence, a repeated name, a name that is 'model' or 'observed', an
    unknown string, 'climatology' or an AnomalyPersistence in a call without a climatology, a damping of the wrong shape or
    dtype, with NaN or infinite entries or outside [-1, 1], a clip that is not lo < hi, both finite."""
    if isinstance(references, (str, AnomalyPersistence, torch.Tensor, np.ndarray)) \
            or not isinstance(references, collections.abc.Iterable):
        raise TypeError(f'{who}: references must be a sequence of {PERSISTENCE!r}, {CLIMATOLOGY!r}, {ANOMALY!r} or '
                        f'AnomalyPersistence objects, got {references!r}')
    specs = list(references)
    for s in specs:
        if not isinstance(s, (str, AnomalyPersistence)):
            raise TypeError(f'{who}: references must hold names or AnomalyPersistence objects, got {s!r}')
    if not specs:
        raise ValueError(f'{who}: references is empty: name at least one reference forecast (None for the default)')
    checked, seen = [], set()
    for s in specs:
        if isinstance(s, str):
            if s in RESERVED:
                raise ValueError(f'{who}: references: {s!r} is the name of the forecast or the truth, no reference')
            if s not in (PERSISTENCE, CLIMATOLOGY, ANOMALY):
                raise ValueError(f'{who}: references: unknown reference {s!r}: the names are {PERSISTENCE!r}, {CLIMATOLOGY!r} and '
                                 f'{ANOMALY!r}')
            if s == ANOMALY:
                s = AnomalyPersistence()
        if not isinstance(s, str):
            if s.name in RESERVED:
                raise ValueError(f'{who}: references: {s.name!r} is the name of the forecast or the truth, no reference')
            s = s.checked(who, T_out, frame)
        name = spec_name(s)
        if name in seen:
            raise ValueError(f'{who}: references: {name!r} is given twice: every reference needs a name of its own '
                             '(AnomalyPersistence(name=...))')
        seen.add(name)
        if s != PERSISTENCE and not with_clim:
            raise ValueError(f'{who}: references: {name!r} needs a climatology and the call has none')
        checked.append(s)
    return tuple(checked)


def needs_launch_climatology(specs):
    return any(not isinstance(s, str) for s in specs)


def launch_frame(x):
    """Channel 0 of the last input frame, (W, H) or (B, W, H): the persistence forecast of every lead time, and the state at launch
    that the event dates count from."""
    return x[..., -1, :, :, 0]


def reference_fields(x, concat, c0, specs):
    """The dense field of every spec of `specs` for one batch -> {spec: tensor}, on x's device.  x: (T_in, W, H, C) or
    (B, T_in, W, H, C); concat: the climatology of the output days, (T_out, W, H, 1) or (B, T_out, W, H, 1), or None; c0: the
    climatology of the launch-state day, (W, H, 1) or (B, W, H, 1), needed by the AnomalyPersistence specs only.
    'persistence' is launch_frame(x) and 'climatology' is concat, the tensors themselves; an AnomalyPersistence is the field of
    the module docstring, (T_out, P) or (B, T_out, P) float32, in its fixed order of operations.  The verification launches
    read a (B, P) field as one frame for every lead time and a (B, T, P) field per step (ops._score_args)."""
    fields, d = {}, None
    for s in specs:
        if s in fields:
            continue
        if s == PERSISTENCE:
            fields[s] = launch_frame(x)
        elif s == CLIMATOLOGY:
            fields[s] = concat
        else:
            if concat is None or c0 is None:
                raise ValueError(f'references: {s.name!r} needs the climatology of the output days and of the launch-state day')
            if concat.shape[-1] != 1 or c0.shape[-1] != 1:
                raise ValueError(f'references: {s.name!r} needs a climatology of one variable, got {concat.shape[-1]}')
            lead = tuple(concat.shape[:-3])                         # (T_out,) or (B, T_out)
            c = concat.to(torch.float32).reshape(*lead, -1)
            if d is None:                                           # one anomaly for every anomaly reference of the batch
                d = (launch_frame(x).to(torch.float32).reshape(*lead[:-1], -1)
                     - c0.to(torch.float32).reshape(*lead[:-1], -1)).unsqueeze(-2)
            a = d
            if s.damping is not None:
                r = s.damping_on(x.device)
                if r.shape[-1] not in (1, c.shape[-1]):
                    raise ValueError(f'references: {s.name!r}: damping of {tuple(s.damping.shape)} for frames of {c.shape[-1]} pixels')
                a = torch.mul(r, d)
            f = c + a
            fields[s] = f if s.clip is None else f.clamp(s.clip[0], s.clip[1])
    return fields


def reference_launches(k):
    """The launches of k references: the verification kernels take two dense fields per launch, so launch i carries the
    references [2 i, 2 i + 2) -> ceil(k / 2) ranges (one launch, without a field, for k = 0)."""
    return [(i, min(i + 2, k)) for i in range(0, k, 2)] or [(0, 0)]
