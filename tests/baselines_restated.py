"""The reference forecasts of qtmpnn.baselines, restated in numpy: the anomaly-persistence field in float64 and in float32 with
the stated order of operations, the launch-state day from the calendar, and the anomaly autocorrelation of a series as an
explicit loop over segments and day pairs.  Nothing here imports the package."""
import datetime

import numpy as np

DAY = 86_400_000_000_000


def day_index(stamp):
    """0-based day of the year of a ns stamp, from the calendar (local time, as the loaders' stamps are read)."""
    d = datetime.datetime.fromtimestamp(int(stamp) / 1e9).date()
    return (d - datetime.date(d.year, 1, 1)).days


def launch_day(stamp):
    """The day-of-year index of the calendar day before the first output day: 31 December of the year before for a 1 January
    launch (365 after a leap year, 364 after a common one)."""
    d = datetime.datetime.fromtimestamp(int(stamp) / 1e9).date() - datetime.timedelta(days=1)
    return (d - datetime.date(d.year, 1, 1)).days


def output_days(stamp, T_out):
    d0 = datetime.datetime.fromtimestamp(int(stamp) / 1e9).date()
    return [((d0 + datetime.timedelta(days=t)) - datetime.date((d0 + datetime.timedelta(days=t)).year, 1, 1)).days
            for t in range(T_out)]


def _r(damping, T_out, dtype):
    if damping is None:
        return np.ones((T_out, 1, 1), dtype)
    r = np.asarray(damping, dtype=np.float32).astype(dtype)         # (the damping is held as float32)
    return r.reshape(T_out, 1, 1) if r.ndim == 1 else r


def field64(c, x0, c0, damping=None, clip=(0.0, 1.0)):
    """f[t] = clamp(c[t] + r[t] * (x0 - c0)) in float64 from the float32 inputs.  c (T_out, W, H), x0 and c0 (W, H)."""
    c, x0, c0 = (np.asarray(a, np.float32).astype(np.float64) for a in (c, x0, c0))
    f = c + _r(damping, len(c), np.float64) * (x0 - c0)[None]
    return f if clip is None else np.clip(f, clip[0], clip[1])


def field32(c, x0, c0, damping=None, clip=(0.0, 1.0)):
    """The float32 form in the stated order: d = x0 - c0, then r * d as its own rounded product (left out for r = 1), then
    c + that, then the clamp."""
    c, x0, c0 = (np.asarray(a, np.float32) for a in (c, x0, c0))
    d = (x0 - c0).astype(np.float32)[None]
    a = d if damping is None else (_r(damping, len(c), np.float32) * d).astype(np.float32)
    f = (c + a).astype(np.float32)
    return f if clip is None else np.clip(f, np.float32(clip[0]), np.float32(clip[1]))


def autocorrelation(y, times, normals, segments, selected, max_lag):
    """(Cy, max_lag, W, H) float64: per channel, lag and pixel  sum a[d] a[d + lag] / sqrt(sum a[d]^2 sum a[d + lag]^2)  over the
    day pairs (d, d + lag) of one segment that are both selected, a[d] = y[d] - normals[c, day_index(times[d])]; 0 where the
    denominator is 0.  y (D, W, H, Cy) float32, normals (Cy, 366, W, H) float32, selected (D,) bool."""
    D, W, H, Cy = y.shape
    a = np.stack([y[d].astype(np.float64) - np.moveaxis(normals[:, day_index(times[d])].astype(np.float64), 0, -1) for d in range(D)])
    out = np.zeros((Cy, max_lag, W, H))
    for k in range(max_lag):
        lag = k + 1
        sxy, sxx, syy = (np.zeros((W, H, Cy)) for _ in range(3))
        for s, e in segments:
            for d in range(s, e - lag):
                if selected[d] and selected[d + lag]:
                    sxy += a[d] * a[d + lag]
                    sxx += a[d] * a[d]
                    syy += a[d + lag] * a[d + lag]
        den = np.sqrt(sxx * syy)
        with np.errstate(divide='ignore', invalid='ignore'):
            out[:, k] = np.moveaxis(np.where(den > 0, sxy / den, 0.0), -1, 0)
    return out
