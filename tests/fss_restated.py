"""Fractions Skill Score sums restated in numpy int64 from dense frames, written from the definition: zero-padded indicator
fields and window counts by 2-D cumulative sums.  The checker of qt_fss_rollout, ops.rollout_fss and
NextFramePredictorS2S.fss() (tests only; imports nothing of the package).

counted(p): not under the mask and, where `counted` is given, true there (a pixel with a node).  I_o = counted & (truth > thr),
I_s = counted & (field > thr), on the fp32 values with the threshold rounded to fp32 once, strict: a NaN is not ice.  The window
count of scale n = 2h + 1 at (r, c) is the sum of the indicator over rows r - h .. r + h and columns c - h .. c + h, positions
outside the frame adding 0.  Per step and scale, over the counted centres: [n, events = sum I_o, sum (c_s - c_o)^2, sum c_s^2,
sum c_o^2]."""
import numpy as np


def indicator(values, counted, thr):
    """(..., W, H) int64 0 / 1: counted & (values > fp32(thr)) on fp32 values."""
    values = np.asarray(values)
    assert values.dtype == np.float32
    with np.errstate(invalid='ignore'):
        return (counted & (values > np.float32(thr))).astype(np.int64)


def window_counts(ind, n):
    """(W, H) int64 indicator -> (W, H) int64 sums over the n x n window around every pixel, zero outside the frame."""
    assert n % 2 == 1 and ind.ndim == 2
    h, (W, H) = n // 2, ind.shape
    cs = np.zeros((W + 2 * h + 1, H + 2 * h + 1), dtype=np.int64)
    cs[h + 1:h + 1 + W, h + 1:h + 1 + H] = ind
    cs = cs.cumsum(axis=0).cumsum(axis=1)                               # cs[i, j] = sum of the padded field over [0, i) x [0, j)
    return cs[n:n + W, n:n + H] - cs[:W, n:n + H] - cs[n:n + W, :H] + cs[:W, :H]


def restated_fss(field, truth, mask, thr, scales, counted=None):
    """field, truth (T, W, H) float32; mask (W, H) bool, True = not counted, or None; counted (T, W, H) bool or None (all);
    -> sums (T, K, 5) int64."""
    field, truth = np.asarray(field), np.asarray(truth)
    assert field.dtype == np.float32 and truth.dtype == np.float32 and field.shape == truth.shape and field.ndim == 3
    keep = np.ones(field.shape, dtype=bool) if counted is None else np.asarray(counted, dtype=bool).copy()
    assert keep.shape == field.shape
    if mask is not None:
        keep &= ~np.asarray(mask, dtype=bool)[None]
    sums = np.zeros((len(field), len(scales), 5), dtype=np.int64)
    for t in range(len(field)):
        io, i_s = indicator(truth[t], keep[t], thr), indicator(field[t], keep[t], thr)
        for k, n in enumerate(scales):
            co, cs = window_counts(io, n)[keep[t]], window_counts(i_s, n)[keep[t]]
            sums[t, k] = [keep[t].sum(), io.sum(), ((cs - co) ** 2).sum(), (cs * cs).sum(), (co * co).sum()]
    return sums
