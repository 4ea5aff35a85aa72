"""Probability verification restated in numpy from dense frames, written from the definitions: per lead time the forecast
values of the counted pixels are binned into K equal bins of [0, 1] and every bin keeps [n, events, sum f, sum (f - o)^2] with
o = (truth > thr).  The checker of qt_reliability_rollout, ops.rollout_reliability and NextFramePredictorS2S.reliability()
(tests only).

What decides an integer is done as the device does it: the event on the fp32 truth with the threshold rounded to fp32 once
(strict >), the bin from t = f * K in np.float32 arithmetic (one rounding): 0 if not t >= 1 (small, negative and NaN values),
K - 1 if t >= K, else the integer part of t.  The float sums are float64 sums of terms formed in float64 from the fp32 values."""
import numpy as np


def bin_of(f, K):
    """Bins (int64, shape of f) of fp32 values f for K bins."""
    f = np.asarray(f)
    assert f.dtype == np.float32 and 2 <= K <= 32
    Kf = np.float32(K)
    with np.errstate(invalid='ignore', over='ignore'):
        t = f * Kf
    assert t.dtype == np.float32
    k = np.zeros(f.shape, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        mid, top = (t >= np.float32(1)) & ~(t >= Kf), t >= Kf
    k[mid] = t[mid].astype(np.int64)
    k[top] = K - 1
    return k


def restated_reliability(field, truth, mask, thr, K):
    """field, truth (T, W, H) float32; mask (W, H) bool, True = not counted, or None; -> (sums (T, K, 4), absterms (T, K, 2)).
    sums[t, k] = [n, events, sum f, sum (f - o)^2] over the unmasked pixels of bin k; absterms[t, k] = [sum |f|,
    sum (f - o)^2]: the sum of |term| of slots 2 and 3 (what a rounding-error bound scales with)."""
    field, truth = np.asarray(field), np.asarray(truth)
    assert field.dtype == np.float32 and truth.dtype == np.float32 and field.shape == truth.shape and field.ndim == 3
    keep = np.ones(field.shape[1:], dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    t32 = np.float32(thr)
    sums, absterms = np.zeros((len(field), K, 4)), np.zeros((len(field), K, 2))
    for t in range(len(field)):
        f, y = field[t][keep], truth[t][keep]
        o = y > t32
        k = bin_of(f, K)
        f64 = f.astype(np.float64)
        d = f64 - o.astype(np.float64)
        for b in range(K):
            sel = k == b
            sums[t, b] = [sel.sum(), (sel & o).sum(), f64[sel].sum(), (d[sel] * d[sel]).sum()]
            absterms[t, b] = [np.abs(f64[sel]).sum(), (d[sel] * d[sel]).sum()]
    return sums, absterms
