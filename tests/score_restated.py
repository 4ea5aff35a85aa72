"""Forecast verification restated in numpy float64 from dense frames, written from the definitions: per lead time the masked
RMSE / MAE / bias of a field against the truth and the ice / no-ice contingency table of `field > thr`.  The checker of
qt_score_rollout, ops.rollout_scores, NextFramePredictorS2S.score() and qtmpnn.score.Scores (tests only).

Comparisons are done on the fp32 values with the threshold rounded to fp32 once: that is what decides a count.  Differences are
formed in float64 from the two fp32 values, i.e. exactly."""
import numpy as np


def restated_sums(field, truth, mask, thr):
    """field, truth (T, W, H) float32; mask (W, H) bool, True = not counted, or None; -> (sums (T, 8), absterms (T, 3)).
    sums[t] = [n, sum d, sum |d|, sum d^2, hits, over, under, correct negatives] over the unmasked pixels, d = field - truth;
    absterms[t] = [sum |d|, sum |d|, sum d^2]: the sum of |term| of slots 1-3 (what a rounding-error bound scales with)."""
    field, truth = np.asarray(field), np.asarray(truth)
    assert field.dtype == np.float32 and truth.dtype == np.float32 and field.shape == truth.shape and field.ndim == 3
    keep = np.ones(field.shape[1:], dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    t32 = np.float32(thr)
    sums, absterms = np.zeros((len(field), 8)), np.zeros((len(field), 3))
    for t in range(len(field)):
        f, y = field[t][keep], truth[t][keep]
        d = f.astype(np.float64) - y.astype(np.float64)
        fi, yi = f > t32, y > t32
        sums[t] = [f.size, d.sum(), np.abs(d).sum(), (d * d).sum(), (fi & yi).sum(), (fi & ~yi).sum(), (~fi & yi).sum(),
                   (~fi & ~yi).sum()]
        absterms[t] = [np.abs(d).sum(), np.abs(d).sum(), (d * d).sum()]
    return sums, absterms


def restated_metrics(sums):
    """The derived numbers of one (..., 8) array of sums, straight from their definitions."""
    s = np.asarray(sums, dtype=np.float64)
    out = {k: np.full(s.shape[:-1], np.nan) for k in ('bias', 'mae', 'rmse', 'accuracy')}
    out['n'] = s[..., 0].copy()
    out['over'], out['under'], out['iiee'] = s[..., 5].copy(), s[..., 6].copy(), s[..., 5] + s[..., 6]
    for idx in np.ndindex(*s.shape[:-1]):
        n = s[idx][0]
        if n > 0:
            out['bias'][idx] = s[idx][1] / n
            out['mae'][idx] = s[idx][2] / n
            out['rmse'][idx] = (s[idx][3] / n) ** 0.5
            out['accuracy'][idx] = (s[idx][4] + s[idx][7]) / n
    return out
