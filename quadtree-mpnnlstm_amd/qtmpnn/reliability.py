"""Probability verification numbers as NextFramePredictorS2S.reliability() returns them (numpy only).

The device leaves four sums per (clip, lead time, source, bin) over the counted pixels whose forecast value falls in the bin
(ops.rollout_reliability, qt_reliability_rollout): the K bins divide [0, 1] equally, values below 0 and above 1 are in the end
bins.  Everything a user reads is derived from those sums here, and clips are pooled by summing their sums first, as
qtmpnn.score.Scores does: never a mean of ratios."""
import numpy as np

SLOTS = ('n', 'events', 'sum_f', 'sum_sq_err')


def _ratio(a, b):
    """a / b, NaN where b == 0, without a warning."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


class Reliability:
    """sums (n_clips, T_out, S, K, 4) float64 in SLOTS order: per bin the counted pixels n, the observed events
    (y > threshold), the sum of the forecast values f and the sum of (f - o)^2 with o the event as 0 / 1.  sources: S names
    ('model', then the references'); threshold: the one that defined the event."""

    def __init__(self, sums, sources, threshold):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.sources = tuple(sources)
        self.threshold = float(threshold)
        if self.sums.ndim != 5 or self.sums.shape[2] != len(self.sources) or self.sums.shape[4] != 4:
            raise ValueError(f'Reliability: sums of shape {self.sums.shape} for sources {self.sources}: expected '
                             f'(n_clips, T_out, {len(self.sources)}, bins, 4)')
        if not 2 <= self.sums.shape[3] <= 32:
            raise ValueError(f'Reliability: {self.sums.shape[3]} bins (sums of shape {self.sums.shape}): expected 2..32')
        if not self.sources or len(set(self.sources)) != len(self.sources):
            raise ValueError(f'Reliability: sources must be distinct names, got {self.sources}')
        self.bins = self.sums.shape[3]

    def _of(self, source):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these reliability sums (have {self.sources})')
        return self.sums[:, :, self.sources.index(source)]                 # (n_clips, T_out, K, 4)

    def _pooled(self, source):
        return self._of(source).sum(axis=0)                                # (T_out, K, 4)

    def curve(self, source='model'):
        """The reliability diagram per lead time over all clips: {'edges' (K + 1,) bin edges k / K, 'n' (T_out, K) pixels per
        bin (the sharpness histogram), 'mean_forecast' = sum f / n and 'observed_frequency' = events / n, both (T_out, K)}.
        An empty bin gives NaN.  A calibrated forecast has observed_frequency == mean_forecast."""
        s = self._pooled(source)
        n = s[..., 0]
        return {'edges': np.arange(self.bins + 1) / self.bins, 'n': n, 'mean_forecast': _ratio(s[..., 2], n),
                'observed_frequency': _ratio(s[..., 1], n)}

    def brier(self, source='model'):
        """Brier score (n_clips, T_out) per launch date and lead time: sum (f - o)^2 over all bins / counted pixels."""
        s = self._of(source)
        return _ratio(s[..., 3].sum(axis=-1), s[..., 0].sum(axis=-1))

    def by_lead(self, source='model'):
        """{name: (T_out,)} over all clips, from the pooled sums: 'n', 'brier', 'base_rate' (events / n) and Murphy's
        decomposition over the bins, with f_k, o_k a bin's mean forecast and observed frequency and o the base rate:
        'reliability' = sum n_k (f_k - o_k)^2 / n, 'resolution' = sum n_k (o_k - o)^2 / n, 'uncertainty' = o (1 - o).
        The forecasts of a bin are not all equal, so the three terms do not add up to the Brier score: 'residual' =
        brier - (reliability - resolution + uncertainty) is what the binning leaves (the within-bin variance and covariance
        terms), reported rather than assumed zero."""
        s = self._pooled(source)
        n, ev, sf, sq = (s[..., k] for k in range(4))
        N = n.sum(axis=-1)
        base = _ratio(ev.sum(axis=-1), N)
        fk, ok = _ratio(sf, n), _ratio(ev, n)
        full = n > 0
        rel = _ratio(np.where(full, n * (np.where(full, fk, 0.0) - np.where(full, ok, 0.0)) ** 2, 0.0).sum(axis=-1), N)
        res = _ratio(np.where(full, n * (np.where(full, ok, 0.0) - base[..., None]) ** 2, 0.0).sum(axis=-1), N)
        unc = base * (1.0 - base)
        brier = _ratio(sq.sum(axis=-1), N)
        return {'n': N, 'brier': brier, 'base_rate': base, 'reliability': rel, 'resolution': res, 'uncertainty': unc,
                'residual': brier - (rel - res + unc)}

    def skill(self, source='model', reference='climatology'):
        """Brier skill score (T_out,) over all clips: 1 - BS(source) / BS(reference); NaN where BS(reference) == 0."""
        for name in (source, reference):
            if name not in self.sources:
                raise KeyError(f'skill: no source {name!r} in these reliability sums (have {self.sources})')
        bs, ref = self.by_lead(source)['brier'], self.by_lead(reference)['brier']
        return 1.0 - _ratio(bs, ref)

    def roc(self, source='model'):
        """The ROC per lead time over all clips, from cumulative bin sums: {'thresholds' (K + 1,) = k / K, 'pod' and 'pofd'
        (T_out, K + 1), 'auc' (T_out,) by the trapezoid rule}.  At threshold k / K a pixel is a "yes" iff its bin is >= k,
        i.e. f * K >= k in fp32 (inclusive: a value exactly on an edge belongs to the bin above it), not score()'s strict
        f > threshold.  pod = hits / events, pofd = false alarms / non-events; the curve runs from (1, 1) at k = 0 to (0, 0)
        at k = K.  NaN where a lead time has no event or no non-event."""
        s = self._pooled(source)
        ev, non = s[..., 1], s[..., 0] - s[..., 1]

        def above(c):       # [sum over bins >= k for k = 0..K]
            tail = np.cumsum(c[..., ::-1], axis=-1)[..., ::-1]
            return np.concatenate([tail, np.zeros(c.shape[:-1] + (1,))], axis=-1)
        pod, pofd = _ratio(above(ev), ev.sum(axis=-1, keepdims=True)), _ratio(above(non), non.sum(axis=-1, keepdims=True))
        auc = ((pofd[..., :-1] - pofd[..., 1:]) * (pod[..., :-1] + pod[..., 1:]) / 2.0).sum(axis=-1)
        return {'thresholds': np.arange(self.bins + 1) / self.bins, 'pod': pod, 'pofd': pofd, 'auc': auc}
