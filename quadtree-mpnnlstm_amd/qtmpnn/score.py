"""Forecast verification numbers as NextFramePredictorS2S.score() returns them (numpy only).

The device leaves eight sums per (clip, lead time, source) over the counted pixels (ops.rollout_scores, qt_score_rollout);
everything a user reads is derived from them here, so pooling over clips is pooling of sums, never a mean of ratios."""
import numpy as np

SLOTS = ('n', 'sum_d', 'sum_abs_d', 'sum_sq_d', 'hits', 'over', 'under', 'correct_negatives')
METRICS = ('n', 'bias', 'mae', 'rmse', 'accuracy', 'over', 'under', 'iiee')


def derive(sums):
    """{metric: array} from sums (..., 8).  bias / mae / rmse / accuracy are ratios over n and NaN where n == 0; over (false
    alarms), under (misses) and iiee = over + under are pixel counts."""
    s = np.asarray(sums, dtype=np.float64)
    n, sd, sa, sq, hits, over, under, cn = (s[..., k] for k in range(8))
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'n': n, 'bias': sd / n, 'mae': sa / n, 'rmse': np.sqrt(sq / n), 'accuracy': (hits + cn) / n,
                'over': over, 'under': under, 'iiee': over + under}


class Scores:
    """sums (n_clips, T_out, S, 8) float64 in SLOTS order, sources: S names ('model', 'persistence', 'climatology').
    Every metric of METRICS is a method metric(source='model') -> (n_clips, T_out); by_lead pools the clips."""

    def __init__(self, sums, sources):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.sources = tuple(sources)
        if self.sums.ndim != 4 or self.sums.shape[2:] != (len(self.sources), 8):
            raise ValueError(f'sums of shape {self.sums.shape} for sources {self.sources}: expected (n_clips, T_out, {len(self.sources)}, 8)')

    def _of(self, source):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these scores (have {self.sources})')
        return self.sums[:, :, self.sources.index(source)]

    def metrics(self, source='model'):
        """{metric: (n_clips, T_out)} per launch date and lead time."""
        return derive(self._of(source))

    def by_lead(self, source='model'):
        """{metric: (T_out,)} over all clips, from the pooled sums (rmse = sqrt(sum of SSE / sum of n))."""
        return derive(self._of(source).sum(axis=0))


for _name in METRICS:
    setattr(Scores, _name, (lambda name: lambda self, source='model': self.metrics(source)[name])(_name))
