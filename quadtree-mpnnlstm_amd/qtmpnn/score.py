"""Forecast verification numbers as NextFramePredictorS2S.score() returns them (numpy only).

The device leaves eight sums per (clip, lead time, source) over the counted pixels (ops.rollout_scores, qt_score_rollout);
everything a user reads is derived from them here, so pooling over clips is pooling of sums, never a mean of ratios.
ScoreMaps holds the same eight sums per pixel, pooled over the clips (ops.rollout_score_maps, qt_score_maps): error maps per
lead time, and sums over a region or weighted by cell area."""
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
    """sums (n_clips, T_out, S, 8) float64 in SLOTS order, sources: S names ('model', then the references').
    Every metric of METRICS is a method metric(source='model') -> (n_clips, T_out); by_lead pools the clips.  maps: the
    ScoreMaps of the same pass, or None."""

    def __init__(self, sums, sources, maps=None):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.sources = tuple(sources)
        self.maps = maps
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


class ScoreMaps:
    """sums (T_out, S, 8, W, H) float64 in SLOTS order: per lead time, source and pixel, summed over every clip of the loader.
    Every metric of METRICS is a method metric(source='model') -> (T_out, W, H); a pixel that no clip counts (masked, no
    node) has n == 0 and NaN ratios.  pooled() sums the pixels, optionally weighted, before the ratios are formed."""

    def __init__(self, sums, sources):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.sources = tuple(sources)
        if self.sums.ndim != 5 or self.sums.shape[1:3] != (len(self.sources), 8):
            raise ValueError(f'ScoreMaps: sums of shape {self.sums.shape} for sources {self.sources}: expected '
                             f'(T_out, {len(self.sources)}, 8, W, H)')

    def _of(self, source):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these maps (have {self.sources})')
        return self.sums[:, self.sources.index(source)]                    # (T_out, 8, W, H)

    def metrics(self, source='model'):
        """{metric: (T_out, W, H)} per lead time and pixel."""
        return derive(np.moveaxis(self._of(source), 1, -1))

    def pooled(self, source='model', weights=None):
        """{metric: (T_out,)} from the sums over the pixels.  weights (W, H) multiplies every slot of a pixel first: cell areas
        (over / under / iiee become areas, n the counted area, rmse area-weighted), a 0/1 region, or their product."""
        s = self._of(source)
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != s.shape[2:]:
                raise ValueError(f'ScoreMaps.pooled: weights of shape {w.shape} for maps of {s.shape[2:]} pixels')
            s = s * w
        return derive(s.sum(axis=(-2, -1)))


for _name in METRICS:
    setattr(Scores, _name, (lambda name: lambda self, source='model': self.metrics(source)[name])(_name))
    setattr(ScoreMaps, _name, (lambda name: lambda self, source='model': self.metrics(source)[name])(_name))
