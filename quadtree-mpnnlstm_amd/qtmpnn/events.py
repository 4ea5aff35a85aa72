"""Break-up / freeze-up dates as NextFramePredictorS2S.event_dates() returns them (numpy only).

The device leaves one date per (clip, source, pixel) and eight integer sums per (clip, forecast source) over the counted
pixels (ops.rollout_event_dates: qt_event_scan, qt_event_sums); everything a user reads is derived from them here, so pooling
over clips is pooling of sums, never a mean of ratios.

Date codes: >= 0 the 0-based output step of the event (launch date + that many days, as get_climatology_array counts), -1 no
event (already in the target state at launch, or no run of `persist` steps completes within the rollout), -2 not counted
(masked, or without a node at some step)."""
import numpy as np

SLOTS = ('n', 'sum_e', 'sum_abs_e', 'sum_sq_e', 'hits', 'false_alarms', 'misses', 'neither')
METRICS = ('n', 'bias', 'mae', 'rmse', 'hit_rate', 'false_alarm_ratio', 'hits', 'false_alarms', 'misses')
KINDS = ('breakup', 'freezeup')
NO_EVENT, NOT_COUNTED = -1, -2


def derive(sums):
    """{metric: array} from sums (..., 8).  bias / mae / rmse are in days over the hits (e = forecast date - observed date),
    hit_rate = hits / (hits + misses), false_alarm_ratio = false alarms / (hits + false alarms); NaN where the denominator
    is 0.  n, hits, false_alarms and misses are pixel counts."""
    s = np.asarray(sums, dtype=np.float64)
    if s.shape[-1:] != (8,):
        raise ValueError(f'derive: sums of shape {s.shape}: the last axis must hold the 8 slots {SLOTS}')
    n, se, sa, sq, hits, fa, miss, _ = (s[..., k] for k in range(8))
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'n': n, 'bias': se / hits, 'mae': sa / hits, 'rmse': np.sqrt(sq / hits), 'hit_rate': hits / (hits + miss),
                'false_alarm_ratio': fa / (hits + fa), 'hits': hits, 'false_alarms': fa, 'misses': miss}


class EventDates:
    """dates (n_clips, S1, W, H) int32 in the codes above; sums (n_clips, S1 - 1, 8) int64 in SLOTS order, one row per
    forecast source; sources: S1 names, 'observed' first, then 'model' and the references' names (by default 'climatology', when
    given)."""

    def __init__(self, dates, sums, sources, kind, persist, threshold):
        self.dates = np.asarray(dates)
        self.sums = np.asarray(sums)
        self.sources = tuple(sources)
        self.kind, self.persist, self.threshold = kind, persist, threshold
        S1 = len(self.sources)
        if S1 < 2 or self.sources[0] != 'observed':
            raise ValueError(f'EventDates: sources {self.sources}: expected \'observed\' followed by the forecast sources')
        if self.dates.ndim != 4 or self.dates.shape[1] != S1 or self.dates.dtype.kind != 'i':
            raise ValueError(f'EventDates: dates of shape {self.dates.shape} and type {self.dates.dtype} for sources '
                             f'{self.sources}: expected integers (n_clips, {S1}, W, H)')
        if self.sums.shape != (self.dates.shape[0], S1 - 1, 8) or self.sums.dtype.kind != 'i':
            raise ValueError(f'EventDates: sums of shape {self.sums.shape} and type {self.sums.dtype} for '
                             f'{self.dates.shape[0]} clip(s) and sources {self.sources}: expected integers '
                             f'({self.dates.shape[0]}, {S1 - 1}, 8)')
        if kind not in KINDS:
            raise ValueError(f'EventDates: kind must be one of {KINDS}, got {kind!r}')
        if persist < 1:
            raise ValueError(f'EventDates: persist must be >= 1, got {persist!r}')
        self.dates = self.dates.astype(np.int32, copy=False)
        self.sums = self.sums.astype(np.int64, copy=False)

    def _index(self, source, forecast):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these event dates (have {self.sources})')
        if forecast and source == 'observed':
            raise KeyError(f'\'observed\' is what the forecast sources {self.sources[1:]} are compared with: it has no errors')
        return self.sources.index(source)

    def date(self, source='model'):
        """(n_clips, W, H) int32 dates of one source ('observed' included)."""
        return self.dates[:, self._index(source, False)]

    def metrics(self, source='model'):
        """{metric: (n_clips,)} per launch date."""
        return derive(self.sums[:, self._index(source, True) - 1])

    def pooled(self, source='model'):
        """{metric: scalar array} over all clips, from the summed sums."""
        return derive(self.sums[:, self._index(source, True) - 1].sum(axis=0))

    def error_map(self, source='model'):
        """(W, H) mean of e = date - observed date over the clips in which both have an event at the pixel; NaN where
        none has."""
        f, o = self.dates[:, self._index(source, True)].astype(np.int64), self.dates[:, 0].astype(np.int64)
        both = (f >= 0) & (o >= 0)
        cnt = both.sum(axis=0)
        tot = np.where(both, f - o, 0).sum(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(cnt > 0, tot / cnt, np.nan)


for _name in METRICS:
    setattr(EventDates, _name, (lambda name: lambda self, source='model': self.metrics(source)[name])(_name))
