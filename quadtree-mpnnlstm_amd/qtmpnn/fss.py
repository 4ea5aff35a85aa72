"""Neighbourhood verification numbers as NextFramePredictorS2S.fss() returns them (numpy only).

The device leaves five integers per (clip, lead time, source, scale) over the counted pixels (ops.rollout_fss, qt_fss_rollout):
with c_s and c_o the numbers of forecast and observed ice pixels in the scale's window around a pixel, [n, events,
sum (c_s - c_o)^2, sum c_s^2, sum c_o^2].  The Fractions Skill Score (Roberts & Lean 2008) is 1 - sum (c_s - c_o)^2 /
(sum c_s^2 + sum c_o^2): the window's area, which turns a count into a fraction, cancels.  Everything a user reads is derived
from those sums here, and clips are pooled by summing their sums first, as qtmpnn.score.Scores does: never a mean of ratios."""
import numpy as np

SLOTS = ('n', 'events', 'sum_sq_diff', 'sum_sq_f', 'sum_sq_o')


def _ratio(a, b):
    """a / b, NaN where b == 0, without a warning."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _fss(s):
    """FSS of (..., 5) sums: NaN where neither field has ice (denominator 0)."""
    return 1.0 - _ratio(s[..., 2], s[..., 3] + s[..., 4])


class FSS:
    """sums (n_clips, T_out, S, K, 5) int64 in SLOTS order: per scale the counted pixels n, the observed events
    (y > threshold) among them, and the three sums of squares of the window counts.  sources: S names ('model', then the
    references'); threshold: the one that defined ice; scales: the K odd window sizes, increasing."""

    def __init__(self, sums, sources, threshold, scales):
        sums = np.asarray(sums)
        self.sources = tuple(sources)
        self.threshold = float(threshold)
        self.scales = tuple(int(v) for v in scales)
        if sums.ndim != 5 or sums.shape[2] != len(self.sources) or sums.shape[3] != len(self.scales) or sums.shape[4] != 5:
            raise ValueError(f'FSS: sums of shape {sums.shape} for sources {self.sources} and scales {self.scales}: expected '
                             f'(n_clips, T_out, {len(self.sources)}, {len(self.scales)}, 5)')
        if not np.issubdtype(sums.dtype, np.integer):
            raise ValueError(f'FSS: sums must be integers, got {sums.dtype}')
        if not self.sources or len(set(self.sources)) != len(self.sources):
            raise ValueError(f'FSS: sources must be distinct names, got {self.sources}')
        if (not 1 <= len(self.scales) <= 8 or any(v % 2 == 0 or not 1 <= v <= 33 for v in self.scales)
                or any(b <= a for a, b in zip(self.scales, self.scales[1:]))):
            raise ValueError(f'FSS: scales must be 1..8 odd window sizes in 1..33, strictly increasing, got {self.scales}')
        self.sums = sums.astype(np.int64)

    def _of(self, source):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these FSS sums (have {self.sources})')
        return self.sums[:, :, self.sources.index(source)]                 # (n_clips, T_out, K, 5)

    def fss(self, source='model'):
        """Fractions Skill Score (n_clips, T_out, K) per launch date, lead time and scale; NaN where neither the forecast nor
        the truth has ice in any window."""
        return _fss(self._of(source))

    def by_lead(self, source='model'):
        """Over all clips, from the pooled sums: {'n' (T_out,) counted pixels, 'base_rate' (T_out,) = events / n, 'fss'
        (T_out, K), 'useful' (T_out,) = 0.5 + base_rate / 2 (the score of a forecast with the observed fraction everywhere is
        base_rate, of a perfect one 1: halfway is the customary "useful" level), 'useful_scale' (T_out,): the smallest scale
        with fss >= useful, NaN if there is none}."""
        s = self._of(source).sum(axis=0)                                   # (T_out, K, 5)
        n, base = s[:, 0, 0].astype(np.float64), _ratio(s[:, 0, 1], s[:, 0, 0])
        fss = _fss(s)
        useful = 0.5 + base / 2.0
        with np.errstate(invalid='ignore'):
            ok = fss >= useful[:, None]                                    # NaN compares false
        scale = np.where(ok.any(axis=1), np.asarray(self.scales, dtype=np.float64)[ok.argmax(axis=1)], np.nan)
        return {'n': n, 'base_rate': base, 'fss': fss, 'useful': useful, 'useful_scale': scale}

    def skill(self, source='model', reference='persistence'):
        """FSS(source) - FSS(reference), (T_out, K) over all clips: positive where the source places the ice better than the
        reference at that lead time and scale; NaN where either score is."""
        for name in (source, reference):
            if name not in self.sources:
                raise KeyError(f'skill: no source {name!r} in these FSS sums (have {self.sources})')
        return self.by_lead(source)['fss'] - self.by_lead(reference)['fss']
