"""Ice-edge distances as NextFramePredictorS2S.edge_distance() returns them (numpy only).

The device leaves eight integers per (clip, lead time, source) (ops.rollout_edges, qt_edge_rollout).  With E(f) and E(y) the edge
sets of the forecast and of the truth (ice pixels with an open-water 4-neighbour), d2(p, E) the squared pixel distance from p to
the nearest pixel of E and q = isqrt(65536 d2) that distance in 1/256 pixel: [n_f = |E(f)|, n_o = |E(y)|, sum_q_fo, sum_q_of,
sum_d2_fo, sum_d2_of, max_d2_fo, max_d2_of], `fo` over p in E(f) against E(y), `of` over p in E(y) against E(f).  Everything a
user reads is derived from those sums here (Dukhovskoy et al. 2015; Melsom et al. 2019), in pixels, and clips are pooled by
summing their sums first, as qtmpnn.score.Scores does: never a mean of ratios."""
import numpy as np

SLOTS = ('n_f', 'n_o', 'sum_q_fo', 'sum_q_of', 'sum_d2_fo', 'sum_d2_of', 'max_d2_fo', 'max_d2_of')
Q = 256.0           # q counts 1/256 pixel


def _ratio(a, b):
    """a / b, NaN where b == 0, without a warning."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _distances(s, defined):
    """The four distances of (..., 8) sums in pixels, NaN where `defined` (both edge sets non-empty) is false."""
    fo, of = _ratio(s[..., 2], s[..., 0]) / Q, _ratio(s[..., 3], s[..., 1]) / Q          # the two directed mean distances
    out = {'displacement': (fo + of) / 2.0,
           'modified_hausdorff': np.maximum(fo, of),
           'hausdorff': np.sqrt(np.maximum(s[..., 6], s[..., 7]).astype(np.float64)),
           'rms': np.sqrt(_ratio(s[..., 4] + s[..., 5], s[..., 0] + s[..., 1]))}
    return {k: np.where(defined, v, np.nan) for k, v in out.items()}


class EdgeDistance:
    """sums (n_clips, T_out, S, 8) int64 in SLOTS order.  sources: S names ('model', then the references'); threshold:
    the one that defined ice.  All distances are in pixels."""

    def __init__(self, sums, sources, threshold):
        sums = np.asarray(sums)
        self.sources = tuple(sources)
        self.threshold = float(threshold)
        if sums.ndim != 4 or sums.shape[2] != len(self.sources) or sums.shape[3] != 8:
            raise ValueError(f'EdgeDistance: sums of shape {sums.shape} for sources {self.sources}: expected '
                             f'(n_clips, T_out, {len(self.sources)}, 8)')
        if not np.issubdtype(sums.dtype, np.integer):
            raise ValueError(f'EdgeDistance: sums must be integers, got {sums.dtype}')
        if not self.sources or len(set(self.sources)) != len(self.sources):
            raise ValueError(f'EdgeDistance: sources must be distinct names, got {self.sources}')
        self.sums = sums.astype(np.int64)

    def _of(self, source):
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these edge sums (have {self.sources})')
        return self.sums[:, :, self.sources.index(source)]                 # (n_clips, T_out, 8)

    def _per_clip(self, source, which):
        s = self._of(source)
        return _distances(s, (s[..., 0] > 0) & (s[..., 1] > 0))[which]

    def displacement(self, source='model'):
        """Average ice-edge displacement (n_clips, T_out): the mean of the two directed mean distances, forecast edge to observed
        edge and back, (sum_q_fo / n_f + sum_q_of / n_o) / 2 / 256.  NaN where either field has no edge."""
        return self._per_clip(source, 'displacement')

    def modified_hausdorff(self, source='model'):
        """Modified Hausdorff distance (n_clips, T_out): the larger of the two directed mean distances.  NaN where either field
        has no edge."""
        return self._per_clip(source, 'modified_hausdorff')

    def hausdorff(self, source='model'):
        """Hausdorff distance (n_clips, T_out): sqrt(max(max_d2_fo, max_d2_of)), the farthest any edge pixel lies from the other
        edge.  NaN where either field has no edge."""
        return self._per_clip(source, 'hausdorff')

    def rms(self, source='model'):
        """Root-mean-square edge distance (n_clips, T_out): sqrt((sum_d2_fo + sum_d2_of) / (n_f + n_o)).  NaN where either field
        has no edge."""
        return self._per_clip(source, 'rms')

    def by_lead(self, source='model', pixel_km=None):
        """Over all clips, from the pooled sums (the max slots pooled as maxima): {'n_defined' (T_out,) the (clip, lead) pairs
        with both edge sets non-empty, which are the only ones pooled; 'edge_length' (T_out,) mean n_o over them;
        'displacement', 'modified_hausdorff', 'hausdorff', 'rms' (T_out,)}, NaN where n_defined is 0.  The four distances are in
        pixels, or multiplied by `pixel_km` when it is given."""
        s = self._of(source)
        ok = (s[..., 0] > 0) & (s[..., 1] > 0)                             # (n_clips, T_out)
        kept = np.where(ok[..., None], s, 0)
        pooled = np.concatenate([kept[..., :6].sum(axis=0), kept[..., 6:].max(axis=0, initial=0)], axis=-1)
        n_defined = ok.sum(axis=0)
        out = {'n_defined': n_defined, 'edge_length': _ratio(pooled[:, 1], n_defined)}
        scale = 1.0 if pixel_km is None else float(pixel_km)
        for k, v in _distances(pooled, n_defined > 0).items():
            out[k] = v * scale
        return out

    def skill(self, source='model', reference='persistence'):
        """1 - D(source) / D(reference), (T_out,), D the pooled average ice-edge displacement: positive where the source's edge
        lies closer to the observed one than the reference's; NaN where either is undefined or the reference's is 0."""
        for name in (source, reference):
            if name not in self.sources:
                raise KeyError(f'skill: no source {name!r} in these edge sums (have {self.sources})')
        return 1.0 - _ratio(self.by_lead(source)['displacement'], self.by_lead(reference)['displacement'])
