"""Sea-ice extent, sea-ice area and the integrated ice-edge error as NextFramePredictorS2S.extent() returns them (numpy only).

The device leaves, per (clip, lead time, region), one row of four sums for the truth and one per source over the region's
counted pixels with weight a (ops.rollout_extent, qt_extent_rollout; I = value > threshold, strict):
    row 0      [n, A = sum a, E_o = sum a I_o, SIA_o = sum a y]
    row 1 + s  [E_s = sum a I_s, SIA_s = sum a f_s, O_s = sum a I_s (1 - I_o), U_s = sum a (1 - I_s) I_o]
Everything a user reads is derived from those sums here.  The integrated ice-edge error and its decomposition (Goessling et al.
2016) are IIEE = O + U, the absolute extent error AEE = |O - U| and the misplacement error ME = 2 min(O, U); AEE and ME are not
linear in the sums, so they are formed per forecast (clip, lead time, region) and averaged afterwards, never from pooled sums."""
import numpy as np

TRUTH_SLOTS = ('n', 'total_area', 'extent', 'area')
SOURCE_SLOTS = ('extent', 'area', 'over', 'under')
OBSERVED = 'observed'


def _ratio(a, b):
    """a / b, NaN where b == 0, without a warning."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


class Extent:
    """sums (n_clips, T_out, R, 1 + S, 4) float64: row 0 in TRUTH_SLOTS order, row 1 + s of source s in SOURCE_SLOTS order, in
    the unit of the areas the call was given (pixels without them).  sources: S names ('model', then the references');
    where a method takes a source, 'observed' is one too (the truth: its errors are zero).  threshold: the one that separates ice
    from no ice; region_names: R names (default 'region0' ...)."""

    def __init__(self, sums, sources, threshold, region_names=None):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.sources = tuple(sources)
        self.threshold = float(threshold)
        if self.sums.ndim != 5 or self.sums.shape[3] != 1 + len(self.sources) or self.sums.shape[4] != 4:
            raise ValueError(f'Extent: sums of shape {self.sums.shape} for sources {self.sources}: expected '
                             f'(n_clips, T_out, regions, {1 + len(self.sources)}, 4)')
        if not self.sources or len(set(self.sources)) != len(self.sources) or OBSERVED in self.sources:
            raise ValueError(f'Extent: sources must be distinct names other than {OBSERVED!r}, got {self.sources}')
        R = self.sums.shape[2]
        self.region_names = tuple(f'region{r}' for r in range(R)) if region_names is None else tuple(region_names)
        if R < 1 or len(self.region_names) != R or len(set(self.region_names)) != R:
            raise ValueError(f'Extent: region_names must be {R} distinct names (sums of shape {self.sums.shape}), got '
                             f'{self.region_names}')

    def _row(self, source):
        """(n_clips, T_out, R, 4): the source's row, or for 'observed' the truth's as a forecast of itself [E_o, SIA_o, 0, 0]."""
        if source == OBSERVED:
            t = self.sums[:, :, :, 0]
            return np.stack([t[..., 2], t[..., 3], np.zeros_like(t[..., 0]), np.zeros_like(t[..., 0])], axis=-1)
        if source not in self.sources:
            raise KeyError(f'no source {source!r} in these extent sums (have {(OBSERVED,) + self.sources})')
        return self.sums[:, :, :, 1 + self.sources.index(source)]

    def _region(self, region):
        if isinstance(region, str):
            if region not in self.region_names:
                raise KeyError(f'no region {region!r} in these extent sums (have {self.region_names})')
            return self.region_names.index(region)
        if isinstance(region, (bool, np.bool_)) or not isinstance(region, (int, np.integer)) \
                or not 0 <= region < len(self.region_names):
            raise KeyError(f'no region {region!r} in these extent sums (have {len(self.region_names)}: {self.region_names})')
        return int(region)

    def n(self):
        """Counted pixels (n_clips, T_out, R)."""
        return self.sums[:, :, :, 0, 0]

    def total_area(self):
        """A: the area of the counted pixels (n_clips, T_out, R)."""
        return self.sums[:, :, :, 0, 1]

    def extent(self, source='model'):
        """Sea-ice extent (n_clips, T_out, R): the area of the counted pixels whose value is above the threshold."""
        return self._row(source)[..., 0]

    def area(self, source='model'):
        """Sea-ice area (n_clips, T_out, R): the area-weighted sum of the values (concentrations) of the counted pixels."""
        return self._row(source)[..., 1]

    def over(self, source='model'):
        """O: the area forecast as ice that is observed as no ice (n_clips, T_out, R)."""
        return self._row(source)[..., 2]

    def under(self, source='model'):
        """U: the area observed as ice that is forecast as no ice (n_clips, T_out, R)."""
        return self._row(source)[..., 3]

    def iiee(self, source='model'):
        """Integrated ice-edge error O + U per clip, lead time and region."""
        return self.over(source) + self.under(source)

    def aee(self, source='model'):
        """Absolute extent error |O - U| per clip, lead time and region (= |forecast extent - observed extent|)."""
        return np.abs(self.over(source) - self.under(source))

    def me(self, source='model'):
        """Misplacement error 2 min(O, U) per clip, lead time and region; IIEE = AEE + ME."""
        return 2.0 * np.minimum(self.over(source), self.under(source))

    def error(self, source='model', what='extent'):
        """Forecast minus observed, (n_clips, T_out, R), of the extent (what='extent') or the ice area ('area')."""
        if what not in ('extent', 'area'):
            raise ValueError(f"error: what must be 'extent' or 'area', got {what!r}")
        k = 0 if what == 'extent' else 1
        return self._row(source)[..., k] - self._row(OBSERVED)[..., k]

    def total(self):
        """The Extent of one region 'total': the regions' sums added (per clip and lead time, before anything is derived)."""
        return Extent(self.sums.sum(axis=2, keepdims=True), self.sources, self.threshold, ('total',))

    def by_lead(self, source='model', region=None):
        """{name: (T_out,)} over the clips for one region (an index or a name; None: all regions added first, per clip, before
        AEE and ME are formed): 'n_clips'; 'observed_extent', 'forecast_extent' (means), 'extent_bias', 'extent_mae',
        'extent_rmse' of the extent error; 'observed_area', 'forecast_area', 'area_bias', 'area_mae', 'area_rmse' likewise for
        the ice area; 'iiee', 'aee', 'me' (means over the clips of the per-clip values)."""
        self._row(source)
        one = self.total() if region is None else self
        r = 0 if region is None else self._region(region)
        out = {'n_clips': np.full(self.sums.shape[1], self.sums.shape[0])}
        mean = lambda v: v.mean(axis=0) if len(v) else np.full(v.shape[1:], np.nan)
        for what in ('extent', 'area'):
            k = 0 if what == 'extent' else 1
            err = one.error(source, what)[:, :, r]
            out[f'observed_{what}'] = mean(one._row(OBSERVED)[:, :, r, k])
            out[f'forecast_{what}'] = mean(one._row(source)[:, :, r, k])
            out[f'{what}_bias'], out[f'{what}_mae'], out[f'{what}_rmse'] = mean(err), mean(np.abs(err)), np.sqrt(mean(err * err))
        out['iiee'], out['aee'], out['me'] = (mean(f(source)[:, :, r]) for f in (one.iiee, one.aee, one.me))
        return out

    def skill(self, source='model', reference='persistence', metric='iiee'):
        """1 - mean(metric of source) / mean(metric of reference) per lead time (T_out,), the means over the clips of the
        metric ('iiee', 'aee' or 'me') of all regions added; NaN where the reference's mean is 0."""
        if metric not in ('iiee', 'aee', 'me'):
            raise ValueError(f"skill: metric must be 'iiee', 'aee' or 'me', got {metric!r}")
        for name in (source, reference):
            if name != OBSERVED and name not in self.sources:
                raise KeyError(f'skill: no source {name!r} in these extent sums (have {(OBSERVED,) + self.sources})')
        return 1.0 - _ratio(self.by_lead(source)[metric], self.by_lead(reference)[metric])

    def concentration(self, source='model'):
        """Mean concentration of a region, ice area / total area (n_clips, T_out, R); NaN for a region without a counted pixel."""
        return _ratio(self.area(source), self.total_area())
