"""ClipBank: a time series held on the device once, and the training windows formed from it there (beyond the reference, whose
IceDataset materialises every window on the host: consecutive launch dates share all but one day, so every day is stored
T_in + T_out times).  The bank's loader yields what the reference's loaders yield -- (x, y, launch_date) per batch -- so train,
predict, verify and every product take it where they take a DataLoader, unchanged.

No kernel of the library is involved: a batch is one advanced-index gather per field, series[start[:, None] + arange(T)], torch
indexing on device tensors (capturable; DESIGN.md, "ClipBank").  Everything here is pure torch, so device='cpu' works too."""
import numpy as np
import torch
from torch.utils.data import DataLoader


def _whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _channels(name, channels, C):
    if channels is None:
        return list(range(C))
    picked = list(channels)
    if not picked or not all(_whole(c) and 0 <= c < C for c in picked):
        raise ValueError(f'{name}: channel indices must be a non-empty list of integers in 0..{C - 1}, got {picked}')
    return [int(c) for c in picked]


def day_ranges(name, ranges, D):
    """`ranges` as a list of (start, stop) day ranges within 0..D, ordered and without overlap, or a ValueError under `name` (the
    rule of `segments`, which ClipBank.normals(days=) shares)."""
    checked, last = [], 0
    for k, seg in enumerate(tuple(seg) for seg in ranges):
        if len(seg) != 2 or not all(_whole(v) for v in seg):
            raise ValueError(f'{name}: {name}[{k}] must be (start, stop) day numbers, got {seg!r}')
        s, e = int(seg[0]), int(seg[1])
        if not 0 <= s < e <= D:
            raise ValueError(f'{name}: {name}[{k}] = ({s}, {e}) is not a range of days within 0..{D}')
        if s < last:
            raise ValueError(f'{name}: {name}[{k}] = ({s}, {e}) starts before {name}[{k - 1}] stops at day {last} ({name} must '
                             'be ordered and must not overlap)')
        last = e
        checked.append((s, e))
    return checked


def window_table(D, input_timesteps, output_timesteps, segments=None):
    """The first x day of every window, int64 (n,): per segment (s, e) of length L = e - s the windows i, 0 <= i < L - T_in - T_out
    (the reference's `while i + T_out + T_in < size`: the last window that would fit is left out), numbered segment after
    segment.  Window i of a segment has x days [s + i, s + i + T_in), y days [s + i + T_in, s + i + T_in + T_out) and the launch
    date of day s + i + T_in.  ValueErrors by argument name for step counts below 1, segments out of 0..D, unordered or
    overlapping, and for no window at all."""
    for name, T in (('input_timesteps', input_timesteps), ('output_timesteps', output_timesteps)):
        if not _whole(T) or T < 1:
            raise ValueError(f'{name}: must be an integer >= 1, got {T!r}')
    segments = [(0, D)] if segments is None else [tuple(seg) for seg in segments]
    starts = [s + np.arange(max(0, e - s - int(input_timesteps) - int(output_timesteps)), dtype=np.int64)
              for s, e in day_ranges('segments', segments, D)]
    table = np.concatenate(starts) if starts else np.zeros(0, np.int64)
    if not len(table):
        raise ValueError(f'segments: no segment holds a window: {input_timesteps} in + {output_timesteps} out need a segment of more '
                         f'than {input_timesteps + output_timesteps} days, got {segments}')
    return table


class ClipBank:
    """series (D, W, H, C) (numpy or tensor) -> an x series (D, W, H, Cx) and a y series (D, W, H, Cy), float32, contiguous on
    `device`, each day stored once: converted to float32 and passed through nan_to_num once, split by the channel index lists
    (default: all channels); with y_binary_thresh the y series is (y > thresh) as float32, the threshold rounded to float32 and
    compared with the float32 values after nan_to_num.  Normalisation is the caller's (the reference normalises per season,
    before windowing).  times (D,): the day stamps, int64 ns as the reference's launch_dates.astype(int), kept on the host.
    segments: (start, stop) day ranges, one per season, which no window crosses (default: one, (0, D)); see window_table for the
    window rule.  Every argument is checked, by name, before anything is uploaded."""

    def __init__(self, series, times, input_timesteps, output_timesteps, segments=None, x_channels=None, y_channels=None,
                 y_binary_thresh=None, device=None):
        series = torch.as_tensor(series)
        if series.dim() != 4:
            raise ValueError(f'series: must be (D, W, H, C), got {tuple(series.shape)}')
        D, W, H, C = series.shape
        times = np.asarray(times.cpu() if torch.is_tensor(times) else times)
        if times.shape != (D,):
            raise ValueError(f'times: must be ({D},), one stamp per day of the series, got {times.shape}')
        first_day = window_table(D, input_timesteps, output_timesteps, segments)
        self.segments = day_ranges('segments', [(0, D)] if segments is None else [tuple(seg) for seg in segments], D)
        xc, yc = _channels('x_channels', x_channels, C), _channels('y_channels', y_channels, C)
        self.input_timesteps, self.output_timesteps = int(input_timesteps), int(output_timesteps)
        self.device = torch.device('cuda' if device is None else device)
        self.image_shape = (W, H)
        self.times = times.astype(np.int64)
        self.launch_dates = self.times[first_day + self.input_timesteps]
        self._first_day = torch.from_numpy(first_day)
        self._launch = torch.from_numpy(self.launch_dates)

        def stored(channels):           # (one field at a time, selected on the host: the device never holds more than it keeps)
            return torch.nan_to_num_(series[..., channels].to(torch.float32).to(self.device).contiguous())
        self.x, self.y = stored(xc), stored(yc)
        self.device = self.x.device
        if y_binary_thresh is not None:
            self.y = (self.y > float(np.float32(y_binary_thresh))).to(torch.float32)
        self._steps_x = torch.arange(self.input_timesteps, device=self.device)
        self._steps_y = self.input_timesteps + torch.arange(self.output_timesteps, device=self.device)

    def __len__(self):
        return len(self._first_day)

    @property
    def nbytes(self):
        """The device bytes held: D * W * H * (Cx + Cy) * 4."""
        return self.x.numel() * 4 + self.y.numel() * 4

    def window(self, idx):
        """idx: window numbers, a sequence or an int64 tensor (B,) on the host -> (x (B, T_in, W, H, Cx), y (B, T_out, W, H, Cy),
        launch_dates (B,)): x and y contiguous float32 on the bank's device, one gather each; launch_dates int64 on the host (what
        get_climatology_array reads).  The one host-to-device transfer is the windows' first days; nothing waits for the device."""
        idx = torch.as_tensor(idx, dtype=torch.int64, device='cpu').reshape(-1)
        n = len(self)
        if len(idx) and not (int(idx.min()) >= 0 and int(idx.max()) < n):
            raise ValueError(f'idx: window numbers must be in 0..{n - 1}, got {idx.tolist()}')
        first = self._first_day[idx].to(self.device)[:, None]
        return self.x[first + self._steps_x], self.y[first + self._steps_y], self._launch[idx]

    def loader(self, batch_size=1, shuffle=False, generator=None, drop_last=False):
        return ClipLoader(self, batch_size, shuffle, generator, drop_last)

    def normals(self, days=None):
        """The daily normals of the stored y series -> (Cy, 366, W, H) float32 on the bank's device, the layout
        train(climatology=) and get_climatology_array index: entry [c, d] is the mean of channel c over the selected days whose
        stamp has the day-of-year index d (model.utils.day_of_year_index of `times`: 0-based, local time, 365 for 31 December of
        a leap year), and 0 where no selected day has it -- the reference's fillna(0).groupby('time.dayofyear').mean() and
        nan_to_num.  The series is what the bank stores: float32 after nan_to_num, and after y_binary_thresh if one was given.
        days: which days enter, a boolean (D,) selection or a list of (start, stop) ranges checked as `segments` are (default:
        every stored day), so that the test seasons can be left out.
        The sums are float64, taken in ascending day order within every index, divided in float64 and rounded to float32 once:
        round r adds the r-th selected day of every index that has one, each a gather and an indexed add on distinct rows.  No
        atomics, no kernel of the library: two calls give the same bits.  Meant to run once per experiment."""
        from model.utils import day_of_year_index
        D, W, H, Cy = self.y.shape
        picked = self._picked(days)
        index = np.array([day_of_year_index(t) for t in self.times[picked]], dtype=np.int64)
        order = np.argsort(index, kind='stable')                # by index; ascending days within one (picked is ascending)
        index, picked = index[order], picked[order]
        groups, first, count = np.unique(index, return_index=True, return_counts=True)
        sums = torch.zeros(366, W, H, Cy, dtype=torch.float64, device=self.device)
        for r in range(int(count.max())):
            has = count > r
            rows = torch.from_numpy(groups[has]).to(self.device)
            sums[rows] = sums[rows] + self.y[torch.from_numpy(picked[first[has] + r]).to(self.device)].double()
        n = torch.ones(366, dtype=torch.float64)
        n[torch.from_numpy(groups)] = torch.from_numpy(count).double()
        return (sums / n.to(self.device)[:, None, None, None]).to(torch.float32).permute(3, 0, 1, 2).contiguous()

    def _picked(self, days):
        """The stored days that `days` selects, ascending: a boolean (D,) selection, a list of (start, stop) ranges checked as
        `segments` are, or None for every day; a ValueError that names `days` otherwise (normals, anomaly_autocorrelation)."""
        D = self.y.shape[0]
        if days is None:
            picked = np.arange(D)
        elif (torch.is_tensor(days) and days.dtype == torch.bool) or (isinstance(days, np.ndarray) and days.dtype == np.bool_):
            sel = days.cpu().numpy() if torch.is_tensor(days) else days
            if sel.shape != (D,):
                raise ValueError(f'days: a boolean selection must be ({D},), one entry per stored day, got {sel.shape}')
            picked = np.flatnonzero(sel)
        elif isinstance(days, (torch.Tensor, np.ndarray)) or not hasattr(days, '__iter__'):
            raise ValueError(f'days: must be a boolean ({D},) selection or a list of (start, stop) day ranges, got '
                             f'{getattr(days, "dtype", type(days).__name__)}')
        else:
            picked = np.concatenate([np.arange(s, e) for s, e in day_ranges('days', days, D)] + [np.zeros(0, np.int64)])
        if not len(picked):
            raise ValueError('days: no day is selected')
        return picked

    def anomaly_autocorrelation(self, max_lag, days=None, normals=None):
        """The lag autocorrelation of the stored y series' anomalies per pixel -> (Cy, max_lag, W, H) float32 on the bank's
        device; entry [c, k] is that of lag k + 1:

            a[d]    = y[d] - normals[c, day_of_year_index(d)]
            r[c, k] = sum a[d] a[d + lag] / sqrt(sum a[d]^2 * sum a[d + lag]^2),   lag = k + 1

        over the day pairs (d, d + lag) that lie in one segment of the bank and are both selected by `days` (normals()'s
        selection, checked the same way); 0 where the denominator is 0.  normals: (Cy, 366, W, H), default self.normals(days).
        r[0, :T_out] is what qtmpnn.baselines.AnomalyPersistence(damping=) takes.  max_lag: an integer >= 1 and less than the
        number of selected days of the shortest segment that has any.
        The sums are float64 and take the pairs in ascending order of d, every lag at once: one rounded product and one add
        per day, element-wise torch ops (a pair that does not count adds an exact 0), rounded to float32 once.  No atomics, no
        kernel of the library: two calls give the same bits.  Meant to run once per experiment."""
        from model.utils import day_of_year_index
        D, W, H, Cy = self.y.shape
        picked = self._picked(days)
        selected = np.zeros(D, bool)
        selected[picked] = True
        shortest = min(int(selected[s:e].sum()) for s, e in self.segments if selected[s:e].any())
        if not _whole(max_lag) or not 1 <= max_lag < shortest:
            raise ValueError(f'max_lag: must be an integer >= 1 and less than the {shortest} selected days of the shortest segment, '
                             f'got {max_lag!r}')
        L = int(max_lag)
        if normals is None:
            normals = self.normals(days)
        normals = torch.as_tensor(normals).to(self.device, torch.float32)
        if tuple(normals.shape) != (Cy, 366, W, H):
            raise ValueError(f'normals: shape {tuple(normals.shape)}, expected {(Cy, 366, W, H)}')
        index = torch.tensor([day_of_year_index(t) for t in self.times], dtype=torch.int64, device=self.device)
        a = torch.zeros(D + L, W, H, Cy, dtype=torch.float64, device=self.device)          # (zero days past the end: never counted)
        a[:D] = self.y.double() - normals.permute(1, 2, 3, 0)[index].double()
        segment = np.full(D + L, -1)
        for k, (s, e) in enumerate(self.segments):
            segment[s:e] = k
        counts = np.zeros((D, L))
        for k in range(L):
            counts[:D - k - 1, k] = selected[:D - k - 1] & selected[k + 1:] & (segment[:D - k - 1] == segment[k + 1:D])
        counts = torch.from_numpy(counts).to(self.device)[:, :, None, None, None]
        sxy, sxx, syy = (torch.zeros(L, W, H, Cy, dtype=torch.float64, device=self.device) for _ in range(3))
        for d in np.flatnonzero(selected):
            here, there, v = a[d], a[d + 1:d + 1 + L], counts[d]
            sxy += torch.mul(here, there) * v
            sxx += torch.mul(here, here) * v
            syy += torch.mul(there, there) * v
        den = torch.sqrt(sxx * syy)
        r = torch.where(den > 0, sxy / den, torch.zeros_like(den))
        return r.to(torch.float32).permute(3, 0, 1, 2).contiguous()


class ClipLoader:
    """Batches of a ClipBank, re-iterable: bank.window(batch) per batch, `.dataset` the bank (train reads
    loader.dataset.image_shape).  The order of the window numbers IS that of torch.utils.data.DataLoader(dataset_of_len_n,
    batch_size, shuffle, generator=generator, drop_last=drop_last), because such a loader over range(n) draws them: whatever torch
    takes from `generator` -- or, with generator=None, from the global CPU generator -- per pass, this loader takes.  A host
    loader replaced by a bank therefore keeps its sample order, and a run resumed from a checkpoint (which carries the CPU
    generator's state) its bits."""

    def __init__(self, bank, batch_size=1, shuffle=False, generator=None, drop_last=False):
        if not _whole(batch_size) or batch_size < 1:
            raise ValueError(f'batch_size: must be an integer >= 1, got {batch_size!r}')
        self.dataset = bank
        self.batch_size = int(batch_size)
        self._numbers = DataLoader(range(len(bank)), batch_size=self.batch_size, shuffle=bool(shuffle), generator=generator,
                                   drop_last=bool(drop_last))

    def __len__(self):
        return len(self._numbers)

    def __iter__(self):
        for batch in self._numbers:
            yield self.dataset.window(batch)
