"""The window rule of qtmpnn.data.ClipBank restated in numpy with plain loops: every window materialised, one by one, as a host
dataset holds them.  The yardstick of tests/test_clipbank_host.py and tests/test_gpu_clipbank.py -- not the code under test."""
import numpy as np
import torch


def restated_windows(series, times, T_in, T_out, segments=None, x_channels=None, y_channels=None, y_binary_thresh=None):
    """-> x (n, T_in, W, H, Cx) float32, y (n, T_out, W, H, Cy) float32, launch_dates (n,) int64, first_days (list).
    Per segment of length L, window i exists while i + T_out + T_in < L; its x days are the T_in days from s + i, its y days the
    T_out days after them, its launch date the stamp of its first y day.  The series is float32 after nan_to_num; a binary y is
    1.0 where that float32 value is above the threshold (itself taken as a float32)."""
    series = np.nan_to_num(np.asarray(series).astype(np.float32))
    D, W, H, C = series.shape
    segments = [(0, D)] if segments is None else segments
    x_channels = list(range(C)) if x_channels is None else x_channels
    y_channels = list(range(C)) if y_channels is None else y_channels
    xs, ys, dates, first_days = [], [], [], []
    for s, e in segments:
        size = e - s
        i = 0
        while i + T_out + T_in < size:
            x = np.zeros((T_in, W, H, len(x_channels)), np.float32)
            y = np.zeros((T_out, W, H, len(y_channels)), np.float32)
            for t in range(T_in):
                for k, c in enumerate(x_channels):
                    x[t, :, :, k] = series[s + i + t, :, :, c]
            for t in range(T_out):
                for k, c in enumerate(y_channels):
                    day = series[s + i + T_in + t, :, :, c]
                    y[t, :, :, k] = day if y_binary_thresh is None else np.where(day > np.float32(y_binary_thresh), 1.0, 0.0)
            xs.append(x)
            ys.append(y)
            dates.append(int(np.asarray(times)[s + i + T_in]))
            first_days.append(s + i)
            i += 1
    return np.stack(xs), np.stack(ys), np.array(dates, dtype=np.int64), first_days


class RestatedDataset(torch.utils.data.Dataset):
    """The materialised windows as the reference's dataset serves them: items (x, y, launch_date), `.image_shape`."""

    def __init__(self, *args, **kwargs):
        self.x, self.y, self.launch_dates, self.first_days = restated_windows(*args, **kwargs)
        self.image_shape = self.x.shape[2:4]

    def __len__(self):
        return len(self.y)

    def __getitem__(self, idx):
        return self.x[idx], self.y[idx], self.launch_dates[idx]
