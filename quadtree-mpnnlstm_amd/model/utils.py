"""Helpers of the reference's model/utils.py that the hot path and its callers use."""
import datetime

import numpy as np
import torch

_PE_CACHE = {}


def positional_grid(w, h, device=None, dtype=torch.float32):
    """(w, h, 2) grid: channel 0 = column / h, channel 1 = row / w (model/utils.py:37-45).
    Constant per image shape, so it is built once per (shape, device) instead of on every call."""
    key = (w, h, str(device), dtype)
    if key not in _PE_CACHE:
        g = np.empty((w, h, 2), dtype=np.float64)
        g[..., 0] = (np.arange(h, dtype=np.float64) / h)[None, :]
        g[..., 1] = (np.arange(w, dtype=np.float64) / w)[:, None]
        _PE_CACHE[key] = torch.from_numpy(g).to(dtype).to(device)
    return _PE_CACHE[key]


def add_positional_encoding(x):
    """(n_samples, w, h, c) -> (n_samples, w, h, c + 2), tensors or arrays (model/utils.py:30-52)."""
    assert len(x.shape) == 4, f'array should be 4-dimensional (n_samples, w, h, c); got {x.shape}'
    n, w, h, _ = x.shape
    if isinstance(x, torch.Tensor):
        pe = positional_grid(w, h, x.device, x.dtype)
        return torch.cat((x, pe.unsqueeze(0).expand(n, w, h, 2)), dim=-1)
    pe = positional_grid(w, h).numpy().astype(x.dtype)
    return np.concatenate((x, np.broadcast_to(pe, (n, w, h, 2))), axis=-1)


def cell_area_weights(latitudes, n_lon):
    """Relative cell areas of a regular latitude-longitude grid (beyond the reference): cos(latitude in degrees), one row per
    latitude, repeated over n_lon columns and scaled to mean 1; float32 (len(latitudes), n_lon).  The map to pass as
    `loss_weights` to the trainer and as `weights` to ScoreMaps.pooled."""
    lat = np.asarray(latitudes, dtype=np.float64).reshape(-1)
    if lat.size == 0 or int(n_lon) < 1:
        raise ValueError(f'latitudes / n_lon: an empty grid ({lat.size} x {n_lon})')
    if not np.isfinite(lat).all() or (np.abs(lat) > 90).any():
        raise ValueError('latitudes: degrees in [-90, 90] are needed')
    c = np.where(np.abs(lat) < 90, np.cos(np.deg2rad(lat)), 0.0)        # (cos(pi / 2) is 6e-17 in float64: a pole has no area)
    if not c.sum() > 0:
        raise ValueError('latitudes: every row lies at a pole (all areas are 0)')
    return np.repeat((c / c.mean())[:, None], int(n_lon), axis=1).astype(np.float32)


def get_n_params(model):
    """Number of parameters of a torch module (model/utils.py:19-27)."""
    return sum(p.numel() for p in model.parameters())


def normalize(arr):
    """Per-variable min-max scaling over axes (0, 2, 3, 4) (model/utils.py:70-73)."""
    lo = np.min(arr, (0, 2, 3, 4))[:, None, None, None]
    hi = np.max(arr, (0, 2, 3, 4))[:, None, None, None]
    return (arr - lo) / (hi - lo)


def int_to_datetime(x):
    """Nanosecond timestamp -> datetime (model/utils.py:75-76)."""
    return datetime.datetime.fromtimestamp(x / 1e9)


def day_of_year_index(stamp):
    """Nanosecond timestamp (int or float) -> 0-based day of the year, 0..365, in local time: the index of the daily normals
    (mpnnlstm.py:393).  The one statement of the rule: get_climatology_array and ClipBank.normals both come here."""
    return int_to_datetime(stamp).timetuple().tm_yday - 1


def output_day_indices(launch, output_timesteps):
    """The day-of-year indices of the output days of a clip launched at `launch` (int64 ns): day t is launch + 8.640e13 * t, a
    float64 addition as in the reference (mpnnlstm.py:391-394)."""
    return [day_of_year_index(launch + 8.640e13 * t) for t in range(output_timesteps)]


def launch_day_index(launch):
    """The day-of-year index of the launch-state day of a clip launched at `launch` (int64 ns): the calendar day before the first
    output day, launch - 8.640e13 in the float64 arithmetic of output_day_indices, by the same rule (31 December of a leap year
    is 365; a 1 January launch reads the previous year's 31 December).  It is the day of the last input frame, whose anomaly
    the anomaly-persistence reference carries (qtmpnn.baselines)."""
    return day_of_year_index(launch - 8.640e13)


def round_to_day(dt):
    return datetime.datetime(*dt.timetuple()[:3])
