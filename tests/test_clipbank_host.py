"""qtmpnn.data.ClipBank without a GPU (a CPU bank): the windows against the plain-loop restatement, the batch order against a torch
DataLoader, the sizes, and every refusal by argument name.  Nothing here may reach the library: _lib.call fails."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from clipbank_restated import RestatedDataset, restated_windows

@pytest.fixture(autouse=True)
def no_launch(monkeypatch):
    from qtmpnn import _lib

    def fail(*a):
        raise AssertionError(f'ClipBank launched {a[0]}')
    monkeypatch.setattr(_lib, 'call', fail)


def _series(D=30, shape=(5, 7), C=3, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    series = rng.random((D, *shape, C)).astype(dtype)
    times = (np.datetime64('2011-02-20T12', 'ns') + np.arange(D) * np.timedelta64(1, 'D')).astype(np.int64)
    return series, times


def _nans(series):
    series = series.copy()
    series[2, 1, 3, 0] = np.nan
    series[7, :, 0, 1] = np.nan
    series[9, 0, 0, 2] = np.inf
    series[11, 4, 6, 0] = -np.inf
    return series


CASES = {
    'one_segment': dict(T=(3, 4), kw={}),
    'two_segments_gap': dict(T=(3, 4), kw=dict(segments=[(0, 12), (15, 30)])),
    'short_segment': dict(T=(3, 4), kw=dict(segments=[(0, 10), (10, 17), (17, 30)])),        # 7 days: `i + 7 < 7` never holds
    'channels': dict(T=(2, 5), kw=dict(x_channels=[2, 0], y_channels=[1])),
    'binary': dict(T=(3, 4), kw=dict(y_channels=[0], y_binary_thresh=0.3)),
    'nans': dict(T=(4, 2), kw=dict(segments=[(0, 14), (14, 30)]), prepare=_nans),
    'one_in_one_out': dict(T=(1, 1), kw=dict(segments=[(3, 6)])),
}


@pytest.mark.parametrize('name', list(CASES))
def test_windows_equal_the_restatement(name):
    from qtmpnn.data import ClipBank, window_table
    case = CASES[name]
    series, times = _series()
    series = case.get('prepare', lambda s: s)(series)
    if name == 'binary':                    # values AT the float32 threshold: not above it (in float64 they would be)
        series[5, :, :, 0] = np.float32(0.3)
    T_in, T_out = case['T']
    x, y, dates, first_days = restated_windows(series, times, T_in, T_out, **case['kw'])
    bank = ClipBank(series, times, T_in, T_out, device='cpu', **case['kw'])
    n = len(first_days)
    assert len(bank) == n and window_table(len(series), T_in, T_out, case['kw'].get('segments')).tolist() == first_days
    assert bank.image_shape == (5, 7)
    assert bank.launch_dates.dtype == np.int64 and np.array_equal(bank.launch_dates, dates)
    bx, by, bd = bank.window(range(n))
    assert bx.dtype == by.dtype == torch.float32 and bx.is_contiguous() and by.is_contiguous()
    assert bd.dtype == torch.int64 and bd.device.type == 'cpu' and bd.shape == (n,)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    assert torch.equal(bx, torch.from_numpy(x)) and torch.equal(by, torch.from_numpy(y)) and torch.equal(bd, torch.from_numpy(dates))
    if name == 'binary':
        assert set(np.unique(y)) == {0.0, 1.0} and bank.y[5].eq(0).all() and set(bank.y.unique().tolist()) == {0.0, 1.0}
    if name == 'short_segment':
        assert n == 3 + 0 + 6
    if name == 'one_segment':
        assert n == 30 - 3 - 4              # the last window that would fit (first day 23) is left out, as in the reference
    # any order, repeats, a tensor of numbers, one number
    pick = torch.tensor([n - 1, 0, n - 1], dtype=torch.int64)
    px, py, pd = bank.window(pick)
    assert torch.equal(px, torch.from_numpy(x[pick.numpy()])) and torch.equal(py, torch.from_numpy(y[pick.numpy()]))
    assert pd.tolist() == dates[pick.numpy()].tolist()
    assert bank.window([n - 1])[0].shape == (1, T_in, 5, 7, x.shape[-1])


def test_binary_threshold_is_compared_in_float32():
    from qtmpnn.data import ClipBank
    series, times = _series(D=12, C=1)
    series[...] = np.float32(0.3)           # 0.30000001192092896: above 0.3 as a float64, equal to it as a float32
    series[4] = np.nextafter(np.float32(0.3), np.float32(1))
    bank = ClipBank(series, times, 2, 2, y_binary_thresh=0.3, device='cpu')
    assert bank.y[4].eq(1).all() and bank.y.sum() == bank.y[4].numel()
    _, y, _, _ = restated_windows(series, times, 2, 2, y_binary_thresh=0.3)
    assert torch.equal(bank.window(range(len(bank)))[1], torch.from_numpy(y))


def test_tensor_series_and_float32_input():
    from qtmpnn.data import ClipBank
    series, times = _series(dtype=np.float32)
    a = ClipBank(series, times, 3, 4, device='cpu')
    b = ClipBank(torch.from_numpy(series), torch.from_numpy(times), 3, 4, device='cpu')
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y) and np.array_equal(a.launch_dates, b.launch_dates)
    assert a.x.is_contiguous() and a.y.is_contiguous() and a.x.dtype == torch.float32


def _order(loader, passes=2):
    """The batches of `passes` passes as ([launch dates per batch], x batches, y batches)."""
    dates, xs, ys = [], [], []
    for _ in range(passes):
        for x, y, d in loader:
            dates.append(d.tolist())
            xs.append(x)
            ys.append(y)
    return dates, xs, ys


@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('shuffle, seeded', [(False, 'global'), (True, 'explicit'), (True, 'global')])
@pytest.mark.parametrize('batch_size', [1, 4])
def test_batch_order_is_the_dataloaders(batch_size, shuffle, seeded, drop_last):
    from qtmpnn.data import ClipBank
    series, times = _series()
    kw = dict(segments=[(0, 12), (15, 30)], y_channels=[0])
    host = RestatedDataset(series, times, 3, 4, **kw)
    bank = ClipBank(series, times, 3, 4, device='cpu', **kw)
    n = len(host)
    assert n == 5 + 8 and len(bank) == n and n % 4

    def run(make):
        torch.manual_seed(1234)
        g = torch.Generator().manual_seed(77) if seeded == 'explicit' else None
        loader = make(g)
        out = _order(loader), len(loader)
        return out, torch.get_rng_state(), None if g is None else g.get_state()
    (ref, ref_len), ref_global, ref_g = run(lambda g: DataLoader(host, batch_size=batch_size, shuffle=shuffle, generator=g,
                                                                 drop_last=drop_last))
    (got, got_len), got_global, got_g = run(lambda g: bank.loader(batch_size=batch_size, shuffle=shuffle, generator=g,
                                                                  drop_last=drop_last))
    # the same window numbers from a DataLoader over range(n), which is how the order is defined
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(77) if seeded == 'explicit' else None
    numbers = DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, generator=g, drop_last=drop_last)
    want = [host.launch_dates[b.numpy()].tolist() for _ in range(2) for b in numbers]
    assert got[0] == ref[0] == want
    assert got_len == ref_len == (n // batch_size if drop_last else -(-n // batch_size)) and len(got[0]) == 2 * got_len
    for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert got[1][0].shape == (batch_size, 3, 5, 7, 3) and got[2][0].shape == (batch_size, 4, 5, 7, 1)
    assert torch.equal(got_global, ref_global), 'the global CPU generator after two passes'
    assert (got_g is None and ref_g is None) or torch.equal(got_g, ref_g), 'the explicit generator after two passes'
    if shuffle:
        flat = [d for batch in got[0][:got_len] for d in batch]
        assert flat != sorted(flat) and got[0][:got_len] != got[0][got_len:], 'shuffled, and anew per pass'
    elif not drop_last:
        assert [d for batch in got[0][:got_len] for d in batch] == host.launch_dates.tolist()


def test_sizes():
    from qtmpnn.data import ClipBank
    series, times = _series(D=30, shape=(5, 7), C=3)
    bank = ClipBank(series, times, 3, 4, x_channels=[0, 1, 2], y_channels=[1], device='cpu')
    assert bank.nbytes == 30 * 5 * 7 * (3 + 1) * 4
    assert ClipBank(series, times, 3, 4, y_channels=[1], y_binary_thresh=0.5, device='cpu').nbytes == bank.nbytes
    assert ClipBank(series, times, 3, 4, device='cpu').nbytes == 30 * 5 * 7 * 6 * 4
    assert len(bank) == 23
    assert [len(bank.loader(batch_size=b)) for b in (1, 4, 23, 24)] == [23, 6, 1, 1]
    assert [len(bank.loader(batch_size=b, drop_last=True)) for b in (1, 4, 23, 24)] == [23, 5, 1, 0]
    assert bank.loader().dataset is bank and bank.loader().dataset.image_shape == (5, 7)


def test_refusals_by_name():
    from qtmpnn.data import ClipBank
    series, times = _series(D=20)
    ok = dict(series=series, times=times, input_timesteps=3, output_timesteps=4, device='cpu')

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            ClipBank(**{**ok, **change})
    refused(r'^series: must be \(D, W, H, C\)', series=series[..., 0])
    refused(r'^series: must be \(D, W, H, C\)', series=series[None])
    refused(r'^times: must be \(20,\)', times=times[:-1])
    refused(r'^times: must be \(20,\)', times=times[:, None])
    refused(r'^input_timesteps: must be an integer >= 1', input_timesteps=0)
    refused(r'^output_timesteps: must be an integer >= 1', output_timesteps=0)
    refused(r'^output_timesteps: must be an integer >= 1', output_timesteps=2.0)
    refused(r'^segments: .*within 0\.\.20', segments=[(0, 21)])
    refused(r'^segments: .*within 0\.\.20', segments=[(-1, 10)])
    refused(r'^segments: .*within 0\.\.20', segments=[(10, 10)])
    refused(r'^segments: .*ordered', segments=[(10, 20), (0, 10)])
    refused(r'^segments: .*overlap', segments=[(0, 12), (11, 20)])
    refused(r'^segments: .*\(start, stop\)', segments=[(0, 10, 20)])
    refused(r'^segments: no segment holds a window', segments=[(0, 7), (7, 14)])
    refused(r'^segments: no segment holds a window', input_timesteps=10, output_timesteps=10)
    refused(r'^segments: no segment holds a window', segments=[])
    refused(r'^x_channels: channel indices', x_channels=[])
    refused(r'^x_channels: channel indices', x_channels=[0, 3])
    refused(r'^y_channels: channel indices', y_channels=[-1])
    refused(r'^y_channels: channel indices', y_channels=[0.0])
    bank = ClipBank(**ok)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='^batch_size: must be an integer >= 1'):
            bank.loader(batch_size=bad)
    for bad in ([len(bank)], [-1], torch.tensor([0, 13])):
        with pytest.raises(ValueError, match=r'^idx: window numbers must be in 0\.\.12'):
            bank.window(bad)


def test_refusals_come_before_any_upload():
    """A device that does not exist is only touched after every check: the bad argument is what is reported."""
    from qtmpnn.data import ClipBank
    series, times = _series(D=20)
    with pytest.raises(ValueError, match='^y_channels:'):
        ClipBank(series, times, 3, 4, y_channels=[9], device='cuda:63')
    with pytest.raises(ValueError, match='^segments:'):
        ClipBank(series, times, 3, 4, segments=[(0, 5)], device='cuda:63')
