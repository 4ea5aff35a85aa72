"""A climatology per clip, host side: get_climatology_array for one launch date (the reference's, untouched) and for a batch of
them (entry [c] IS the single-date call on date c), the dates as the loaders give them, the memo of the day indices, the
clip-count check before any launch, and ClipBank.normals on a CPU bank against a plain-loop float64 restatement of the
reference's fillna(0).groupby('time.dayofyear').mean().  Nothing here may reach the library or the model's forward."""
import datetime

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from helpers import TinyLoader

T_OUT = 4
DAY = np.timedelta64(1, 'D')
# four launch dates at 12:00: across a new year into a leap year, up to 29 February (index 59), up to index 365 and round to 0,
# and an ordinary one
DATES = np.array(['2011-12-30T12', '2012-02-27T12', '2012-12-29T12', '2013-03-01T12'], dtype='datetime64[ns]').astype(np.int64)
WANT_DAYS = [[363, 364, 0, 1], [57, 58, 59, 60], [363, 364, 365, 0], [59, 60, 61, 62]]


@pytest.fixture
def nfp(monkeypatch):
    """A predictor without a device whose first launch of any kind fails the test (as tests/test_accumulate_host.py's)."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_OUT, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    for name in ('forward', 'process_inputs', 'unroll_output'):
        monkeypatch.setattr(Seq2Seq, name, launched)
    monkeypatch.setattr(_lib, 'call', launched)
    monkeypatch.setattr(nfp, 'zero_grad', launched)
    return nfp


def _climatology():
    """(1, 366, 8, 8): every day and every pixel its own value."""
    d = torch.arange(366, dtype=torch.float32)[:, None, None]
    return (d + torch.arange(64, dtype=torch.float32).reshape(8, 8) / 128.0)[None].contiguous()


def test_single_date_is_the_reference_expression(nfp):
    from model.utils import int_to_datetime
    clim = _climatology()
    for c, date in enumerate(DATES):
        launch = torch.from_numpy(DATES[c:c + 1])
        got = nfp.get_climatology_array(clim, launch)
        doys = [int_to_datetime(launch.numpy()[0] + 8.640e13 * t).timetuple().tm_yday - 1 for t in range(T_OUT)]
        assert doys == WANT_DAYS[c]
        want = torch.moveaxis(clim[:, doys], 0, -1)
        assert got.shape == (T_OUT, 8, 8, 1) and got.dtype == torch.float32 and got.device == clim.device
        assert torch.equal(got, want)
        assert got[:, 0, 0, 0].tolist() == [float(d) for d in doys]
    # the exceptions of the single-date path: what has no .numpy(), and an empty batch of dates
    with pytest.raises(AttributeError):
        nfp.get_climatology_array(clim, [int(DATES[0])])
    with pytest.raises(IndexError):
        nfp.get_climatology_array(clim, torch.zeros(0, dtype=torch.int64))


def test_batch_of_dates_gives_every_clip_its_own_normals(nfp):
    clim = _climatology()
    got = nfp.get_climatology_array(clim, torch.from_numpy(DATES))
    assert got.shape == (4, T_OUT, 8, 8, 1) and got.dtype == torch.float32 and got.device == clim.device
    for c in range(4):
        assert torch.equal(got[c], nfp.get_climatology_array(clim, torch.from_numpy(DATES[c:c + 1]))), c
        assert got[c, :, 0, 0, 0].tolist() == [float(d) for d in WANT_DAYS[c]]
    # several channels of normals keep their place: (B, T_out, W, H, Cy)
    two = torch.cat([clim, -clim])
    got2 = nfp.get_climatology_array(two, torch.from_numpy(DATES[:3]))
    assert got2.shape == (3, T_OUT, 8, 8, 2) and torch.equal(got2[..., :1], got[:3]) and torch.equal(got2[..., 1:], -got[:3])
    # a repeated date, any order
    pick = [2, 0, 2]
    got3 = nfp.get_climatology_array(clim, torch.from_numpy(DATES[pick]))
    assert torch.equal(got3, got[pick])


class _Dates(torch.utils.data.Dataset):
    """Items (x, y, launch_date) as the reference's IceDataset gives them: the date a numpy int64."""

    def __init__(self):
        self.x, self.y = np.zeros((4, 2, 8, 8, 1), np.float32), np.zeros((4, T_OUT, 8, 8, 1), np.float32)

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return self.x[i], self.y[i], DATES[i]


def test_dates_as_the_loaders_give_them(nfp):
    from qtmpnn.data import ClipBank
    clim = _climatology()
    want = torch.stack([nfp.get_climatology_array(clim, torch.from_numpy(DATES[c:c + 1])) for c in range(4)])
    (x, y, launch), = list(DataLoader(_Dates(), batch_size=4))
    assert launch.shape == (4,) and launch.dtype == torch.int64
    assert torch.equal(nfp.get_climatology_array(clim, launch), want)
    halves = [nfp.get_climatology_array(clim, launch) for _, _, launch in DataLoader(_Dates(), batch_size=2)]
    assert torch.equal(torch.cat(halves), want)
    # a CPU bank: a series of 8 days from each launch date's second day before, one segment each (T_in = 2)
    times = np.concatenate([date + (np.arange(8) - 2) * DAY.astype('timedelta64[ns]').astype(np.int64) for date in DATES])
    bank = ClipBank(np.zeros((32, 8, 8, 1), np.float32), times, 2, T_OUT, segments=[(8 * s, 8 * s + 8) for s in range(4)],
                    device='cpu')
    assert len(bank) == 4 * 2 and np.array_equal(bank.launch_dates[::2], DATES)
    (x, y, launch), = list(bank.loader(8))
    got = nfp.get_climatology_array(clim, launch)
    assert launch.dtype == torch.int64 and got.shape == (8, T_OUT, 8, 8, 1) and torch.equal(got[::2], want)
    assert got[5, :, 0, 0, 0].tolist() == [364.0, 365.0, 0.0, 1.0]         # (the window launched on 2012-12-30)
    # batches of one from the same loaders stay the reference's four-dimensional array
    _, _, launch = next(iter(bank.loader(1)))
    assert nfp.get_climatology_array(clim, launch).shape == (T_OUT, 8, 8, 1)


def test_day_indices_are_kept_per_launch_date(nfp, monkeypatch):
    import model.utils
    calls, real = [], model.utils.int_to_datetime

    def counted(x):
        calls.append(x)
        return real(x)
    monkeypatch.setattr(model.utils, 'int_to_datetime', counted)
    clim = _climatology()
    first = nfp.get_climatology_array(clim, torch.from_numpy(DATES))
    assert len(calls) == 4 * T_OUT
    again = nfp.get_climatology_array(clim, torch.from_numpy(DATES[[3, 1, 0, 2]]))
    assert len(calls) == 4 * T_OUT, 'a second batch of the same dates converts nothing'
    assert torch.equal(again, first[[3, 1, 0, 2]])
    nfp.get_climatology_array(clim, torch.from_numpy(np.array([DATES[0], DATES[0] + 86400 * 10 ** 9])))
    assert len(calls) == 5 * T_OUT, 'one new date'
    # the conversions see the float64 sums of the reference's expression
    assert all(isinstance(c, np.float64) for c in calls) and calls[1] == DATES[0] + 8.640e13 * 1


def test_clip_count_is_checked_by_name_before_any_launch(nfp):
    x, y = torch.zeros(4, 2, 8, 8, 1), torch.zeros(4, T_OUT, 8, 8, 1)
    three, four = torch.zeros(3, T_OUT, 8, 8, 1), torch.zeros(4, T_OUT, 8, 8, 1)
    match = r'climatology: .* 3 clips, x has 4'
    for call in (lambda: nfp.forward_loss(x, y, three),
                 lambda: nfp.train_step(x, y, three),
                 lambda: nfp.accumulated_step([(x, y, four), (x, y, three)]),
                 lambda: nfp.truncated_backward(x, y, three, None, truncated_backprop=2),
                 lambda: nfp.make_graphed_step(x, y, three),
                 lambda: nfp.make_graphed_step(x, y, three, accumulate=2),
                 lambda: nfp.make_graphed_rollout(x, three),
                 lambda: nfp.make_graphed_verification(x, y, three, products=('score',)),
                 lambda: nfp.sensitivity(x, three),
                 lambda: nfp.attention_weights(x, three)):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(ValueError, match=r'climatology: .* 2 clips, x has 1'):
        nfp.forward_loss(x[0], y[0], four[:2])
    assert not nfp.training_initiated and not nfp.model.static_shapes
    # a loader whose dates do not go with its clips: refused in the loops, before the first launch
    clim = _climatology()
    loader = TinyLoader([(x, y, torch.from_numpy(DATES[:3]))], (8, 8))
    with pytest.raises(ValueError, match=match):
        nfp.predict(loader, clim)
    # as many clips as x: no refusal, the call goes on to the model (which this fixture turns into a failure)
    for concat in (four, torch.zeros(T_OUT, 8, 8, 1), None):
        with pytest.raises(AssertionError, match='a launch was reached'):
            nfp.forward_loss(x, y, concat)


def test_the_model_itself_checks_before_its_encoder(monkeypatch):
    from model.seq2seq import Seq2Seq

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(Seq2Seq, 'process_inputs', launched)
    model = Seq2Seq(8, 0.0, 0.1, input_timesteps=2, input_features=4, output_timesteps=T_OUT, n_layers=1)
    x, y = torch.zeros(4, 2, 8, 8, 1), torch.zeros(4, T_OUT, 8, 8, 1)
    with pytest.raises(ValueError, match=r'climatology: .* 3 clips, x has 4'):
        model(x, y, torch.zeros(3, T_OUT, 8, 8, 1))
    with pytest.raises(AssertionError, match='a launch was reached'):
        model(x, y, torch.zeros(4, T_OUT, 8, 8, 1))


# -- ClipBank.normals ----------------------------------------------------------------------------------------------------------
def _normals_series():
    """(40, 6, 5, 2) float64 with NaNs and an infinity; the same 20 calendar days, 19 - 28 February and 1 - 10 March, in 2011
    and in 2012, a leap year: February's fall on indices 49..58 in both, March's on 59..68 in 2011 and on 60..69 in 2012, so
    index 59 has one day (1 March 2011), as has 69, the others between 49 and 68 two, and most none."""
    rng = np.random.default_rng(3)
    series = rng.random((40, 6, 5, 2))
    series[3, 1, 2, 0] = np.nan
    series[::9, 4, :, 1] = np.nan
    series[25, 0, 0, 0] = np.inf
    times = np.concatenate([np.datetime64(f'{year}-{start}T12', 'ns') + np.arange(10) * DAY
                            for year in (2011, 2012) for start in ('02-19', '03-01')]).astype(np.int64)
    return series, times


def restated_normals(series, times, picked, y_channels, thresh=None):
    """Plain loops, float64: per selected day in ascending order, its float32 nan_to_num values (or 0 / 1 against the float32
    threshold) added to the sum of its day-of-year index (0-based, local time); the mean where there is a day, 0 elsewhere."""
    stored = np.nan_to_num(np.asarray(series).astype(np.float32))
    D, W, H, _ = stored.shape
    sums, counts = np.zeros((len(y_channels), 366, W, H), np.float64), np.zeros(366, np.int64)
    for day in range(D):
        if not picked[day]:
            continue
        d = datetime.datetime.fromtimestamp(int(times[day]) / 1e9).timetuple().tm_yday - 1
        counts[d] += 1
        for k, c in enumerate(y_channels):
            for i in range(W):
                for j in range(H):
                    v = stored[day, i, j, c]
                    if thresh is not None:
                        v = np.float32(1.0) if v > np.float32(thresh) else np.float32(0.0)
                    sums[k, d, i, j] += np.float64(v)
    for d in range(366):
        if counts[d]:
            sums[:, d] /= counts[d]
    return sums, counts


def _held(got, want, counts):
    """|got - want| <= 2^-24 |want|: one float32 rounding of a float64 mean (whose own error, n 2^-53 relative, is far below
    that); indices without a day are exactly 0."""
    got = got.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want)).all(), float(np.abs(got - want).max())
    assert (got[:, counts == 0] == 0).all() and (want[:, counts == 0] == 0).all()


def test_normals_on_a_cpu_bank_equal_the_restatement():
    from qtmpnn.data import ClipBank
    series, times = _normals_series()
    bank = ClipBank(series, times, 3, 4, segments=[(0, 10), (10, 20), (20, 30), (30, 40)], x_channels=[0], device='cpu')
    got = bank.normals()
    want, counts = restated_normals(series, times, np.ones(40, bool), [0, 1])
    assert got.shape == (2, 366, 6, 5) and got.dtype == torch.float32 and got.is_contiguous() and got.device.type == 'cpu'
    assert counts[49:70].tolist() == [2] * 10 + [1] + [2] * 9 + [1] and counts.sum() == 40
    _held(got, want, counts)
    assert torch.equal(bank.normals(), got), 'two calls give the same bits'
    assert got[:, 49:70].abs().sum() > 0 and torch.isfinite(got).all()
    # days= as a mask and as ranges: the first year, and both years without their last five days
    first = np.arange(40) < 20
    want1, counts1 = restated_normals(series, times, first, [0, 1])
    assert counts1[49:69].tolist() == [1] * 20 and counts1.sum() == 20
    for days in (first, torch.from_numpy(first), [(0, 20)]):
        _held(bank.normals(days), want1, counts1)
        assert torch.equal(bank.normals(days), bank.normals([(0, 20)]))
    # one day of index 59 alone: its mean is the day itself
    assert torch.equal(bank.normals(first)[:, 59], bank.y[10].permute(2, 0, 1))
    ranges = [(0, 15), (20, 36)]
    picked = np.zeros(40, bool)
    picked[0:15] = picked[20:36] = True
    want2, counts2 = restated_normals(series, times, picked, [0, 1])
    assert counts2[49:67].tolist() == [2] * 10 + [1] + [2] * 4 + [1, 1, 0]
    _held(bank.normals(ranges), want2, counts2)
    _held(bank.normals(picked), want2, counts2)
    assert torch.equal(bank.normals(ranges), bank.normals(picked))
    # it is the array train(climatology=) takes: get_climatology_array indexes it
    from model.mpnnlstm import NextFramePredictorS2S
    concat = NextFramePredictorS2S.get_climatology_array(type('P', (), {'output_timesteps': 4, '_output_days': {}})(), got,
                                                         torch.from_numpy(bank.launch_dates[:2]))
    assert concat.shape == (2, 4, 6, 5, 2) and torch.equal(concat[1, 0], got[:, 53].permute(1, 2, 0))


def test_normals_of_a_binary_bank_and_one_channel():
    from qtmpnn.data import ClipBank
    series, times = _normals_series()
    series[5, :, :, 1] = np.float32(0.4)            # AT the float32 threshold: not above it
    bank = ClipBank(series, times, 3, 4, y_channels=[1], y_binary_thresh=0.4, device='cpu')
    want, counts = restated_normals(series, times, np.ones(40, bool), [1], thresh=0.4)
    got = bank.normals()
    assert got.shape == (1, 366, 6, 5)
    _held(got, want, counts)
    assert set(got.unique().tolist()) <= {0.0, 0.5, 1.0} and len(got.unique()) == 3
    assert torch.equal(bank.normals(), got)


def test_normals_refusals_name_the_argument():
    from qtmpnn.data import ClipBank
    series, times = _normals_series()
    bank = ClipBank(series, times, 3, 4, device='cpu')
    for bad, match in ((np.ones(39, bool), r'days: a boolean selection must be \(40,\)'),
                       (np.zeros(40, bool), 'days: no day is selected'),
                       (np.ones(40, np.float32), 'days: must be a boolean'),
                       (torch.ones(40), 'days: must be a boolean'),
                       (5, 'days: must be a boolean'),
                       ([(0, 41)], r'days: days\[0\] = \(0, 41\) is not a range of days within 0..40'),
                       ([(5, 5)], r'days: days\[0\] = \(5, 5\) is not a range'),
                       ([(0, 10), (8, 12)], r'days: days\[1\] = \(8, 12\) starts before days\[0\] stops at day 10'),
                       ([(0, 10, 2)], r'days: days\[0\] must be \(start, stop\)'),
                       ([(0.0, 10)], r'days: days\[0\] must be \(start, stop\)'),
                       ([], 'days: no day is selected')):
        with pytest.raises(ValueError, match=match):
            bank.normals(bad)
    # the refusals of `segments` keep their words
    with pytest.raises(ValueError, match=r'segments: segments\[1\] = \(8, 12\) starts before segments\[0\] stops at day 10'):
        ClipBank(series, times, 3, 4, segments=[(0, 10), (8, 12)], device='cpu')
