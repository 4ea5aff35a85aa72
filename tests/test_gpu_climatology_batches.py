"""Batches of B > 1 clips with a climatology on the GPU: every clip gets the normals of its own output days, through train (eager,
graphed, accumulated, 'stream'), predict and verify, and ClipBank.normals() on the device.

The data recipe of tests/test_gpu_clipbank.py -- 64 x 64 frames, 40 days in two seasons of 22 and 18 days, 3 in / 4 out (15 + 11
windows), two channels, x on both and y on channel 0; hidden 8, ChebConv, one layer, that file's mask -- with two changes: the
first season runs across 2012-12-31 / 2013-01-01, so a leap year's index 365 and the wrap to 0 are among the output days, and the
normals have 366 days (helpers.climatology_from_base's formula one day further).  Batches of 4: the last one holds 2 windows."""
import functools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from clipbank_restated import RestatedDataset
from helpers import climatology_from_base, close, dev

pytestmark = pytest.mark.gpu

T_IN, T_OUT, SEGMENTS = 3, 4, [(0, 22), (22, 40)]
KW = dict(segments=SEGMENTS, x_channels=[0, 1], y_channels=[0])
LR, DECAY, SEED, THRESHOLD = 0.01, 0.5, 23, 0.15
# the model of the batch-against-single-clips case: of the seeds 20..69 this one leaves no pixel of the single-clip run within
# 1e-4 of the threshold while 15 % of the pixels lie above it (the test asserts the former)
VERIFY_SEED = 41


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)         # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _data():
    """(series (40, 64, 64, 2) float64 with NaNs, times, mask, the restated host dataset, the bank): made once, not modified."""
    from qtmpnn import synthetic
    from qtmpnn.data import ClipBank
    seasons = [np.concatenate([synthetic.make_clip(900 + 10 * s + c, n_digits=2, n_frames=e - b, pixel_noise=0.02)
                               for c in range(2)], axis=-1) for s, (b, e) in enumerate(SEGMENTS)]
    series = np.concatenate(seasons).astype(np.float64)
    series[::7, 60:, 60:, 1] = np.nan
    day = np.timedelta64(1, 'D')
    times = np.concatenate([np.datetime64('2012-12-20T12', 'ns') + np.arange(22) * day,       # (across 31 December of a leap year)
                            np.datetime64('2013-03-01T12', 'ns') + np.arange(18) * day]).astype(np.int64)
    mask = np.zeros((64, 64), dtype=bool)
    mask[:16, :24] = True
    host = RestatedDataset(series, times, T_IN, T_OUT, **KW)
    bank = ClipBank(series, times, T_IN, T_OUT, device=dev(), **KW)
    assert len(host) == 15 + 11 and host.y.shape == (26, 4, 64, 64, 1)
    return series, times, mask, host, bank


@functools.lru_cache(maxsize=None)
def _climatology():
    """(1, 366, 64, 64) on the device: climatology_from_base and, by the same formula, day 365."""
    base = np.random.default_rng(11).random((64, 64), dtype=np.float32)
    d = np.float32(365)
    last = (base[None] * (0.5 + 0.5 * np.cos(2 * np.pi * d / 365.0)) + 0.001 * d)[None].astype(np.float32)
    clim = np.concatenate([climatology_from_base(base), last], axis=1)
    assert clim.shape == (1, 366, 64, 64) and clim.dtype == np.float32
    return torch.from_numpy(clim).to(dev())


@functools.lru_cache(maxsize=None)
def _single_date_arrays():
    """The (T_out, 64, 64, 1) normals of every window, each by the single-date call: (26, T_out, 64, 64, 1).  Computed once."""
    nfp = _predictor()
    host = _data()[3]
    days = [[d.item() for d in nfp.get_climatology_array(torch.arange(366.0).reshape(1, 366, 1, 1), torch.from_numpy(host.launch_dates[i:i + 1])).reshape(-1)]
            for i in range(26)]
    assert any(365.0 in row and 0.0 in row for row in days), 'a window reaches index 365 and wraps'
    return torch.stack([nfp.get_climatology_array(_climatology(), torch.from_numpy(host.launch_dates[i:i + 1])) for i in range(26)])


def _seed(seed):
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())


def _predictor(dropout=0.1):
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=2, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=dropout, n_layers=1, n_conv_layers=1, convolution_type='ChebConv'))
    nfp.model.train()
    return nfp


def _perturbed(seed=SEED):
    _seed(seed)
    nfp = _predictor()
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    nfp.model.eval()
    return nfp


def _loaders(kind, batch_size, shuffle=False):
    """(train loader, test loader) over the bank or over the restated windows on the host; shuffle: False or 'explicit' (a
    generator of a fixed seed per loader)."""
    _, _, _, host, bank = _data()
    g = torch.Generator().manual_seed(5) if shuffle == 'explicit' else None
    if kind == 'bank':
        return bank.loader(batch_size, shuffle=bool(shuffle), generator=g), bank.loader(batch_size)
    return DataLoader(host, batch_size=batch_size, shuffle=bool(shuffle), generator=g), DataLoader(host, batch_size=batch_size)


def test_every_clip_is_given_the_normals_of_its_own_days(monkeypatch):
    """What the model is given: the concat_layers of every self.model(...) call of predict over batches of 4 is
    (b, T_out, 64, 64, 1), the stack of the single-date arrays of its clips -- the short last batch of 2 included.  (On the
    parent commit the array is the first clip's (T_out, 64, 64, 1) and the rollout ends in `RuntimeError: shape '[4, 1, 4096,
    1]' is invalid for input of size 4096`.)"""
    nfp, want = _perturbed(), _single_date_arrays()
    seen, forward = [], nfp.model.forward

    def spy(x, *a, **k):
        seen.append((x.shape[0], k['concat_layers'].clone()))
        return forward(x, *a, **k)
    monkeypatch.setattr(nfp.model, 'forward', spy)
    out = nfp.predict(_loaders('bank', 4)[1], _climatology(), mask=_data()[2])
    assert out.shape == (26, T_OUT, 64, 64, 1)
    assert [b for b, _ in seen] == [4] * 6 + [2]
    lo = 0
    for b, concat in seen:
        assert concat.shape == (b, T_OUT, 64, 64, 1) and concat.device == dev() and concat.dtype == torch.float32
        assert torch.equal(concat, want[lo:lo + b]), f'clips {lo}..{lo + b - 1}'
        lo += b
    assert not torch.equal(want[0], want[1]), 'the clips of a batch differ in their normals'


def _train(kind, use_graph, shuffle, dropout=0.1, static=False):
    _seed(SEED)
    nfp = _predictor(dropout)
    if static:          # static capacities and the capturable optimiser, as the captured step's own warm-up steps run
        nfp.initiate_training(LR, DECAY, capturable=True)
        nfp.model.static_shapes = True
    train, test = _loaders(kind, 4, shuffle)
    nfp.train(train, test, _climatology(), n_epochs=2, lr=LR, lr_decay=DECAY, mask=_data()[2], truncated_backprop=0,
              use_graph=use_graph)
    return nfp, torch.get_rng_state()


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('shuffle', [False, 'explicit'])
def test_training_over_the_bank_equals_training_over_host_windows(use_graph, shuffle):
    """Batches of 4 with a climatology, as tests/test_gpu_clipbank.py holds batches of 1: the same losses, parameters and
    generator state from the bank's loader and from a DataLoader of the restated windows, bit for bit."""
    a, a_rng = _train('bank', use_graph, shuffle)
    b, b_rng = _train('host', use_graph, shuffle)
    print(f'bank train {a.train_loss} test {a.test_loss}\nhost train {b.train_loss} test {b.test_loss}')
    assert len(a.train_loss) == 2 and np.isfinite(a.train_loss + a.test_loss).all()
    assert a.train_loss == b.train_loss and a.test_loss == b.test_loss
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(a_rng, b_rng), 'the global CPU generator after the run'


@pytest.mark.parametrize('use_graph', [False, True])
def test_predict_over_the_bank_equals_the_host_loader(use_graph):
    nfp = _perturbed()
    clim, mask = _climatology(), _data()[2]
    pa = nfp.predict(_loaders('bank', 4)[1], clim, mask=mask, use_graph=use_graph)
    pb = nfp.predict(_loaders('host', 4)[1], clim, mask=mask, use_graph=use_graph)
    assert pa.shape == (26, T_OUT, 64, 64, 1) and pa.dtype == pb.dtype and np.nanstd(pa) > 0
    assert np.array_equal(pa, pb, equal_nan=True)


def test_graphed_training_follows_eager_training():
    """train(use_graph=True) at batch 4 with a climatology against eager training from the same state, held as
    tests/test_gpu_rollout.py::test_baseline_config_shapes_train holds a captured step to its eager twin: both predictors train
    with static capacities and the capturable optimiser, dropout is off (captured and eager steps draw different masks), and
    every epoch's losses agree to 1e-4 relative.  The parameters after the two epochs are held to the suite's bound for float32
    results (helpers.close: rtol 1e-4, atol 1e-5)."""
    e, _ = _train('bank', False, False, dropout=0.0, static=True)
    g, _ = _train('bank', True, False, dropout=0.0, static=True)
    print(f'eager train {e.train_loss} test {e.test_loss}\ngraph train {g.train_loss} test {g.test_loss}')
    assert len(g.train_loss) == 2 and np.isfinite(g.train_loss + g.test_loss).all()
    for a, b in zip(e.train_loss + e.test_loss, g.train_loss + g.test_loss):
        assert abs(a - b) <= 1e-4 * abs(a), (e.train_loss, g.train_loss, e.test_loss, g.test_loss)
    worst = max(float((p - q).detach().abs().max()) for p, q in zip(e.model.parameters(), g.model.parameters()))
    print(f'largest parameter difference {worst:.3e}')
    for (k, p), (_, q) in zip(e.model.named_parameters(), g.model.named_parameters()):
        close(q, p, msg=k)


def test_verification_of_batches_equals_verification_of_single_clips():
    """verify(products=('score', 'extent', 'fss')) with a climatology over batches of 4 against batches of 1.  The 'climatology'
    and 'persistence' rows, and the truth's, do not depend on the model: equal to the bit, per clip and lead time (the parent's
    first-date rule would have given clips 1..3 of a batch the normals of clip 0).  The 'model' rows: the rollout of a batch
    against that of its clips one by one is held to 1e-4 relative per pixel (tests/test_gpu_rollout.py::
    test_rollout_batched_equals_single), |f' - f| <= 1e-4 |f|, which bounds the sums of differences by 1e-4 sum |f| and the sums
    of squares by 1e-4 sum |f| (2 |f - y| + 1e-4 |f|), with f and y from the single-clip run.  Counts may differ by the pixels
    whose value lies within 1e-4 (relative) of the threshold; the seed is chosen so that the single-clip run has none, which
    is asserted: the counts are then equal."""
    nfp = _perturbed(VERIFY_SEED)
    clim, mask = _climatology(), _data()[2]
    products = ('score', 'extent', 'fss')
    v4 = nfp.verify(_loaders('bank', 4)[1], clim, mask=mask, products=products)
    v1 = nfp.verify(_loaders('bank', 1)[1], clim, mask=mask, products=products)
    assert v4.sources == v1.sources == ('model', 'persistence', 'climatology')
    s4, s1, e4, e1, f4, f1 = v4.score.sums, v1.score.sums, v4.extent.sums, v1.extent.sums, v4.fss.sums, v1.fss.sums
    assert s4.shape == (26, T_OUT, 3, 8) and e4.shape == (26, T_OUT, 1, 4, 4) and f4.shape[:3] == (26, T_OUT, 3)
    assert s1.shape == s4.shape and e1.shape == e4.shape and f1.shape == f4.shape
    # what does not depend on the model
    assert np.array_equal(s4[:, :, 1:], s1[:, :, 1:]) and np.array_equal(f4[:, :, 1:], f1[:, :, 1:])
    assert np.array_equal(e4[:, :, :, 0], e1[:, :, :, 0]) and np.array_equal(e4[:, :, :, 2:], e1[:, :, :, 2:])
    # ... and is each clip's own: the climatology's sum |d| against the single-date arrays, restated on the host with d in
    # float32 as the kernel forms it and the sum in float64.  The kernel sums a tile of 1024 pixels in float32 -- 3 additions
    # per thread, a 6-level butterfly, 2 levels over the waves: 11 roundings on any term's path -- and the tiles in float64;
    # the terms are non-negative, so it is within 11 * 2^-24 relative of the exact sum (12 allows for the float64 additions)
    keep = ~mask
    y = _data()[3].y[..., 0][:, :, keep]                                                     # (26, T_out, pixels) float32
    c = _single_date_arrays().cpu().numpy()[..., 0][:, :, keep]
    assert y.dtype == c.dtype == np.float32
    np.testing.assert_allclose(s4[:, :, 2, 2], np.abs(c - y).astype(np.float64).sum(-1), rtol=12 * 2.0 ** -24)
    assert np.array_equal(s4[:, :, 2, 5], ((c > THRESHOLD) & ~(y > THRESHOLD)).sum(-1))
    assert len({tuple(row) for row in s4[:, 0, 2, 2:4].tolist()}) == 26, 'every clip has normals of its own'
    # the model's rows
    f = nfp.predict(_loaders('bank', 1)[1], clim, mask=mask)[..., 0].astype(np.float64)[:, :, keep]
    near = np.abs(f - THRESHOLD) <= 1e-4 * np.maximum(np.abs(f), THRESHOLD)
    assert not near.any(), f'{int(near.sum())} pixels of the single-clip run lie within 1e-4 of the threshold: choose another seed'
    sum_f = np.abs(f).sum(-1)
    sum_sq = (np.abs(f) * (2 * np.abs(f - y.astype(np.float64)) + 1e-4 * np.abs(f))).sum(-1)
    for slot, bound in ((1, sum_f), (2, sum_f), (3, sum_sq)):
        err = np.abs(s4[:, :, 0, slot] - s1[:, :, 0, slot])
        print(f'score slot {slot}: largest difference {err.max():.3e}, smallest bound {1e-4 * bound.min():.3e}')
        assert (err <= 1e-4 * bound).all(), slot
    assert np.array_equal(s4[:, :, 0, [0, 4, 5, 6, 7]], s1[:, :, 0, [0, 4, 5, 6, 7]]), 'counts'
    assert np.array_equal(f4[:, :, 0], f1[:, :, 0]), 'neighbourhood counts'
    assert np.array_equal(e4[:, :, 0, 1, [0, 2, 3]], e1[:, :, 0, 1, [0, 2, 3]]), 'extent, over, under: pixel counts'
    assert (np.abs(e4[:, :, 0, 1, 1] - e1[:, :, 0, 1, 1]) <= 1e-4 * sum_f).all(), 'ice area'
    assert s1[..., 0].min() > 0, 'counted pixels'


def _micro_batches():
    """Two micro-batches of 4 windows with their per-clip normals, on the device."""
    nfp, out = _predictor(), []
    for _, (x, y, launch) in zip(range(2), _loaders('bank', 4)[0]):
        out.append((x, y, nfp.get_climatology_array(_climatology(), launch)))
    assert out[0][2].shape == (4, T_OUT, 64, 64, 1)
    return out


def _trainer(dropout=0.0, static=True):
    _seed(SEED)
    nfp = _predictor(dropout)
    nfp.initiate_training(1e-3, 0.95, capturable=True)
    nfp.model.static_shapes = static
    return nfp


def test_graphed_accumulated_step_with_per_clip_normals_equals_the_eager_one():
    """make_graphed_step(accumulate=2) on micro-batches of 4 clips with their climatology against eager static-mode
    accumulated_step from the same state: torch.equal, as tests/test_gpu_accumulate.py::
    test_graphed_accumulated_step_matches_the_eager_one holds them without one."""
    group, mask = _micro_batches(), _data()[2]
    eager, graphed = _trainer(), _trainer()
    step = graphed.make_graphed_step(*group[0], mask, warmup=1, accumulate=2)
    assert torch.equal(eager.accumulated_step([group[0]], mask), graphed.last_warmup_loss)
    for batches in (group, group[:1], group):
        le, lg = eager.accumulated_step(batches, mask), step(batches)
        print(f'{len(batches)} micro-batches: eager {float(le):.8f} graphed {float(lg):.8f}')
        assert torch.isfinite(le) and torch.equal(le, lg)
    for (k, p), (_, q) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p, q), k
    with pytest.raises(ValueError, match='climatology'):
        step([(group[0][0], group[0][1], group[0][2][:3])])


def test_stream_step_with_per_clip_normals_has_the_plain_loss():
    x, y, concat = _micro_batches()[1]
    mask = _data()[2]
    plain, stream = _trainer(0.1, False), _trainer(0.1, False)
    stream.set_recompute('stream')
    _seed(SEED + 1)
    lp = plain.train_step(x, y, concat, mask)
    _seed(SEED + 1)
    ls = stream.train_step(x, y, concat, mask)
    print(f'plain {float(lp):.8f} stream {float(ls):.8f}')
    assert torch.isfinite(lp) and torch.equal(lp, ls)


def test_normals_on_the_device_equal_the_cpu_bank():
    """bank.normals() on the device against a device='cpu' bank of the same series, |got - want| <= 2^-24 |want| (the bound of
    tests/test_climatology_batches_host.py: one float32 rounding of a float64 mean); two calls give the same bits."""
    from qtmpnn.data import ClipBank
    series, times, _, _, bank = _data()
    cpu = ClipBank(series, times, T_IN, T_OUT, device='cpu', **KW)
    got, want = bank.normals(), cpu.normals()
    assert got.shape == (1, 366, 64, 64) and got.dtype == torch.float32 and got.device == dev() and got.is_contiguous()
    assert torch.equal(bank.normals(), got)
    a, b = got.cpu().double(), want.double()
    assert bool(((a - b).abs() <= 2.0 ** -24 * b.abs()).all()), float((a - b).abs().max())
    picked = np.arange(40) < 22
    assert torch.equal(bank.normals(picked), bank.normals([(0, 22)]))
    # 20 December of a leap year is index 354: the first season fills 354..365 and 0..9, the second 59..76
    assert bool(got[0, 365].abs().sum() > 0) and bool(got[0, 9].abs().sum() > 0) and bool((got[0, 77:354] == 0).all())


def test_train_and_predict_on_the_banks_own_normals():
    """End to end: train(train_loader, test_loader, bank.normals(), ...) at batch 4 for one epoch, then predict."""
    _seed(SEED)
    nfp = _predictor()
    bank, mask = _data()[4], _data()[2]
    normals = bank.normals()
    nfp.train(bank.loader(4, shuffle=True, generator=torch.Generator().manual_seed(5)), bank.loader(4), normals, n_epochs=1, lr=LR,
              lr_decay=DECAY, mask=mask, truncated_backprop=0, use_graph=True)
    assert len(nfp.train_loss) == 1 and np.isfinite(nfp.train_loss + nfp.test_loss).all()
    nfp.model.eval()
    out = nfp.predict(bank.loader(4), normals, mask=mask)
    assert out.shape == (26, T_OUT, 64, 64, 1) and np.isfinite(out[:, :, ~mask]).all()
