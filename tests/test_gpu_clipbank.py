"""qtmpnn.data.ClipBank on the GPU: its batches against the plain-loop restatement uploaded, and every loop that takes a loader --
train (eager and graphed, shuffled and not), predict, verify, a captured step -- over the bank's loader against the same call
over a torch DataLoader of the restated windows, bit for bit.  The bank has no kernel of its own, so the second run IS the reference.

The data: 64 x 64 frames, 40 days in two seasons of 22 and 18 days, 3 in / 4 out (15 + 11 windows), two channels, x on both and y
on channel 0; hidden 8, ChebConv, one layer.  Batches of 4 (the last one short) without a climatology; with a climatology batches
of 1, the reference's loaders: get_climatology_array reads the first clip's launch date for a whole batch."""
import functools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from clipbank_restated import RestatedDataset
from helpers import climatology_from_base, dev

pytestmark = pytest.mark.gpu

T_IN, T_OUT, SEGMENTS = 3, 4, [(0, 22), (22, 40)]
KW = dict(segments=SEGMENTS, x_channels=[0, 1], y_channels=[0])
LR, DECAY, SEED = 0.01, 0.5, 23


@functools.lru_cache(maxsize=None)
def _data():
    """(series (40, 64, 64, 2) float64 with NaNs, times, mask, the restated host dataset, the bank): made once, not modified."""
    from qtmpnn import synthetic
    from qtmpnn.data import ClipBank
    seasons = [np.concatenate([synthetic.make_clip(900 + 10 * s + c, n_digits=2, n_frames=e - b, pixel_noise=0.02)
                               for c in range(2)], axis=-1) for s, (b, e) in enumerate(SEGMENTS)]
    series = np.concatenate(seasons).astype(np.float64)
    series[::7, 60:, 60:, 1] = np.nan                       # (missing values, as over land in the reanalysis)
    day = np.timedelta64(1, 'D')
    times = np.concatenate([np.datetime64('2010-12-20T12', 'ns') + np.arange(22) * day,           # (the output days wrap the year)
                            np.datetime64('2012-03-01T12', 'ns') + np.arange(18) * day]).astype(np.int64)
    mask = np.zeros((64, 64), dtype=bool)
    mask[:16, :24] = True
    host = RestatedDataset(series, times, T_IN, T_OUT, **KW)
    bank = ClipBank(series, times, T_IN, T_OUT, device=dev(), **KW)
    assert len(host) == 15 + 11 and host.x.shape == (26, 3, 64, 64, 2) and host.y.shape == (26, 4, 64, 64, 1)
    return series, times, mask, host, bank


@functools.lru_cache(maxsize=None)
def _climatology():
    base = np.random.default_rng(11).random((64, 64), dtype=np.float32)
    return torch.from_numpy(climatology_from_base(base)).to(dev())


def _seed(seed):
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())


def _predictor():
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=2, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.1, n_layers=1, n_conv_layers=1, convolution_type='ChebConv'))
    nfp.model.train()
    return nfp


def _loaders(kind, batch_size, shuffle):
    """(train loader, test loader) over the bank or over the restated windows on the host; shuffle: False, 'explicit' (a
    generator of a fixed seed per loader) or 'global' (torch's CPU generator, as seeded by the caller)."""
    _, _, _, host, bank = _data()
    g = torch.Generator().manual_seed(5) if shuffle == 'explicit' else None
    if kind == 'bank':
        return bank.loader(batch_size, shuffle=bool(shuffle), generator=g), bank.loader(batch_size)
    return DataLoader(host, batch_size=batch_size, shuffle=bool(shuffle), generator=g), DataLoader(host, batch_size=batch_size)


@pytest.mark.parametrize('batch_size', [1, 4])
def test_batches_equal_the_restated_windows(batch_size):
    _, _, _, host, bank = _data()
    assert bank.nbytes == 40 * 64 * 64 * (2 + 1) * 4 and bank.image_shape == (64, 64)
    assert bank.x.device == dev() and bank.y.device == dev() and bank.x.is_contiguous() and bank.y.is_contiguous()
    loader = bank.loader(batch_size)
    assert len(loader) == -(-26 // batch_size)
    seen = 0
    for x, y, launch in loader:
        b = min(batch_size, 26 - seen)
        assert x.device == dev() and y.device == dev() and x.dtype == y.dtype == torch.float32
        assert x.shape == (b, 3, 64, 64, 2) and y.shape == (b, 4, 64, 64, 1) and x.is_contiguous() and y.is_contiguous()
        assert launch.device.type == 'cpu' and launch.dtype == torch.int64 and launch.numpy()[0] == host.launch_dates[seen]
        assert torch.equal(x, torch.from_numpy(host.x[seen:seen + b]).to(dev()))
        assert torch.equal(y, torch.from_numpy(host.y[seen:seen + b]).to(dev()))
        assert torch.equal(launch, torch.from_numpy(host.launch_dates[seen:seen + b]))
        seen += b
    assert seen == 26 and b == (1 if batch_size == 1 else 2), 'the short last batch'
    assert not torch.isnan(bank.x).any() and bank.x[0, 60:, 60:, 1].eq(0).all()


def _train(kind, batch_size, with_clim, use_graph, shuffle):
    _seed(SEED)
    nfp = _predictor()
    train, test = _loaders(kind, batch_size, shuffle)
    nfp.train(train, test, _climatology() if with_clim else None, n_epochs=2, lr=LR, lr_decay=DECAY, mask=_data()[2],
              truncated_backprop=0, use_graph=use_graph)
    return nfp, torch.get_rng_state()


@pytest.mark.parametrize('batch_size, with_clim, use_graph, shuffle', [
    (4, False, False, False), (4, False, False, 'explicit'), (4, False, True, False), (4, False, True, 'explicit'),
    (4, False, True, 'global'),
    (1, True, False, False), (1, True, False, 'explicit'), (1, True, False, 'global'), (1, True, True, False),
    (1, True, True, 'explicit')])
def test_training_over_the_bank_equals_training_over_host_windows(batch_size, with_clim, use_graph, shuffle, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a, a_rng = _train('bank', batch_size, with_clim, use_graph, shuffle)
    b, b_rng = _train('host', batch_size, with_clim, use_graph, shuffle)
    print(f'bank train {a.train_loss} test {a.test_loss}\nhost train {b.train_loss} test {b.test_loss}')
    assert len(a.train_loss) == 2 and np.isfinite(a.train_loss + a.test_loss).all()
    assert a.train_loss == b.train_loss and a.test_loss == b.test_loss
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(a_rng, b_rng), 'the global CPU generator after the run'
    if shuffle and batch_size == 4 and not use_graph:       # the control: the order matters to these numbers
        c, _ = _train('bank', batch_size, with_clim, use_graph, False)
        assert c.train_loss != a.train_loss


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('batch_size, with_clim', [(4, False), (1, True)])
def test_predict_and_verify_over_the_bank_equal_the_host_loader(batch_size, with_clim, use_graph):
    _seed(SEED)
    nfp = _predictor()
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    nfp.model.eval()
    clim, mask = _climatology() if with_clim else None, _data()[2]
    bank, host = (_loaders(kind, batch_size, False)[1] for kind in ('bank', 'host'))
    pa = nfp.predict(bank, clim, mask=mask, use_graph=use_graph)
    pb = nfp.predict(host, clim, mask=mask, use_graph=use_graph)
    assert pa.shape == (26, T_OUT, 64, 64, 1) and pa.dtype == pb.dtype and np.nanstd(pa) > 0
    assert np.array_equal(pa, pb, equal_nan=True)
    va = nfp.verify(bank, clim, mask=mask, use_graph=use_graph, products=('score', 'fss'))
    vb = nfp.verify(host, clim, mask=mask, use_graph=use_graph, products=('score', 'fss'))
    assert va.sources == vb.sources == ('model', 'persistence') + (('climatology',) if with_clim else ())
    for name in ('score', 'fss'):
        assert va[name].sums.shape == vb[name].sums.shape and va[name].sums.shape[0] == 26
        assert np.array_equal(va[name].sums, vb[name].sums, equal_nan=True), name
        assert va[name].sources == vb[name].sources
    assert va.score.sums[..., 0].min() > 0, 'counted pixels'


def test_step_captured_on_a_bank_batch_replays_on_later_ones():
    """make_graphed_step on the bank's first batch (its warm-up is that batch's update), replayed on the next four: the losses
    and the parameters of eager static-mode train_steps on the same batches of the host loader."""
    mask = _data()[2]
    bank, host = (_loaders(kind, 4, False)[0] for kind in ('bank', 'host'))
    _seed(SEED)
    graphed = _predictor()
    graphed.initiate_training(LR, DECAY, capturable=True)
    lg = []
    for i, (x, y, _) in zip(range(5), bank):
        if i == 0:
            step = graphed.make_graphed_step(x, y, None, mask, warmup=1)
            lg.append(float(graphed.last_warmup_loss))
        else:
            lg.append(float(step(x, y)))
    step.check()
    _seed(SEED)
    eager = _predictor()
    eager.initiate_training(LR, DECAY)
    eager.model.static_shapes = True
    le = [float(eager.train_step(x.to(dev()), y.to(dev()), None, mask)) for _, (x, y, _) in zip(range(5), host)]
    print(f'captured on a bank batch {lg}\neager over the host windows {le}')
    assert np.isfinite(lg).all() and len(set(lg)) == 5 and lg == le
    for (k, p), (_, q) in zip(graphed.model.named_parameters(), eager.model.named_parameters()):
        assert torch.equal(p, q), k
