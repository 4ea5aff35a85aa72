"""references= on the GPU: the defaults did not move, the anomaly-persistence sources of every product against the product's own
restatement fed the restated float32 field (tests/baselines_restated.py), damping 0 against climatology, eager / captured /
verify agreement, a Monitor on an anomaly reference, and ClipBank.anomaly_autocorrelation as a damping.

64 x 64 frames, hidden size 8, 3 input and 4 output steps; a batch of 3 clips of distinct launch dates (31 December of a leap
year, 1 January, mid-July), a single clip, and the 3-clip batch again (a replay of its capture).  All data are multiples of 1/64
and the dampings multiples of 1/8: every anomaly field is a multiple of 1/512 and lies at least 1/2560 from the threshold
0.15, so no one-ulp difference can flip a class (asserted below), and the comparisons are those of each product's own GPU test."""
import datetime
import functools

import numpy as np
import pytest
import torch

import baselines_restated as R
from edges_restated import restated_edges
from events_restated import restated_events
from extent_restated import restated_extent
from fss_restated import restated_fss
from helpers import TinyLoader, dev
from reliability_restated import restated_reliability
from score_restated import restated_sums

pytestmark = pytest.mark.gpu

T_IN, T_OUT, W, H, THR = 3, 4, 64, 64, 0.15
EPS = 16 * 2.0 ** -24                       # the float-slot bound of tests/test_gpu_score.py, test_gpu_reliability.py, test_gpu_extent.py
OPTIONS = {'score': {}, 'score_maps': {}, 'reliability': dict(bins=5), 'fss': dict(scales=(1, 3, 9)), 'edge_distance': {},
           'extent': {}, 'event_dates': dict(persist=2)}


def _stamp(y, m, d):
    return int(datetime.datetime(y, m, d).timestamp() * 1e9)


DATES3 = [_stamp(2016, 12, 31), _stamp(2017, 1, 1), _stamp(2017, 7, 14)]
DATE1 = _stamp(2018, 3, 1)


def _grid(rng, shape, top=64):
    return (rng.integers(0, top + 1, shape) / 64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _data():
    """(loader items, climatology (1, 366, 64, 64) in [0, 1], r4 (4,), r4p (4, 64, 64)): smooth-ish blobs so that edges exist."""
    rng = np.random.default_rng(21)
    ii, jj = np.mgrid[:W, :H]
    clim = np.stack([np.round(32 + 30 * np.sin(ii / 9.0 + d / 20.0) * np.cos(jj / 7.0 - d / 31.0)) / 64 for d in range(366)])
    clim = clim.astype(np.float32)[None]
    assert clim.min() >= 0 and clim.max() <= 1

    def clips(B, seed):
        r = np.random.default_rng(seed)
        base = np.stack([np.round(32 + 30 * np.sin((ii + r.integers(40)) / 8.0) * np.cos((jj + r.integers(40)) / 6.0)) for _ in range(B)])
        x = np.stack([np.clip(base + r.integers(-6, 7, base.shape), 0, 64) / 64 for _ in range(T_IN)], axis=1)
        y = np.stack([np.clip(np.roll(base, 2 * (t + 1), axis=1) + r.integers(-6, 7, base.shape), 0, 64) / 64 for t in range(T_OUT)], axis=1)
        return x.astype(np.float32)[..., None], y.astype(np.float32)[..., None]
    items = []
    for B, seed, dates in ((3, 1, DATES3), (1, 2, [DATE1]), (3, 3, DATES3[::-1])):
        x, y = clips(B, seed)
        items.append((torch.from_numpy(x), torch.from_numpy(y), torch.tensor(dates)))
    r4 = np.array([1.0, 0.75, 0.5, -0.125])
    r4p = (rng.integers(-8, 9, (T_OUT, W, H)) / 8.0)
    return items, clim, r4, r4p


def _mask():
    m = np.zeros((W, H), bool)
    m[:14, :20] = True
    m[np.random.default_rng(5).random((W, H)) < 0.04] = True
    return m


@functools.lru_cache(maxsize=None)
def _case(masked, conv='ChebConv'):
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(3)
    kw = dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2)
    if conv != 'ChebConv':
        kw['convolution_type'] = conv
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                model_kwargs=kw)
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    nfp.model.eval()
    items, clim, r4, r4p = _data()
    extra = dict(mask=_mask()) if masked else {}
    return nfp, TinyLoader(list(items), (W, H)), torch.from_numpy(clim).to(dev()), extra


def _references(pixel):
    from qtmpnn.baselines import AnomalyPersistence
    _, _, r4, r4p = _data()
    return ('anomaly_persistence', 'persistence', 'climatology', AnomalyPersistence(damping=r4p if pixel else r4))


def _arrays(name, res):
    """Every array of a product's result, by a name."""
    if name == 'event_dates':
        return {'dates': res.dates, 'sums': res.sums}
    out = {'sums': res.sums}
    if name == 'score_maps':
        out['maps'] = res.maps.sums
    return out


def _columns(name, res, source):
    """The arrays of one source of a product's result."""
    s = res.sources.index(source)
    if name == 'event_dates':
        return [res.dates[:, s]] + ([res.sums[:, s - 1]] if s else [])
    if name == 'extent':
        return [res.sums[:, :, :, 1 + s]]
    return [res.sums[:, :, s]] + ([res.maps.sums[:, s]] if name == 'score_maps' else [])


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _call(nfp, name, loader, clim, extra, **kw):
    return getattr(nfp, name)(loader, clim, **extra, **OPTIONS[name], **kw)


@pytest.mark.parametrize('masked', [False, True])
def test_defaults_did_not_move(masked):
    nfp, loader, clim, extra = _case(masked)
    for name in OPTIONS:
        plain = _call(nfp, name, loader, clim, extra)
        none = _call(nfp, name, loader, clim, extra, references=None)
        assert none.sources == plain.sources
        _same(_arrays(name, plain), _arrays(name, none), name)
        if name != 'event_dates':                       # (the event dates have no persistence by default)
            named = _call(nfp, name, loader, clim, extra, references=('persistence', 'climatology'))
            assert named.sources == plain.sources == ('model', 'persistence', 'climatology')
            _same(_arrays(name, plain), _arrays(name, named), name)
        else:
            named = _call(nfp, name, loader, clim, extra, references=('climatology',))
            assert named.sources == plain.sources == ('observed', 'model', 'climatology')
            _same(_arrays(name, plain), _arrays(name, named), name)
    bare = nfp.score(loader, None, **extra)
    _same(_arrays('score', bare), _arrays('score', nfp.score(loader, None, references=('persistence',), **extra)), 'no climatology')


def _clip_fields(nfp, loader, clim, extra, refs):
    """Per clip (x0, y (T, W, H), {source: (T, W, H) float32}) with the anomaly fields from the restatement; asserts that no
    pixel of a float64 anomaly field lies within 1e-5 of the threshold."""
    from qtmpnn.baselines import AnomalyPersistence
    frames = nfp.predict(loader, clim, **extra)
    climh = clim.cpu().numpy()[0]
    out, c = [], 0
    for x, y, dates in loader:
        for b in range(x.shape[0]):
            x0, d = x[b, -1, ..., 0].numpy(), int(dates[b])
            cc, c0 = climh[R.output_days(d, T_OUT)], climh[R.launch_day(d)]
            f = {'model': frames[c, ..., 0]}
            for spec in refs:
                if spec == 'persistence':
                    f[spec] = np.repeat(x0[None], T_OUT, axis=0)
                elif spec == 'climatology':
                    f[spec] = cc
                else:
                    spec = AnomalyPersistence() if spec == 'anomaly_persistence' else spec
                    f[spec.name] = R.field32(cc, x0, c0, spec.damping, spec.clip)
                    f64 = R.field64(cc, x0, c0, spec.damping, spec.clip)
                    assert np.abs(f64 - THR).min() > 1e-5, 'a pixel of the field lies at the threshold'
                    assert np.array_equal(f[spec.name], f64.astype(np.float32))
            out.append((x0, y[b, ..., 0].numpy(), f))
            c += 1
    return out


@pytest.mark.parametrize('masked, pixel', [(False, False), (True, True)])
def test_new_sources_are_right(masked, pixel):
    nfp, loader, clim, extra = _case(masked)
    refs = _references(pixel)
    names = ('anomaly_persistence', 'persistence', 'climatology', 'damped_anomaly_persistence')
    mask = extra.get('mask')
    clips = _clip_fields(nfp, loader, clim, extra, refs)
    new = ('anomaly_persistence', 'damped_anomaly_persistence')
    assert not np.array_equal(clips[0][2][new[0]], clips[0][2][new[1]]) and not np.array_equal(clips[0][2][new[0]], clips[0][2]['climatology'])
    for name in OPTIONS:
        plain = _call(nfp, name, loader, clim, extra)
        got = _call(nfp, name, loader, clim, extra, references=refs)
        lead = ('observed', 'model') if name == 'event_dates' else ('model',)
        assert got.sources == lead + names, name
        for source in plain.sources:
            for a, b in zip(_columns(name, got, source), _columns(name, plain, source)):
                assert np.array_equal(a, b, equal_nan=True), (name, source)
        for source in new:
            for c, (x0, y, f) in enumerate(clips):
                field, s = f[source], got.sources.index(source)
                if name in ('score', 'score_maps'):
                    want, absterms = restated_sums(field, y, mask, THR)
                    col = got.sums[c, :, s]
                    np.testing.assert_array_equal(col[:, [0, 4, 5, 6, 7]], want[:, [0, 4, 5, 6, 7]], err_msg=f'{name} {source} clip {c}')
                    assert (np.abs(col[:, 1:4] - want[:, 1:4]) <= EPS * absterms).all(), (name, source, c)
                elif name == 'reliability':
                    want, absterms = restated_reliability(field, y, mask, THR, 5)
                    col = got.sums[c, :, s]
                    np.testing.assert_array_equal(col[..., :2], want[..., :2], err_msg=f'{name} {source} clip {c}')
                    assert (np.abs(col[..., 2:] - want[..., 2:]) <= EPS * absterms).all(), (name, source, c)
                elif name == 'fss':
                    np.testing.assert_array_equal(got.sums[c, :, s], restated_fss(field, y, mask, THR, (1, 3, 9), None))
                elif name == 'edge_distance':
                    np.testing.assert_array_equal(got.sums[c, :, s], restated_edges(field, y, mask, THR, None))
                elif name == 'extent':
                    counted = np.ones((W, H), bool) if mask is None else ~mask
                    want, absterms = restated_extent([field], y, counted, None, None, THR, 1)
                    col = np.stack([got.sums[c, :, :, 0], got.sums[c, :, :, 1 + s]], axis=2)       # (the truth's row and the source's)
                    np.testing.assert_array_equal(col[..., 0, 0], want[..., 0, 0])
                    assert (np.abs(col - want) <= EPS * absterms).all(), (name, source, c)
                else:
                    dates, sums = restated_events([{'observed': y, 'model': f['model'], source: field}], [x0], mask, THR, 'breakup', 2)
                    np.testing.assert_array_equal(got.dates[c, s], dates[0, 2], err_msg=f'{name} {source} clip {c}')
                    np.testing.assert_array_equal(got.sums[c, s - 1], sums[0, 1], err_msg=f'{name} {source} clip {c}')
        if name == 'score_maps':                        # the maps of a new source are the sums over its clips' pixels
            for source in new:
                s = got.sources.index(source)
                np.testing.assert_array_equal(got.maps.sums[:, s, 0].sum(axis=(-2, -1)), got.sums[:, :, s, 0].sum(axis=0))
                np.testing.assert_array_equal(got.maps.sums[:, s, 5].sum(axis=(-2, -1)), got.sums[:, :, s, 5].sum(axis=0))


def test_damping_zero_equals_climatology():
    from qtmpnn.baselines import AnomalyPersistence
    nfp, loader, clim, extra = _case(True)
    for zero in (np.zeros(4), np.zeros((4, W, H))):
        refs = (AnomalyPersistence(damping=zero, name='zero'), 'climatology')
        for name in OPTIONS:
            got = _call(nfp, name, loader, clim, extra, references=refs)
            for a, b in zip(_columns(name, got, 'zero'), _columns(name, got, 'climatology')):
                assert np.array_equal(a, b, equal_nan=True), name


@pytest.mark.parametrize('conv', ['ChebConv', 'TransformerConv'])
def test_eager_captured_and_verify_agree(conv):
    nfp, loader, clim, extra = _case(True, conv)
    refs = _references(True)
    nfp.model.static_shapes = True
    own = {name: _call(nfp, name, loader, clim, extra, references=refs) for name in OPTIONS}
    nfp.model.static_shapes = False
    for name in OPTIONS:                                # three batches, two shapes: the third batch replays the first's capture
        graphed = _call(nfp, name, loader, clim, extra, references=refs, use_graph=True)
        assert graphed.sources == own[name].sources and nfp.model.static_shapes is False
        _same(_arrays(name, own[name]), _arrays(name, graphed), f'graphed {name}')
    # ('score' and 'score_maps' return the same class; the first list holds one and the second the other, with more products)
    for products in ({'score': {}, 'fss': OPTIONS['fss']}, {name: OPTIONS[name] for name in OPTIONS if name != 'score'}):
        _verify_agrees(nfp, loader, clim, extra, refs, products, own)
    # a product's own references go before the call's
    nfp.model.static_shapes = True
    v = nfp.verify(loader, clim, products={'fss': dict(OPTIONS['fss'], references=('climatology',)), 'extent': {}}, references=refs, **extra)
    nfp.model.static_shapes = False
    assert v.fss.sources == ('model', 'climatology') and v.extent.sources == own['extent'].sources
    _same(_arrays('extent', own['extent']), _arrays('extent', v.extent), 'extent beside an fss of its own')


def _verify_agrees(nfp, loader, clim, extra, refs, products, own):
    for use_graph in (False, True):
        nfp.model.static_shapes = not use_graph
        v = nfp.verify(loader, clim, products=products, references=refs, use_graph=use_graph, **extra)
        nfp.model.static_shapes = False
        assert v.sources == own['fss'].sources and v.products == tuple(products)
        for name in products:
            _same(_arrays(name, own[name]), _arrays(name, v[name]), f'verify {name} graph={use_graph}')


def test_graphed_verification_maker_agrees():
    from model.mpnnlstm import split_event_buffer
    nfp, loader, clim, extra = _case(True)
    refs = _references(False)
    names = ('score', 'fss', 'extent', 'event_dates')
    nfp.model.static_shapes = True
    own = {name: _call(nfp, name, loader, clim, extra, references=refs) for name in names}
    batches = [(x.to(dev()), y.to(dev()), nfp.get_climatology_array(clim, d), nfp.get_launch_climatology(clim, d)) for x, y, d in loader]
    try:
        replay = nfp.make_graphed_verification(batches[0][0], batches[0][1], batches[0][2], products={n: OPTIONS[n] for n in names},
                                               references=refs, launch_climatology=batches[0][3], **extra)
        for which, (lo, hi) in ((0, (0, 3)), (2, (4, 7))):
            out = replay.warmup if which == 0 else replay(*batches[which])
            for name, part in zip(names, out):
                part = part.cpu().numpy()
                if name == 'event_dates':
                    dates, sums = split_event_buffer(part, 3, len(own[name].sources), (W, H))
                    assert np.array_equal(dates, own[name].dates[lo:hi]) and np.array_equal(sums, own[name].sums[lo:hi])
                else:
                    assert np.array_equal(np.moveaxis(part, 0, 1), own[name].sums[lo:hi]), (name, which)
    finally:
        nfp.model.static_shapes = False


def test_monitor_reads_an_anomaly_reference(tmp_path, monkeypatch):
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn.validation import Monitor
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(4)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2))
    items, climh, _, _ = _data()
    loader = TinyLoader([items[1], items[1]], (W, H))
    clim = torch.from_numpy(climh).to(dev())
    seen = []

    def value(v):
        assert v.extent.sources == ('model', 'anomaly_persistence')
        seen.append(v.extent.skill('model', reference='anomaly_persistence'))
        assert nfp._asked == (None, None)
        return float(np.nanmean(v.extent.iiee('model')))
    nfp.train(loader, loader, clim, n_epochs=2, monitor=Monitor({'extent': dict(references=('anomaly_persistence',))}, value))
    assert len(nfp.monitor_history) == 2 and np.isfinite(nfp.monitor_history).all()
    assert len(seen) == 2 and all(s.shape == (T_OUT,) for s in seen)


def test_bank_autocorrelation_feeds_a_forecast():
    from qtmpnn.baselines import AnomalyPersistence
    from qtmpnn.data import ClipBank
    rng = np.random.default_rng(8)
    D = 30
    series = _grid(rng, (D, W, H, 1))
    times = np.array([_stamp(2019, 12, 20) + R.DAY * d for d in range(15)] + [_stamp(2020, 12, 19) + R.DAY * d for d in range(15)])
    segments = [(0, 15), (15, 30)]
    gpu = ClipBank(series, times, T_IN, T_OUT, segments=segments, device=dev())
    cpu = ClipBank(series, times, T_IN, T_OUT, segments=segments, device='cpu')
    r = gpu.anomaly_autocorrelation(4)
    assert r.is_cuda and r.shape == (1, 4, W, H) and torch.equal(r.cpu(), cpu.anomaly_autocorrelation(4))
    assert float(r.abs().max()) > 0.1
    nfp, _, _, extra = _case(False)
    sc = nfp.score(gpu.loader(batch_size=2), gpu.normals(), references=(AnomalyPersistence(damping=r[0]),))
    assert sc.sources == ('model', 'damped_anomaly_persistence') and np.isfinite(sc.rmse('damped_anomaly_persistence')).all()
