"""verify(): every verification product from ONE rollout per batch (NextFramePredictorS2S.verify, make_graphed_verification).
No kernel of its own, so the reference of every product is the product's own method: called with the same options and the same
`use_graph`, it must return the same bits, array by array, whatever else shares the rollout and in whatever order.  What gates the
change is structural: the number of model forwards (one per batch eagerly, two per distinct graph key captured) and of captures.

The case is the suite's smallest: tests/test_gpu_extent.py's 64 x 64 quadtree model with a land mask, in eval() mode -- batches of
2, 2 and 1 clips (two distinct batch shapes) without a climatology, its first three clips one by one with one."""
import functools

import numpy as np
import pytest
import torch

from helpers import TinyLoader, dev
from test_gpu_extent import NAMES, _maps64, _reference

pytestmark = pytest.mark.gpu

ALL = ('predict', 'score', 'score_maps', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')


@functools.lru_cache(maxsize=None)
def _options():
    """Non-default options for every product that has any: made once, not modified."""
    regions, areas = _maps64(None)
    return {'predict': {}, 'score': dict(threshold=0.2), 'score_maps': {}, 'reliability': dict(bins=7),
            'fss': dict(scales=(1, 5, 9)), 'edge_distance': dict(threshold=0.25),
            'extent': dict(regions=regions, areas=areas, region_names=NAMES), 'event_dates': dict(kind='freezeup', persist=2)}


def _arrays(name, result):
    """{what: array or tuple} of a product's result: everything the loop computed for it."""
    if name == 'predict':
        return {'frames': result}
    out = {'sums': result.sums, 'sources': result.sources}
    if name == 'score':
        assert result.maps is None
    if name == 'score_maps':
        out.update(maps=result.maps.sums, map_sources=result.maps.sources)
    if name == 'extent':
        out.update(region_names=result.region_names)
    if name == 'event_dates':
        out.update(dates=result.dates, kind=result.kind, persist=result.persist)
    if name == 'fss':
        out.update(scales=result.scales)
    if hasattr(result, 'threshold'):
        out.update(threshold=result.threshold)
    return out


def _assert_same(name, got, want, what=''):
    assert type(got) is type(want), (name, type(got), type(want))
    a, b = _arrays(name, got), _arrays(name, want)
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k, what)
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), (name, k, what)
        else:
            assert a[k] == b[k], (name, k, what)


@functools.lru_cache(maxsize=None)
def _own(with_clim, use_graph):
    """{name: result} of every product's own method, one call (one pass over the loader) each: made once, not modified."""
    nfp, loader, clim, extra, _ = _reference(with_clim)
    return {name: getattr(nfp, name)(loader, clim, use_graph=use_graph, **extra, **opts) for name, opts in _options().items()}


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('with_clim', [False, True])
def test_every_product_equals_its_own_method_bit_for_bit(with_clim, use_graph):
    from qtmpnn.verify import Verification
    nfp, loader, clim, extra, _ = _reference(with_clim)
    assert not nfp.model.training and len({tuple(item[0].shape) for item in loader}) == (1 if with_clim else 2)
    v = nfp.verify(loader, clim, use_graph=use_graph, products=_options(), **extra)
    assert isinstance(v, Verification) and v.products == ALL and nfp.model.static_shapes is False
    assert v.sources == ('model', 'persistence') + (('climatology',) if with_clim else ())
    own = _own(with_clim, use_graph)
    for name in ALL:
        _assert_same(name, v[name], own[name], f'clim={with_clim} graph={use_graph}')
        assert getattr(v, name) is v[name]
    # the comparison has something to compare: counted pixels, events found, frames that are not all alike
    assert v.score.sums[..., 0].min() > 0 and v.score_maps.maps.sums[:, :, 0].max() == len(v.score.sums)
    assert (v.event_dates.dates >= 0).any() and v.event_dates.sources[0] == 'observed'
    assert v.predict.shape == (len(v.score.sums), nfp.output_timesteps, 64, 64, 1) and np.nanstd(v.predict) > 0
    assert v.extent.sums.shape[2] == 3 and v.fss.sums.shape[3] == 3 and v.reliability.sums.shape[3] == 7
    # score and score_maps are two products with two thresholds: same n, other ice tables
    assert np.array_equal(v.score.sums[..., 0], v.score_maps.sums[..., 0]) and not np.array_equal(v.score.sums, v.score_maps.sums)


def test_defaults_are_the_six_report_products():
    """A sequence of names runs every product with its method's defaults; the default request is the six sums products."""
    nfp, loader, clim, extra, _ = _reference(False)
    v = nfp.verify(loader, clim, products=('score', 'reliability', 'fss', 'edge_distance', 'extent'), **extra)
    for name in v:
        _assert_same(name, v[name], getattr(nfp, name)(loader, clim, **extra), 'defaults')
    # event_dates' default persist = 5 exceeds the four output steps of this model: refused as event_dates() refuses it
    with pytest.raises(ValueError, match='event_dates: persist must be an integer in 1..4'):
        nfp.verify(loader, clim, **extra)


def _counted(monkeypatch, nfp):
    """Counters of nfp.model.forward and nfp._graphed_product."""
    n = {'forward': 0, 'captures': 0}
    forward, capture = nfp.model.forward, nfp._graphed_product

    def counting_forward(*a, **k):
        n['forward'] += 1
        return forward(*a, **k)

    def counting_capture(*a, **k):
        n['captures'] += 1
        return capture(*a, **k)
    monkeypatch.setattr(nfp.model, 'forward', counting_forward)
    monkeypatch.setattr(nfp, '_graphed_product', counting_capture)
    return n


def test_one_rollout_per_batch(monkeypatch):
    nfp, loader, clim, extra, _ = _reference(False)
    n = _counted(monkeypatch, nfp)
    batches, keys, k = len(loader), len({tuple(item[0].shape) for item in loader}), len(ALL)
    assert (batches, keys) == (3, 2)
    nfp.verify(loader, clim, products=_options(), **extra)
    assert n == {'forward': batches, 'captures': 0}
    # the separate calls: one rollout per product and batch
    n.update(forward=0)
    for name in ('score', 'fss', 'edge_distance'):
        getattr(nfp, name)(loader, clim, **extra, **_options()[name])
    assert n == {'forward': 3 * batches, 'captures': 0}
    # graphed: the warm-up and the capture of each distinct key, one capture per key whatever the number of products
    n.update(forward=0)
    nfp.verify(loader, clim, use_graph=True, products=_options(), **extra)
    assert n == {'forward': 2 * keys, 'captures': keys} and k == 8
    n.update(forward=0, captures=0)
    nfp.verify(loader, clim, use_graph=True, products=('score',), **extra)
    assert n == {'forward': 2 * keys, 'captures': keys}
    # predict alone reads no y, so y is no part of its key: two batches of one x shape whose y differ in shape are one capture
    n.update(forward=0, captures=0)
    other_y = TinyLoader([loader[0], (loader[1][0], loader[1][1][:, :2], loader[1][2])], loader.dataset.image_shape)
    nfp.verify(other_y, clim, use_graph=True, products=('predict',), **extra)
    assert n == {'forward': 2, 'captures': 1}


@pytest.mark.parametrize('use_graph', [False, True])
def test_order_of_the_products_changes_nothing(use_graph):
    nfp, loader, clim, extra, _ = _reference(True)
    backwards = dict(reversed(list(_options().items())))
    v = nfp.verify(loader, clim, use_graph=use_graph, products=backwards, **extra)
    assert v.products == ALL[::-1] and list(v) == list(ALL[::-1])
    own = _own(True, use_graph)
    for name in ALL:
        _assert_same(name, v[name], own[name], f'reversed graph={use_graph}')


@pytest.mark.parametrize('use_graph', [False, True])
def test_score_maps_inside_verify(use_graph):
    """Every batch is added exactly once (warm-up and capture of a key add its batch once, a replay once), a second call starts
    from zeros, and the one-grid rule still holds."""
    nfp, loader, clim, extra, _ = _reference(False)
    want = _own(False, use_graph)['score_maps']
    for attempt in range(2):
        v = nfp.verify(loader, clim, use_graph=use_graph, products=('score_maps', 'fss'), **extra)
        _assert_same('score_maps', v.score_maps, want, f'call {attempt}')
    n = v.score_maps.maps.sums[:, :, 0]
    assert n.max() == 5 and set(np.unique(n)) == {0.0, 5.0}              # five clips, masked pixels never counted
    other_grid = TinyLoader([loader[0], tuple(t[:, :, :32] if t.dim() == 5 else t for t in loader[1])], (64, 64))
    with pytest.raises(ValueError, match=r'score_maps: a batch of \(32, 64\) frames after \(64, 64\) ones'):
        nfp.verify(other_grid, clim, use_graph=use_graph, products=('fss', 'score_maps'), **extra)
    assert nfp.model.static_shapes is False


def test_make_graphed_verification():
    nfp, loader, clim, extra, _ = _reference(False)
    opts = _options()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    static0 = nfp.model.static_shapes
    try:
        replay = nfp.make_graphed_verification(x, y, products=opts, **extra)
        assert replay.products == ALL and isinstance(replay.warmup, tuple) and len(replay.warmup) == len(ALL)
        warm = [t.clone() for t in replay.warmup]
        maps_once = replay.maps.clone()
        again = replay(x, y)
        assert isinstance(again, tuple) and len(again) == len(ALL)
        for name, w, r in zip(ALL, warm, again):
            assert w.dtype == r.dtype and w.shape == r.shape, name
            assert np.array_equal(w.cpu().numpy(), r.cpu().numpy(), equal_nan=True), name
        # warm-up once, the replay once: the counts (slots 0 and 4-7) have doubled; the float sums are running sums, ((s + c1) + c2)
        # and not 2 s, and are compared with make_graphed_scores' buffer below
        counts = [0, 4, 5, 6, 7]
        assert torch.equal(replay.maps[:, :, counts], 2 * maps_once[:, :, counts]) and maps_once[:, :, 0].max() == x.shape[0]
        maps = torch.zeros_like(maps_once)
        makers = {'predict': nfp.make_graphed_rollout(x, **extra),
                  'score': nfp.make_graphed_scores(x, y, threshold=0.2, **extra),
                  'score_maps': nfp.make_graphed_scores(x, y, maps=maps, **extra),
                  'reliability': nfp.make_graphed_reliability(x, y, bins=7, **extra),
                  'fss': nfp.make_graphed_fss(x, y, scales=(1, 5, 9), **extra),
                  'edge_distance': nfp.make_graphed_edges(x, y, threshold=0.25, **extra),
                  'extent': nfp.make_graphed_extent(x, y, regions=opts['extent']['regions'], areas=opts['extent']['areas'],
                                                     **extra),
                  'event_dates': nfp.make_graphed_events(x, y, kind='freezeup', persist=2, **extra)}
        for name, w in zip(ALL, warm):
            one = makers[name]
            got = one(x) if name == 'predict' else one(x, y)
            for what, t in (('warm-up', one.warmup), ('replay', got)):
                assert t.dtype == w.dtype and t.shape == w.shape, (name, what)
                assert np.array_equal(t.cpu().numpy(), w.cpu().numpy(), equal_nan=True), (name, what)
        assert torch.equal(maps, replay.maps)                                          # two additions of the batch each
        # a second batch shape is a second maker; a replay of another batch of this shape equals its own makers' too
        x2, y2, _ = loader[1]
        x2, y2 = x2.to(dev()), y2.to(dev())
        second = [t.clone() for t in replay(x2, y2)]
        assert np.array_equal(second[ALL.index('fss')].cpu().numpy(), makers['fss'](x2, y2).cpu().numpy())
        assert not np.array_equal(second[ALL.index('fss')].cpu().numpy(), warm[ALL.index('fss')].cpu().numpy())
    finally:
        nfp.model.static_shapes = static0


@pytest.mark.parametrize('use_graph', [False, True])
def test_an_exception_of_a_product_leaves_the_predictor_usable(monkeypatch, use_graph):
    from model import mpnnlstm
    nfp, loader, clim, extra, _ = _reference(False)
    collect, seen = mpnnlstm.PRODUCTS['fss'].collect, []

    def failing(self, part, x):
        seen.append(tuple(x.shape))
        if len(seen) == 2:
            raise RuntimeError('the host ran out of patience')
        return collect(self, part, x)
    with monkeypatch.context() as m:
        m.setattr(mpnnlstm.PRODUCTS['fss'], 'collect', failing)
        with pytest.raises(RuntimeError, match='out of patience'):
            nfp.verify(loader, clim, use_graph=use_graph, products=('score', 'fss', 'edge_distance'), **extra)
    assert len(seen) == 2 and nfp.model.static_shapes is False
    v = nfp.verify(loader, clim, use_graph=use_graph, products={'fss': _options()['fss']}, **extra)
    _assert_same('fss', v.fss, _own(False, use_graph)['fss'], 'after the exception')
