"""CPU-side checks of verify() (no GPU): every refusal of the request by name, before the loader is touched and before the library
launches anything; each product's own checks under its method's name; the product table against the eight methods; and
qtmpnn.verify.Verification (indexing, attribute access, order, its KeyError)."""
import inspect

import numpy as np
import pytest


class _Untouchable:
    """A loader that says its frame shape and must never be iterated."""

    def __init__(self, shape=(8, 12)):
        self.dataset = type('DS', (), {'image_shape': tuple(shape)})()

    def __iter__(self):
        raise AssertionError('the loader was touched before the products were checked')


@pytest.fixture(scope='module')
def nfp():
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=4, device='cpu',
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


@pytest.fixture
def launched(monkeypatch):
    from qtmpnn import _lib
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda *a: calls.append(a[0]))
    return calls


NAMES = ('predict', 'score', 'score_maps', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')


def test_the_table_covers_exactly_the_eight_methods():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    assert tuple(mpnnlstm.PRODUCTS) == NAMES
    assert mpnnlstm.DEFAULT_PRODUCTS == ('score', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')
    want = {'predict': (), 'score': ('threshold',), 'score_maps': ('threshold',), 'reliability': ('threshold', 'bins'),
            'fss': ('threshold', 'scales'), 'edge_distance': ('threshold',),
            'extent': ('threshold', 'regions', 'areas', 'region_names'), 'event_dates': ('threshold', 'kind', 'persist')}
    for name, row in mpnnlstm.PRODUCTS.items():
        assert issubclass(row, mpnnlstm.Product) and callable(getattr(NextFramePredictorS2S, name))
        for entry in ('reduce', 'collect', 'finish'):
            assert callable(getattr(row, entry)), (name, entry)
        options = mpnnlstm.product_options(name)
        assert tuple(options) == want[name]
        # the keywords and defaults are the method's own, and the row's check-and-prepare takes exactly them
        method = inspect.signature(getattr(NextFramePredictorS2S, name)).parameters
        assert all(method[k].default == v or method[k].default is v for k, v in options.items())
        prepare = row.prepare if hasattr(row, 'prepare') else row.__init__
        assert list(inspect.signature(prepare).parameters)[3:] == list(options), name
    assert mpnnlstm.PRODUCTS['predict'].reads_y is False and all(mpnnlstm.PRODUCTS[n].reads_y for n in NAMES[1:])
    # only score_maps has something to do before every batch
    assert [n for n in NAMES if mpnnlstm.PRODUCTS[n].begin is not None] == ['score_maps']


def test_verify_and_its_maker_sit_beside_score():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    verify = inspect.signature(NextFramePredictorS2S.verify).parameters
    assert list(verify) == [k for k in score if k != 'threshold'] + ['products']
    for name in verify:
        if name != 'products':
            assert verify[name].default == score[name].default, name
    assert verify['products'].default == mpnnlstm.DEFAULT_PRODUCTS
    scores = inspect.signature(NextFramePredictorS2S.make_graphed_scores).parameters
    maker = inspect.signature(NextFramePredictorS2S.make_graphed_verification).parameters
    assert list(maker) == [k for k in scores if k not in ('threshold', 'maps')] + ['products']
    assert maker['products'].default == mpnnlstm.DEFAULT_PRODUCTS
    assert list(inspect.signature(mpnnlstm.reference_frames).parameters) == ['image_shape', 'mask']


REQUEST_REFUSALS = [
    ((), 'verify: products is empty'),
    ({}, 'verify: products is empty'),
    (['score', 'sharpness'], "verify: unknown product 'sharpness'"),
    ({'score': {}, 'Score': {}}, "verify: unknown product 'Score'"),
    ([('score', 'fss')], r"verify: unknown product \('score', 'fss'\)"),
    (['fss', 'score', 'fss'], "verify: product 'fss' is given twice"),
    ({'fss': dict(bins=7)}, "verify: product 'fss' takes no keyword 'bins'"),
    ({'predict': dict(threshold=0.5)}, "verify: product 'predict' takes no keyword 'threshold'"),
    ({'score': dict(use_graph=True)}, "verify: product 'score' takes no keyword 'use_graph'"),
    ({'extent': dict(mask=None)}, "verify: product 'extent' takes no keyword 'mask'"),
    ({'score': 0.5}, "verify: the keywords of product 'score' must be a dict"),
    ('score', 'verify: products must be a sequence'),
    (3, 'verify: products must be a sequence'),
]


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('products, message', REQUEST_REFUSALS)
def test_verify_refuses_the_request_by_name(nfp, launched, products, message, use_graph):
    with pytest.raises(ValueError, match=message):
        nfp.verify(_Untouchable(), products=products, use_graph=use_graph)
    assert launched == [] and nfp.model.static_shapes is False


def _bad_areas():
    a = np.ones((8, 12))
    a[2, 3] = -0.5
    return a


PRODUCT_REFUSALS = [
    ({'reliability': dict(bins=1)}, 'reliability: bins must be an integer in 2..32'),
    ({'reliability': dict(bins=7.0)}, 'reliability: bins must be an integer in 2..32'),
    ({'fss': dict(scales=(1, 4))}, 'fss: scales must be odd'),
    ({'fss': dict(scales=())}, 'fss: scales is empty'),
    ({'fss': dict(scales=(5, 3))}, 'fss: scales must be strictly increasing'),
    ({'extent': dict(regions=np.zeros((12, 8), np.int64))}, 'extent: regions of shape .12, 8. for frames of .8, 12.'),
    ({'extent': dict(areas=_bad_areas())}, 'extent: areas must not be negative'),
    ({'extent': dict(regions=np.full((8, 12), 32))}, 'extent: regions name 33 regions'),
    ({'extent': dict(regions=np.arange(96).reshape(8, 12) % 3, region_names=('a', 'b'))},
     'extent: region_names must be 3 distinct names'),
    ({'event_dates': dict(kind='melt', persist=2)}, 'event_dates: kind must be one of'),
    ({'event_dates': dict(persist=0)}, 'event_dates: persist must be an integer in 1..4'),
    ({'event_dates': dict(persist=5)}, 'event_dates: persist must be an integer in 1..4'),
    ({'event_dates': dict(persist=2.0)}, 'event_dates: persist must be an integer in 1..4'),
    # the default persist = 5 does not fit four output steps: refused as event_dates() itself refuses it
    (['score', 'event_dates'], 'event_dates: persist must be an integer in 1..4'),
    # a fault in a later product is found before the first batch too
    ({'score': {}, 'fss': {}, 'reliability': dict(bins=33)}, 'reliability: bins must be an integer in 2..32'),
]


@pytest.mark.parametrize('products, message', PRODUCT_REFUSALS)
def test_every_product_is_checked_as_its_method_checks_it(nfp, launched, products, message):
    with pytest.raises(ValueError, match=message):
        nfp.verify(_Untouchable(), products=products)
    # the message names the product's method, and that method refuses the same options with the same words
    name = message.split(':')[0]
    options = products[name] if isinstance(products, dict) else {}
    with pytest.raises(ValueError, match=message):
        getattr(nfp, name)(_Untouchable(), **options)
    assert launched == []


def test_the_request_is_judged_before_any_product(nfp, launched):
    """An unknown name after a product with a bad option: the request's own fault is reported."""
    with pytest.raises(ValueError, match="verify: unknown product 'nope'"):
        nfp.verify(_Untouchable(), products={'reliability': dict(bins=1), 'nope': {}})
    assert launched == []


def test_a_good_request_reaches_the_loader(nfp, launched):
    """The checks pass, so the loop starts: the first thing it does is iterate the loader."""
    with pytest.raises(AssertionError, match='the loader was touched'):
        nfp.verify(_Untouchable(), products={'score': dict(threshold=0.5), 'fss': dict(scales=(1, 3)), 'reliability': None,
                                             'event_dates': dict(persist=4), 'extent': dict(areas=np.ones((8, 12)))})
    assert launched == [] and nfp.model.static_shapes is False


def test_maker_checks_the_same_request(nfp, launched):
    import torch
    x, y = torch.zeros(2, 2, 8, 12, 1), torch.zeros(2, 4, 8, 12, 1)
    with pytest.raises(ValueError, match="make_graphed_verification: unknown product 'nope'"):
        nfp.make_graphed_verification(x, y, products=['nope'])
    with pytest.raises(ValueError, match='make_graphed_verification: products is empty'):
        nfp.make_graphed_verification(x, y, products=[])
    with pytest.raises(ValueError, match='extent: regions of shape .4, 4. for frames of .8, 12.'):
        nfp.make_graphed_verification(x, y, products={'extent': dict(regions=np.zeros((4, 4), np.int64))})
    with pytest.raises(ValueError, match='event_dates: persist must be'):
        nfp.make_graphed_verification(x, y)
    assert launched == [] and nfp.model.static_shapes is False


def test_verification_container():
    from qtmpnn.verify import Verification
    fss, score, frames = object(), object(), np.zeros((2, 3))
    v = Verification({'fss': fss, 'score': score, 'predict': frames}, ('model', 'persistence'))
    assert v.products == ('fss', 'score', 'predict') and v.sources == ('model', 'persistence')
    assert v['fss'] is fss and v.fss is fss and v['score'] is score and v.score is score and v.predict is frames
    assert list(v) == ['fss', 'score', 'predict'] and len(v) == 3
    assert 'fss' in v and 'extent' not in v and 3 not in v
    assert [k for k, _ in v.items()] == list(v.products)
    with pytest.raises(KeyError, match=r"no product 'extent': this verification computed \('fss', 'score', 'predict'\)"):
        v['extent']
    with pytest.raises(KeyError, match='this verification computed'):
        v[0]
    with pytest.raises(AttributeError, match=r"no product 'extent': this verification computed \('fss', 'score', 'predict'\)"):
        v.extent
    assert not hasattr(v, 'by_lead') and not hasattr(v, 'rmse')        # no metric logic of its own
    assert repr(v) == "Verification(products=('fss', 'score', 'predict'), sources=('model', 'persistence'))"
    # order is the order given
    assert Verification({'score': score, 'fss': fss}, ()).products == ('score', 'fss')
    # copies survive (no recursion through __getattr__ on an empty instance)
    import copy
    import pickle
    assert copy.copy(v).products == v.products
    assert pickle.loads(pickle.dumps(Verification({'a': 1}, ('model',)))).a == 1
