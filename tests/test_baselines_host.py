"""references=, host side (no GPU): the launch-state day and its climatology against the calendar, get_climatology_array's
return values unchanged, the anomaly-persistence field against the numpy restatement (tests/baselines_restated.py), damping 0,
ClipBank.anomaly_autocorrelation against the loop model, every refusal by exception type and argument name before anything
is launched, the source order and the launch chunking, and the entry-point count."""
import datetime

import numpy as np
import pytest
import torch

import baselines_restated as R

T_OUT, W, H = 4, 8, 12


def _stamp(y, m, d):
    return int(datetime.datetime(y, m, d).timestamp() * 1e9)


# a mid-year date, 1 January after a leap year and after a common year, 1 March of a leap year
DATES = np.array([_stamp(2019, 7, 14), _stamp(2017, 1, 1), _stamp(2018, 1, 1), _stamp(2020, 3, 1)], dtype=np.int64)
WANT_LAUNCH_DAY = [193, 365, 364, 59]


class _Untouchable:
    def __init__(self, shape=(W, H)):
        self.dataset = type('DS', (), {'image_shape': tuple(shape)})()

    def __iter__(self):
        raise AssertionError('the loader was touched before the references were checked')


@pytest.fixture(scope='module')
def nfp():
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_OUT, device='cpu',
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


def _climatology(seed=0, Cy=1):
    return torch.from_numpy(np.random.default_rng(seed).random((Cy, 366, W, H), dtype=np.float32))


def test_launch_day_rule_against_the_calendar(nfp):
    from model.utils import launch_day_index
    assert [R.launch_day(d) for d in DATES] == WANT_LAUNCH_DAY                 # (the restated rule, held to the known days)
    assert [launch_day_index(d) for d in DATES] == WANT_LAUNCH_DAY
    clim = _climatology()
    for d, want in zip(DATES, WANT_LAUNCH_DAY):
        got = nfp.get_launch_climatology(clim, torch.from_numpy(np.array([d])))
        assert got.shape == (W, H, 1) and torch.equal(got[..., 0], clim[0, want])
    batch = nfp.get_launch_climatology(clim, torch.from_numpy(DATES))
    assert batch.shape == (4, W, H, 1)
    for c, want in enumerate(WANT_LAUNCH_DAY):
        assert torch.equal(batch[c, ..., 0], clim[0, want])
    again = nfp.get_launch_climatology(clim, torch.from_numpy(DATES[[2, 0, 3, 1]]))
    assert torch.equal(again, batch[[2, 0, 3, 1]])
    two = _climatology(1, Cy=2)
    assert nfp.get_launch_climatology(two, torch.from_numpy(DATES[:3])).shape == (3, W, H, 2)


def test_output_climatology_is_what_it_was(nfp):
    """get_climatology_array against the restated gather, before and after the launch-state day was asked for."""
    clim = _climatology(2)

    def want(dates):
        return torch.stack([torch.stack([clim[0, i] for i in R.output_days(d, T_OUT)]) for d in dates])[..., None]
    one = nfp.get_climatology_array(clim, torch.from_numpy(DATES[1:2]))
    assert one.shape == (T_OUT, W, H, 1) and torch.equal(one, want(DATES[1:2])[0])
    before = nfp.get_climatology_array(clim, torch.from_numpy(DATES))
    nfp.get_launch_climatology(clim, torch.from_numpy(DATES))
    after = nfp.get_climatology_array(clim, torch.from_numpy(DATES))
    assert before.shape == (4, T_OUT, W, H, 1) and torch.equal(before, want(DATES)) and torch.equal(after, before)


def _field_inputs(B, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.random((B, 2, W, H, 1), dtype=np.float32)
    concat = rng.random((B, T_OUT, W, H, 1), dtype=np.float32)
    c0 = rng.random((B, W, H, 1), dtype=np.float32)
    return x, concat, c0


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('damping', [None, 'lead', 'pixel'])
@pytest.mark.parametrize('clip', [(0.0, 1.0), None, (0.2, 0.7)])
def test_field_arithmetic(B, damping, clip):
    from qtmpnn.baselines import AnomalyPersistence, check_references, reference_fields
    rng = np.random.default_rng(4)
    r = {None: None, 'lead': rng.uniform(-1, 1, T_OUT), 'pixel': rng.uniform(-1, 1, (T_OUT, W, H))}[damping]
    x, concat, c0 = _field_inputs(B)
    specs = check_references('test', [AnomalyPersistence(r, clip=clip), 'persistence', 'climatology'], True, T_OUT, (W, H))
    tx, tc, t0 = (torch.from_numpy(a) for a in (x, concat, c0))
    if B == 1:
        tx, tc, t0 = tx[0], tc[0], t0[0]
    fields = reference_fields(tx, tc, t0, specs)
    assert fields['persistence'].data_ptr() == tx[..., -1, :, :, 0].data_ptr() and fields['climatology'] is tc
    got = fields[specs[0]].numpy().reshape(B, T_OUT, W, H)
    assert got.dtype == np.float32
    # three roundings (d, r d, c + r d) of values no larger than the data allow: half an ulp each at the largest magnitude
    top = max(np.abs(concat).max() + np.abs(x[:, -1] - c0).max(), np.abs(x[:, -1] - c0).max(), 1.0)
    bound = 3 * 2.0 ** -24 * 2.0 ** np.ceil(np.log2(top))
    for b in range(B):
        args = (concat[b, ..., 0], x[b, -1, ..., 0], c0[b, ..., 0], r, clip)
        np.testing.assert_array_equal(got[b], R.field32(*args))
        assert np.abs(got[b] - R.field64(*args)).max() <= bound
    assert bound <= 3 * 2.0 ** -23


def test_damping_zero_is_the_clamped_climatology():
    from qtmpnn.baselines import AnomalyPersistence, check_references, reference_fields
    x, concat, c0 = _field_inputs(3, seed=5)
    concat = concat * 1.5 - 0.25                                    # (some of it outside [0, 1])
    for zero in (np.zeros(T_OUT), np.zeros((T_OUT, W, H)), -np.zeros(T_OUT)):
        specs = check_references('test', [AnomalyPersistence(zero)], True, T_OUT, (W, H))
        f = reference_fields(*(torch.from_numpy(a) for a in (x, concat, c0)), specs)[specs[0]]
        want = np.clip(concat[..., 0], np.float32(0), np.float32(1)).reshape(3, T_OUT, -1)
        assert np.array_equal(f.numpy().view(np.uint32), (want + np.float32(0)).view(np.uint32))


def _bank(segments, seed=6, D=40):
    from qtmpnn.data import ClipBank
    rng = np.random.default_rng(seed)
    series = rng.random((D, 3, 4, 2), dtype=np.float32)
    series[:, 1, 2, :] = 0.25                                       # a constant pixel: anomalies 0, denominator 0
    # two winters over the same calendar days (across a new year, the second after a leap day): most indices hold two days
    times = np.array([_stamp(2019, 12, 20) + R.DAY * d for d in range(17)]
                     + [_stamp(2020, 12, 18) + R.DAY * d for d in range(D - 17)], dtype=np.int64)
    return ClipBank(series, times, 2, 3, segments=segments, device='cpu'), series, times


@pytest.mark.parametrize('max_lag', [1, 3])
def test_autocorrelation_against_the_loop_model(max_lag):
    segments = [(0, 17), (17, 40)]                                  # two segments of unequal length
    bank, series, times = _bank(segments)
    for days in (None, [(0, 12), (17, 40)]):                        # the second selection cuts the first segment
        selected = np.zeros(40, bool)
        for s, e in (days or [(0, 40)]):
            selected[s:e] = True
        got = bank.anomaly_autocorrelation(max_lag, days=days)
        normals = bank.normals(days).numpy()
        want = R.autocorrelation(series, times, normals, segments, selected, max_lag)
        assert got.shape == (2, max_lag, 3, 4) and got.dtype == torch.float32
        # one float32 rounding of the float64 result (|r| <= 1), plus the float64 sums' own error, far below it
        assert np.abs(got.numpy() - want).max() <= 2.0 ** -24 + 1e-12
        assert (got[:, :, 1, 2] == 0).all() and (want[:, :, 1, 2] == 0).all()
        assert np.abs(got.numpy()).max() <= 1.0 and np.abs(got.numpy()).max() > 0.05
        assert torch.equal(got, bank.anomaly_autocorrelation(max_lag, days=days, normals=torch.from_numpy(normals)))
    mask = np.zeros(40, bool)
    mask[:12] = mask[17:] = True
    assert torch.equal(bank.anomaly_autocorrelation(max_lag, days=mask), got)


def test_autocorrelation_refuses_max_lag_by_name():
    bank, _, _ = _bank([(0, 17), (17, 40)])
    for bad in (0, -1, 2.0, '2', True, None, 17, 40):
        with pytest.raises(ValueError, match='^max_lag: '):
            bank.anomaly_autocorrelation(bad)
    with pytest.raises(ValueError, match='^max_lag: '):
        bank.anomaly_autocorrelation(12, days=[(0, 12), (17, 40)])
    assert bank.anomaly_autocorrelation(16).shape == (2, 16, 3, 4)
    with pytest.raises(ValueError, match='^days: '):
        bank.anomaly_autocorrelation(2, days=[(5, 3)])


def _refusals():
    from qtmpnn.baselines import AnomalyPersistence as AP
    nan = np.ones(T_OUT)
    nan[1] = np.nan
    inf = np.ones((T_OUT, W, H))
    inf[0, 0, 0] = np.inf
    return [
        ('persistence', TypeError, True), (3, TypeError, True), (AP(), TypeError, True), (['persistence', 3], TypeError, True),
        ([np.ones(T_OUT)], TypeError, True),
        ((), ValueError, True), ([], ValueError, True),
        (('persistence', 'persistence'), ValueError, True), (('anomaly_persistence', AP()), ValueError, True),
        ((AP(np.zeros(T_OUT)), AP(np.ones(T_OUT))), ValueError, True), ((AP(name='climatology'), 'climatology'), ValueError, True),
        (('model',), ValueError, True), (('observed',), ValueError, True), ((AP(name='model'),), ValueError, True),
        ((AP(name='observed'),), ValueError, True), (('damped',), ValueError, True), (('Persistence',), ValueError, True),
        (('climatology',), ValueError, False), (('anomaly_persistence',), ValueError, False), ((AP(),), ValueError, False),
        ((AP(np.ones(T_OUT + 1)),), ValueError, True), ((AP(np.ones((T_OUT, H, W))),), ValueError, True),
        ((AP(np.ones((1, T_OUT))),), ValueError, True), ((AP(0.5),), ValueError, True),
        ((AP(np.array(['a'] * T_OUT)),), ValueError, True), ((AP(np.ones(T_OUT, bool)),), ValueError, True),
        ((AP(np.ones(T_OUT, complex)),), ValueError, True), ((AP(nan),), ValueError, True), ((AP(inf),), ValueError, True),
        ((AP(np.full(T_OUT, 1.001)),), ValueError, True), ((AP(np.full(T_OUT, -1.5)),), ValueError, True),
        ((AP(clip=(1.0, 0.0)),), ValueError, True), ((AP(clip=(0.5, 0.5)),), ValueError, True),
        ((AP(clip=(0.0, np.inf)),), ValueError, True), ((AP(clip=(np.nan, 1.0)),), ValueError, True),
        ((AP(clip=0.5),), ValueError, True), ((AP(clip=(0.0, 0.5, 1.0)),), ValueError, True),
    ]


METHODS = ('score', 'score_maps', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates', 'verify')


@pytest.mark.parametrize('k', range(37))
def test_every_refusal_names_references_and_comes_before_any_launch(nfp, monkeypatch, k):
    from qtmpnn import _lib, ops
    from qtmpnn.baselines import check_references
    bad, error, with_clim = _refusals()[k]
    assert len(_refusals()) == 37

    def reached(*a, **kw):
        raise AssertionError('ops.rollout_scores was reached')
    launched = []
    monkeypatch.setattr(ops, 'rollout_scores', reached)
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    with pytest.raises(error, match='references'):
        check_references('score', bad, with_clim, T_OUT, (W, H))
    clim = _climatology() if with_clim else None
    for name in METHODS:
        kw = dict(persist=2) if name == 'event_dates' else dict(products=('score', 'fss')) if name == 'verify' else {}
        with pytest.raises(error, match=f'^{name}: references'):
            getattr(nfp, name)(_Untouchable(), clim, references=bad, **kw)
    with pytest.raises(error, match='^extent: references'):
        nfp.verify(_Untouchable(), clim, products={'score': {}, 'extent': dict(references=bad)})
    x, y = torch.zeros(2, 2, W, H, 1), torch.zeros(2, T_OUT, W, H, 1)
    concat = torch.zeros(2, T_OUT, W, H, 1) if with_clim else None
    with pytest.raises(error, match='^make_graphed_scores: references'):
        nfp.make_graphed_scores(x, y, concat, references=bad)
    with pytest.raises(error, match='^make_graphed_verification: references'):
        nfp.make_graphed_verification(x, y, concat, products=('score',), references=bad)
    assert launched == [] and nfp.model.static_shapes is False and nfp._asked == (None, None)


def test_good_references_reach_the_loader(nfp):
    from qtmpnn.baselines import AnomalyPersistence as AP
    refs = ('anomaly_persistence', 'persistence', 'climatology', AP(np.linspace(1, 0.2, T_OUT)), AP(np.zeros((T_OUT, W, H)), name='z'))
    for name in METHODS:
        kw = dict(persist=2) if name == 'event_dates' else dict(products=('score', 'extent')) if name == 'verify' else {}
        with pytest.raises(AssertionError, match='the loader was touched'):
            getattr(nfp, name)(_Untouchable(), _climatology(), references=refs, **kw)
    with pytest.raises(AssertionError, match='the loader was touched'):
        nfp.score(_Untouchable(), None, references=('persistence',))
    with pytest.raises(ValueError, match="verify: product 'predict' takes no keyword 'references'"):
        nfp.verify(_Untouchable(), products={'predict': dict(references=('persistence',))})
    with pytest.raises(ValueError, match='launch_climatology'):
        nfp.make_graphed_scores(torch.zeros(2, 2, W, H, 1), torch.zeros(2, T_OUT, W, H, 1), torch.zeros(2, T_OUT, W, H, 1),
                                references=('anomaly_persistence',))
    assert nfp.model.static_shapes is False


def test_a_call_inside_a_call_has_its_own_references(nfp):
    """A method called without references while another runs with them (a callback, a Monitor's value function) inherits
    none; launch_climatology belongs to the makers and is an unknown keyword elsewhere."""
    seen = []

    class _Calls:
        dataset = _Untouchable().dataset

        def __iter__(self):
            seen.append(nfp._asked)
            with pytest.raises(AssertionError, match='the loader was touched'):
                nfp.fss(_Untouchable(), _climatology())
            seen.append(nfp._asked)
            with pytest.raises(ValueError, match="^fss: references: unknown reference 'nope'"):
                nfp.fss(_Untouchable(), _climatology(), references=('nope',))
            raise KeyboardInterrupt('done')
    refs = ('climatology', 'anomaly_persistence')
    with pytest.raises(KeyboardInterrupt, match='done'):
        nfp.score(_Calls(), _climatology(), references=refs)
    assert seen == [(refs, None), (refs, None)] and nfp._asked == (None, None)
    for name in METHODS:
        with pytest.raises(TypeError, match='launch_climatology'):
            getattr(nfp, name)(_Untouchable(), _climatology(), launch_climatology=torch.zeros(W, H, 1))


def test_sources_and_launch_chunking():
    from model import mpnnlstm
    from qtmpnn import ops
    from qtmpnn.baselines import AnomalyPersistence as AP, check_references, default_references, forecast_sources, reference_launches
    assert mpnnlstm.forecast_sources is forecast_sources
    assert forecast_sources(False) == ('model', 'persistence') and forecast_sources(True) == ('model', 'persistence', 'climatology')
    assert default_references(True) == ('persistence', 'climatology')
    refs = check_references('t', ('climatology', AP(np.ones(T_OUT)), 'anomaly_persistence', 'persistence', AP(name='b')),
                            True, T_OUT, None)
    assert forecast_sources(True, refs) == ('model', 'climatology', 'damped_anomaly_persistence', 'anomaly_persistence',
                                            'persistence', 'b')
    assert reference_launches(0) == [(0, 0)]
    for k in range(1, 6):
        launches = reference_launches(k)
        assert len(launches) == -(k // -2) and launches == [(2 * i, min(2 * i + 2, k)) for i in range(len(launches))]
        # the helper every product goes through: launch i carries references 2 i and 2 i + 1, the model's row comes from launch 0
        named, seen = [(f'r{j}', torch.full((1,), float(j))) for j in range(k)], []

        def rollout(persistence=None, climatology=None):
            given = [t for t in (persistence, climatology) if t is not None]
            seen.append([name for name, _ in given])
            return torch.stack([torch.full((1,), -1.0 - len(seen))] + [t for _, t in given], dim=1)      # (1, 1 + n)
        out = ops.with_references(rollout, named, axis=1)
        assert seen == [[f'r{j}' for j in range(i, j2)] for i, j2 in launches]
        assert out.shape == (1, 1 + k) and out[0].tolist() == [-2.0] + [float(j) for j in range(k)]
        two = ops.with_references(lambda **slots: torch.zeros(1, 2 + len(slots)), named, axis=1, lead=2)
        assert two.shape == (1, 2 + k)
    assert ops.named_fields(None, None) == []
    t = torch.zeros(3)
    assert ops.named_fields(t, ('mine', t)) == [('persistence', t), ('mine', t)]


def test_static_batch_carries_the_launch_climatology():
    from model.mpnnlstm import StaticBatch, batch_shapes
    x, y, c, c0 = torch.rand(2, 3, 4, 4, 1), torch.rand(2, 5, 4, 4, 1), torch.rand(2, 5, 4, 4, 1), torch.rand(2, 4, 4, 1)
    assert StaticBatch(x, y, c).shapes == batch_shapes((x, y, c)) and len(StaticBatch(x, y, c, None).tensors) == 3
    full = StaticBatch(x, y, c, c0)
    assert full.shapes == batch_shapes((x, y, c, c0)) and full.shapes != StaticBatch(x, y, c).shapes
    full.load(2 * x, 3 * y, 4 * c, 5 * c0)
    assert torch.equal(full.tensors[3], 5 * c0) and full.tensors[3].data_ptr() != c0.data_ptr()
    with pytest.raises(TypeError):
        full.load(x, y, c)


def test_entry_point_count():
    from qtmpnn import _lib
    assert len(_lib.exported_names()) == 91
