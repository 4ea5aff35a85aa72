"""The rollout horizon on the host: the schedule of train(horizon=) as one pure function, the setting and its context manager,
what stays the built value (the checkpoint description), the per-(date, steps) cache of the climatology days, the refusals that
need no device -- each by message, each before a launch -- and train()'s bookkeeping around scripted steps: which horizon every
training batch and every test pass runs under, across two calls.  The ABI is what it was: the feature adds no entry point."""
import inspect

import numpy as np
import pytest
import torch

from helpers import TinyLoader

BUILT = 4

TRAIN_PARAMETERS = ['self', 'loader_train', 'loader_test', 'climatology', 'n_epochs', 'lr', 'lr_decay', 'mask', 'high_interest_region',
                    'truncated_backprop', 'graph_structure', 'use_graph', 'accumulate', 'pos_weight', 'test_graph', 'patience',
                    'min_delta', 'restore_best', 'keep_best', 'monitor', 'loss_weights', 'lead_weights']


# -- the schedule -------------------------------------------------------------------------------------------------------------------
def test_resolve_schedule_takes_an_integer_a_sequence_and_a_callable():
    from qtmpnn.horizon import resolve_schedule
    assert resolve_schedule(3, 0, 4) == [3, 3, 3, 3]
    assert resolve_schedule(np.int64(3), 0, 2) == [3, 3] and all(type(k) is int for k in resolve_schedule(np.int64(3), 0, 2))
    assert resolve_schedule([1, 2, 4], 0, 5) == [1, 2, 4, 4, 4], 'the last entry holds for every later epoch'
    assert resolve_schedule((1, 2, 4), 0, 2) == [1, 2]
    assert resolve_schedule(np.array([1, 2]), 0, 3) == [1, 2, 2]
    assert resolve_schedule(lambda e: 2 ** e, 0, 4) == [1, 2, 4, 8]
    assert resolve_schedule([1, 2], 0, 0) == []
    assert resolve_schedule(lambda e: min(1 + e, 6), 0, 8, limit=6) == [1, 2, 3, 4, 5, 6, 6, 6]


def test_the_schedule_continues_from_the_first_epoch():
    from qtmpnn.horizon import resolve_schedule
    whole = resolve_schedule([1, 2, 4, 8], 0, 6)
    assert resolve_schedule([1, 2, 4, 8], 2, 4) == whole[2:] == [4, 8, 8, 8]
    assert resolve_schedule([1, 2, 4, 8], 9, 2) == [8, 8]
    assert resolve_schedule(lambda e: e + 1, 3, 2) == [4, 5]
    # only the entries a call uses are looked at: what an earlier call trained under is not checked again
    assert resolve_schedule([0, 2], 1, 2) == [2, 2]
    called = []
    resolve_schedule(lambda e: called.append(e) or 1, 5, 3)
    assert called == [5, 6, 7]


BAD = [(True, TypeError), (False, TypeError), (2.0, TypeError), ('2', TypeError), (None, TypeError), ([2], TypeError),
       (0, ValueError), (-1, ValueError)]


@pytest.mark.parametrize('bad,error', BAD, ids=[repr(b) for b, _ in BAD])
def test_a_value_that_is_no_integer_from_1_is_refused_with_its_epoch(bad, error):
    from qtmpnn.horizon import check_horizon, resolve_schedule
    with pytest.raises(error, match='^horizon: an integer >= 1 is needed'):
        check_horizon(bad)
    if bad is not None and bad != [2] and bad != '2':       # (None is no schedule at all; a list and a string are other forms)
        with pytest.raises(error, match='^horizon: an integer >= 1'):
            resolve_schedule(bad, 0, 3)
    with pytest.raises(error, match='^horizon: epoch 1: an integer >= 1'):
        resolve_schedule([1, bad, 3], 0, 3)
    with pytest.raises(error, match='^horizon: epoch 5: an integer >= 1'):
        resolve_schedule([1, bad], 5, 3)                    # (the held last entry, named by the first epoch that uses it)
    with pytest.raises(error, match='^horizon: epoch 4: an integer >= 1'):
        resolve_schedule(lambda e: bad if e == 4 else 2, 3, 3)


def test_the_other_refusals_of_the_schedule():
    from qtmpnn.horizon import resolve_schedule
    for empty in ([], (), np.array([], dtype=np.int64)):
        with pytest.raises(ValueError, match='^horizon: the sequence is empty'):
            resolve_schedule(empty, 0, 3)
    with pytest.raises(TypeError, match='^horizon: an integer, a sequence'):
        resolve_schedule('12', 0, 3)
    with pytest.raises(ValueError, match='^horizon: epoch 2: y holds 4 output steps, horizon=6 needs 6$'):
        resolve_schedule([1, 2, 6], 0, 3, limit=4)
    with pytest.raises(ValueError, match='^horizon: the first epoch'):
        resolve_schedule(2, -1, 3)


def test_first_steps_is_a_view_and_refuses_by_message():
    from qtmpnn.horizon import first_steps
    y = torch.arange(2 * 4 * 3 * 3, dtype=torch.float32).reshape(2, 4, 3, 3, 1)
    cut = first_steps(y, 2)
    assert tuple(cut.shape) == (2, 2, 3, 3, 1) and cut.data_ptr() == y.data_ptr() and cut.stride(0) == y.stride(0)
    assert torch.equal(cut, y[:, :2]) and first_steps(y, 4) is y and first_steps(None, 3) is None
    one = first_steps(y[0], 3)
    assert tuple(one.shape) == (3, 3, 3, 1) and one.data_ptr() == y.data_ptr()
    with pytest.raises(ValueError, match='^horizon: y holds 4 output steps, horizon=6 needs 6$'):
        first_steps(y, 6)
    with pytest.raises(ValueError, match='^horizon: concat_layers holds 4 output steps, horizon=5 needs 5$'):
        first_steps(y[0], 5, 'concat_layers')
    assert first_steps(y, 6, strict=False) is y             # (no horizon set: the shape checks that were there refuse it)


# -- the setting --------------------------------------------------------------------------------------------------------------------
def _predictor(**kw):
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=BUILT, device=None,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kw)


def test_the_setting_the_built_value_and_the_context_manager():
    nfp = _predictor()
    assert nfp.output_timesteps == nfp.built_output_timesteps == BUILT and nfp.model.horizon == BUILT
    nfp.set_horizon(6)
    assert nfp.output_timesteps == 6 and nfp.model.horizon == 6
    assert nfp.built_output_timesteps == BUILT and nfp.model.output_timesteps == BUILT
    nfp.set_horizon(None)
    assert nfp.output_timesteps == BUILT
    with nfp.horizon(2) as inside:
        assert inside is nfp and nfp.output_timesteps == 2
        with nfp.horizon(7):
            assert nfp.output_timesteps == 7, 'the inner block wins while it runs'
            with nfp.horizon(None):
                assert nfp.output_timesteps == BUILT
            assert nfp.output_timesteps == 7
        assert nfp.output_timesteps == 2
    assert nfp.output_timesteps == BUILT
    nfp.set_horizon(3)
    with pytest.raises(KeyError, match='inside'):
        with nfp.horizon(1):
            with nfp.horizon(5):
                raise KeyError('inside')
    assert nfp.output_timesteps == 3, 'the setting from before the blocks is back after an exception'
    for bad, error in BAD:
        if bad is None:
            continue
        with pytest.raises(error, match='^horizon: '):
            nfp.set_horizon(bad)
        with pytest.raises(error, match='^horizon: '):
            with nfp.horizon(bad):
                raise AssertionError('the block was entered')
    assert nfp.output_timesteps == 3 and nfp.built_output_timesteps == BUILT
    # no state of the model: state_dict does not carry it
    assert not any('horizon' in k for k in nfp.model.state_dict())


def test_forward_unrolls_the_horizon(monkeypatch):
    from model.seq2seq import Seq2Seq
    nfp = _predictor()
    seen = []
    monkeypatch.setattr(Seq2Seq, 'process_inputs', lambda self, *a, **k: None)
    monkeypatch.setattr(Seq2Seq, 'unroll_output', lambda self, steps, *a, **k: seen.append(steps))
    x = torch.zeros(2, 64, 64, 1)
    nfp.model(x)
    with nfp.horizon(6):
        nfp.model(x)
    with nfp.horizon(1):
        nfp.model(x)
    assert seen == [range(4), range(6), range(1)]


def test_train_keeps_its_parameter_list_and_takes_horizon(monkeypatch, tmp_path):
    from model.mpnnlstm import NextFramePredictorS2S as P
    from qtmpnn import _lib
    assert list(inspect.signature(P.train).parameters) == TRAIN_PARAMETERS
    assert list(inspect.signature(P.set_horizon).parameters) == ['self', 'k']
    assert list(inspect.signature(P.horizon).parameters) == ['self', 'k']
    assert 'horizon=None' in P.train.__doc__
    assert len(_lib.exported_names()) == 91
    nfp, trained, tested = _scripted(monkeypatch, tmp_path)
    nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0, horizon=2)
    assert [k for k, _ in trained] == [2, 2] and tested == [BUILT]
    with pytest.raises(TypeError, match='horizons'):
        nfp.train(_loader(), _loader(), n_epochs=1, horizons=2)


def test_the_description_of_a_checkpoint_keeps_the_built_value(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    nfp = _predictor()
    nfp.initiate_training(0.01, 0.5)
    with nfp.horizon(2):
        assert nfp._description()['output_timesteps'] == BUILT
        nfp.save_checkpoint('under.pt')
    nfp.save_checkpoint('plain.pt')
    under, plain = (torch.load(p, weights_only=True) for p in ('under.pt', 'plain.pt'))
    assert under['description'] == plain['description'] and under['description']['output_timesteps'] == BUILT
    assert set(under) == set(plain) and under['format'] == plain['format'] == 1, 'no field, no format change'
    # a file loads under any setting and leaves the setting alone
    nfp.set_horizon(6)
    nfp.load_checkpoint('under.pt')
    assert nfp.output_timesteps == 6
    twin = _predictor()
    twin.load_checkpoint('under.pt')
    assert twin.output_timesteps == BUILT


def test_set_horizon_is_allowed_inside_averaged_weights(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    nfp = _predictor()
    nfp.initiate_training(0.01, 0.5)
    nfp.set_ema(0.9)
    for p in nfp.model.parameters():
        p.grad = torch.ones_like(p)
    nfp._clip_and_step(list(nfp.model.parameters()), 10.0)
    with nfp.averaged_weights():
        nfp.set_horizon(2)
        assert nfp.output_timesteps == 2
        with nfp.horizon(6):
            assert nfp.output_timesteps == 6
    assert nfp.output_timesteps == 2


def test_the_day_cache_is_keyed_by_date_and_step_count():
    from model.utils import output_day_indices
    nfp = _predictor()
    rng = np.random.default_rng(3)
    clim = torch.from_numpy(rng.random((1, 366, 5, 6), dtype=np.float32))
    day = 86400 * 10 ** 9
    dates = torch.tensor([1267444800 * 10 ** 9 + day * i for i in (0, 40)], dtype=torch.int64)

    def want(k):
        return torch.stack([torch.moveaxis(clim[:, output_day_indices(d, k)], 0, -1) for d in dates.numpy()])
    four = nfp.get_climatology_array(clim, dates)
    assert tuple(four.shape) == (2, 4, 5, 6, 1) and torch.equal(four, want(4))
    with nfp.horizon(6):
        six = nfp.get_climatology_array(clim, dates)            # (the same dates: a cache keyed by date alone serves 4 days here)
        assert tuple(six.shape) == (2, 6, 5, 6, 1) and torch.equal(six, want(6))
        assert tuple(nfp.get_climatology_array(clim, dates[:1]).shape) == (6, 5, 6, 1)
    with nfp.horizon(2):
        assert torch.equal(nfp.get_climatology_array(clim, dates), want(2))
    assert torch.equal(nfp.get_climatology_array(clim, dates), four)
    assert sorted({k for _, k in nfp._output_days}) == [2, 4, 6] and len(nfp._output_days) == 6
    assert output_day_indices(dates[0].item(), 6)[:4] == output_day_indices(dates[0].item(), 4)


# -- refusals that need no device: by message, before the model's forward and before any library call -------------------------------
@pytest.fixture
def guarded(monkeypatch, tmp_path):
    """A predictor without a device on which a rollout or a library call is an error."""
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    monkeypatch.chdir(tmp_path)

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(Seq2Seq, 'forward', launched)
    monkeypatch.setattr(Seq2Seq, 'process_inputs', launched)
    monkeypatch.setattr(_lib, 'call', launched)
    return _predictor()


def test_a_horizon_above_the_steps_of_y_is_refused_before_any_launch(guarded):
    nfp = guarded
    x, y = torch.zeros(2, 2, 64, 64, 1), torch.zeros(2, BUILT, 64, 64, 1)
    nfp.initiate_training(0.01, 0.5)
    message = '^horizon: y holds 4 output steps, horizon=6 needs 6$'
    with nfp.horizon(6):
        for call in (lambda: nfp.forward_loss(x, y), lambda: nfp.train_step(x, y), lambda: nfp.accumulated_step([(x, y), (x, y)]),
                     lambda: nfp.truncated_backward(x, y, None, None), lambda: nfp.accumulate_gradients([(x, y)])):
            with pytest.raises(ValueError, match=message):
                call()
        with pytest.raises(ValueError, match=message):
            nfp.verify(TinyLoader([(x[:1], y[:1], torch.zeros(1))], (64, 64)), products=('score',))
    # with no horizon set a short y is refused as it was, in the words it was
    with pytest.raises(AssertionError, match='a launch was reached'):
        nfp.forward_loss(x, y[:, :2])


def test_a_short_concat_layers_is_refused_before_any_launch(guarded):
    nfp = guarded
    x, y, concat = torch.zeros(2, 2, 64, 64, 1), torch.zeros(2, 6, 64, 64, 1), torch.zeros(2, BUILT, 64, 64, 1)
    message = '^horizon: concat_layers holds 4 output steps, horizon=6 needs 6$'
    with nfp.horizon(6):
        for call in (lambda: nfp.forward_loss(x, y, concat), lambda: nfp.truncated_backward(x, y, concat, None),
                     lambda: nfp.attention_weights(x, concat), lambda: nfp.forward_loss(x[0], y[0], concat[0])):
            with pytest.raises(ValueError, match=message):
                call()


def test_lead_weights_are_held_to_the_horizon(guarded):
    nfp = guarded
    x, y = torch.zeros(2, 2, 64, 64, 1), torch.zeros(2, BUILT, 64, 64, 1)
    with nfp.horizon(2):
        for bad in (np.ones(BUILT, np.float32), [1.0] * 3, torch.ones(1)):
            with pytest.raises(ValueError, match=f'^horizon: lead_weights has {len(bad)} entries, horizon=2 needs 2$'):
                nfp.forward_loss(x, y, lead_weights=bad)
        lw = nfp._loss_weights(x, None, None, [1.0, 3.0])
        assert lw.T == 2 and lw.sum_lam == 4.0
    # inside train(horizon=) the built length, cut epoch by epoch
    with pytest.raises(ValueError, match='^horizon: lead_weights has 2 entries, train.horizon=. takes the built length 4'):
        nfp.train(_loader(), _loader(), n_epochs=2, horizon=[1, 2], lead_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match='^horizon: the first 1 lead_weights sum to 0'):
        nfp.train(_loader(), _loader(), n_epochs=2, horizon=[1, 2], lead_weights=[0.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match='^horizon: lead_weights has 4 entries .the built output steps., horizon=6 needs 6$'):
        nfp.train(_loader(), _loader(), n_epochs=2, horizon=[1, 6], lead_weights=[1.0, 1.0, 1.0, 1.0])


def test_horizon_weights_are_the_twins_weights():
    from model.mpnnlstm import LossWeights, horizon_weights
    rng = np.random.default_rng(5)
    w, lam = rng.random((6, 7)).astype(np.float32), rng.random(BUILT).astype(np.float32)
    mask = np.zeros((6, 7), dtype=bool)
    mask[:, 5:] = True
    full = LossWeights(w, lam, (6, 7), BUILT, mask, pos_weight=2.0).to('cpu')
    assert horizon_weights(None, 2) is None and horizon_weights(full, BUILT) is full
    for k in (1, 2, 3):
        cut, twin = horizon_weights(full, k), LossWeights(w, lam[:k], (6, 7), k, mask, pos_weight=2.0).to('cpu')
        assert cut.T == twin.T == k and cut.sum_lam == twin.sum_lam and cut.sum_w == twin.sum_w and cut.pos_weight == 2.0
        assert torch.equal(cut.lam, twin.lam) and torch.equal(cut.w, twin.w) and cut.lam.is_contiguous()


BAD_IN_TRAIN = [(True, TypeError, '^horizon: an integer'), (2.5, TypeError, '^horizon: an integer'), (0, ValueError, '^horizon: an integer'),
                ([], ValueError, '^horizon: the sequence is empty'), ([1, 2.0], TypeError, '^horizon: epoch 1: '),
                ([1, True], TypeError, '^horizon: epoch 1: '), (lambda e: e, ValueError, '^horizon: epoch 0: '),
                (lambda e: 1.0, TypeError, '^horizon: epoch 0: '), ('2', TypeError, '^horizon: an integer, a sequence')]


@pytest.mark.parametrize('bad,error,match', BAD_IN_TRAIN, ids=[str(i) for i in range(len(BAD_IN_TRAIN))])
def test_train_refuses_a_bad_schedule_before_the_optimiser_is_made(guarded, bad, error, match):
    nfp = guarded
    with pytest.raises(error, match=match):
        nfp.train(_loader(), _loader(), n_epochs=3, horizon=bad)
    assert not nfp.training_initiated and nfp.output_timesteps == BUILT and nfp._horizon_asked is None


def test_the_single_chunk_rule_is_judged_per_epoch(guarded):
    nfp = guarded
    for kw, match in ((dict(use_graph=True), r'^use_graph=True needs truncated_backprop=0 or >= the output steps.*horizon=3, epoch 2'),
                      (dict(accumulate=2), r'^accumulate: accumulate=2 needs truncated_backprop=0.*for 3 steps \(horizon=3, epoch 2\)')):
        with pytest.raises(ValueError, match=match):
            nfp.train(_loader(), _loader(), n_epochs=3, truncated_backprop=2, horizon=[1, 2, 3], **kw)
    assert not nfp.training_initiated


# -- train()'s bookkeeping around scripted steps ------------------------------------------------------------------------------------
def _loader(n=2, steps=BUILT):
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(steps, 64, 64, 1)
    return TinyLoader([(x[None], y[None], torch.zeros(1))] * n, (64, 64))


def _scripted(monkeypatch, tmp_path, **kw):
    """A predictor without a device whose training step and test pass record the horizon they run under -> (predictor, the
    (horizon, loss weights) of every training step, the horizon of every test pass)."""
    monkeypatch.chdir(tmp_path)
    nfp = _predictor(**kw)
    trained, tested = [], []

    def train_step(x, y, concat=None, mask=None, hir=None, gs=None, loss_weights=None, **k):
        trained.append((nfp.output_timesteps, loss_weights))
        return torch.tensor(0.5)

    def test_pass(*a, **k):
        tested.append(nfp.output_timesteps)
        return 0.25, 1
    monkeypatch.setattr(nfp, 'train_step', train_step)
    monkeypatch.setattr(nfp, '_test_pass', test_pass)
    return nfp, trained, tested


def test_every_epoch_trains_under_its_horizon_and_tests_under_the_calls(monkeypatch, tmp_path):
    nfp, trained, tested = _scripted(monkeypatch, tmp_path)
    nfp.train(_loader(), _loader(), truncated_backprop=0, n_epochs=3, horizon=[1, 2])
    assert [k for k, _ in trained] == [1, 1, 2, 2, 2, 2] and tested == [BUILT] * 3
    assert all(lw is None for _, lw in trained) and nfp.output_timesteps == BUILT
    # the epoch index is the whole history's: a second call goes on where the schedule stood
    del trained[:], tested[:]
    nfp.train(_loader(), _loader(), truncated_backprop=0, n_epochs=2, horizon=[1, 2, 3, 4, 5, 6])
    assert [k for k, _ in trained] == [4, 4, 5, 5] and len(nfp.train_loss) == 5
    # the test pass runs at the horizon in force when train() was called
    del trained[:], tested[:]
    with nfp.horizon(3):
        nfp.train(_loader(), _loader(), truncated_backprop=0, n_epochs=2, horizon=lambda e: e - 3)
        assert nfp.output_timesteps == 3
    assert [k for k, _ in trained] == [2, 2, 3, 3] and tested == [3, 3]
    # without the keyword every pass runs under the setting in force, and nothing is set
    del trained[:], tested[:]
    nfp.train(_loader(), _loader(), truncated_backprop=0, n_epochs=1)
    assert [k for k, _ in trained] == [BUILT] * 2 and tested == [BUILT]
    # an exception inside an epoch leaves the caller's setting behind
    monkeypatch.setattr(nfp, 'train_step', lambda *a, **k: (_ for _ in ()).throw(KeyError('inside')))
    with pytest.raises(KeyError, match='inside'):
        nfp.train(_loader(), _loader(), truncated_backprop=0, n_epochs=1, horizon=1)
    assert nfp.output_timesteps == BUILT and nfp._horizon_asked is None


def test_lead_weights_are_cut_to_every_epochs_horizon(monkeypatch, tmp_path):
    nfp, trained, tested = _scripted(monkeypatch, tmp_path)
    lam = [1.0, 2.0, 4.0, 8.0]
    nfp.train(_loader(1), _loader(1), truncated_backprop=0, n_epochs=4, horizon=[1, 2, 4], lead_weights=lam)
    assert [(k, lw.T, lw.sum_lam) for k, lw in trained] == [(1, 1, 1.0), (2, 2, 3.0), (4, 4, 15.0), (4, 4, 15.0)]
    assert all(lw.lam.tolist() == lam[:k] for k, lw in trained)
