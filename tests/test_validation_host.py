"""Validation in train(), host side: the stopping rule on hand-written histories, the refusals of the new keywords (by name,
before anything reaches a device or the optimiser is made), the signature, and train()'s bookkeeping around a scripted test
pass -- where it stops, which weights it restores, when it writes the checkpoint, what a Monitor's value may be.  The ABI and the
product table are what they were: this feature adds no entry point and no product."""
import inspect
import math
import pathlib

import numpy as np
import pytest
import torch

from helpers import TinyLoader

T_ = 3
NAN = float('nan')


# -- the rule ---------------------------------------------------------------------------------------------------------------------
def test_best_and_wait_on_plain_histories():
    from qtmpnn.validation import best_and_wait
    assert best_and_wait([], 0.0, 'min') == (None, None, 0)
    assert best_and_wait([0.5], 0.0, 'min') == (0, 0.5, 0)
    # strictly falling: every epoch improves, nothing to wait for
    assert best_and_wait([0.9, 0.8, 0.7, 0.6], 0.0, 'min') == (3, 0.6, 0)
    # constant: the first epoch is the best one, every later one is a tie
    assert best_and_wait([0.5, 0.5, 0.5, 0.5], 0.0, 'min') == (0, 0.5, 3)
    # rising after a minimum
    assert best_and_wait([0.9, 0.4, 0.5, 0.6, 0.7], 0.0, 'min') == (1, 0.4, 3)
    # every prefix: what train() sees epoch by epoch
    h = [0.9, 0.4, 0.5, 0.3, 0.35]
    assert [best_and_wait(h[:k], 0.0, 'min') for k in range(1, 6)] == [(0, 0.9, 0), (1, 0.4, 0), (1, 0.4, 1), (3, 0.3, 0), (3, 0.3, 1)]
    # the defaults are min_delta 0 and 'min'; any sequence of numbers will do
    assert best_and_wait(np.array([2.0, 1.0, 1.5], np.float32)) == (1, 1.0, 1)


def test_best_and_wait_ties_and_min_delta():
    from qtmpnn.validation import best_and_wait
    # a tie does not improve, at min_delta 0 ...
    assert best_and_wait([0.5, 0.5], 0.0, 'min') == (0, 0.5, 1)
    assert best_and_wait([0.5, math.nextafter(0.5, 0.0)], 0.0, 'min') == (1, math.nextafter(0.5, 0.0), 0)
    # ... and at min_delta > 0 an epoch has to be better by MORE than it: 0.5 -> 0.25 at min_delta 0.25 is a tie as well
    assert best_and_wait([0.5, 0.375, 0.3125], 0.25, 'min') == (0, 0.5, 2)
    assert best_and_wait([0.5, 0.25], 0.25, 'min') == (0, 0.5, 1)
    assert best_and_wait([0.5, 0.125], 0.25, 'min') == (1, 0.125, 0)
    # the best value is the last IMPROVING one: 0.375 is smaller than 0.5 but no improvement, and 0.125 is measured against 0.5
    assert best_and_wait([0.5, 0.375, 0.125], 0.25, 'min') == (2, 0.125, 0)
    assert best_and_wait([0.5, 0.375, 0.1875], 0.25, 'min') == (2, 0.1875, 0)
    assert best_and_wait([0.5, 0.375, 0.26], 0.25, 'min') == (0, 0.5, 2)


def test_best_and_wait_mode_max():
    from qtmpnn.validation import best_and_wait
    assert best_and_wait([0.1, 0.2, 0.3], 0.0, 'max') == (2, 0.3, 0)
    assert best_and_wait([0.1, 0.5, 0.4, 0.5], 0.0, 'max') == (1, 0.5, 2)
    assert best_and_wait([0.25, 0.5, 1.0], 0.25, 'max') == (2, 1.0, 0)          # 0.5 ties with 0.25 + 0.25, 1.0 beats it
    assert best_and_wait([0.25, 0.5, 0.5], 0.25, 'max') == (0, 0.25, 2)
    assert best_and_wait([-1.0, -2.0], 0.0, 'max') == (0, -1.0, 1)
    with pytest.raises(ValueError, match='mode'):
        best_and_wait([0.1], 0.0, 'sideways')


def test_best_and_wait_never_improves_on_a_nan():
    from qtmpnn.validation import best_and_wait
    assert best_and_wait([0.5, NAN, 0.6], 0.0, 'min') == (0, 0.5, 2)
    assert best_and_wait([0.5, NAN, 0.4], 0.0, 'min') == (2, 0.4, 0)
    assert best_and_wait([NAN, NAN], 0.0, 'min') == (None, None, 2)
    assert best_and_wait([NAN, 0.5, NAN], 0.0, 'min') == (1, 0.5, 1)
    assert best_and_wait([0.5, NAN, 0.6], 0.0, 'max') == (2, 0.6, 0)
    assert best_and_wait([0.7, NAN], 0.1, 'max') == (0, 0.7, 1)


def test_best_and_wait_runs_over_a_history_of_two_train_calls():
    """The first call's epochs count: a history that a checkpoint brought along is read like one that was never interrupted."""
    from qtmpnn.validation import best_and_wait
    first, second = [0.9, 0.5, 0.6], [0.7, 0.65]
    assert best_and_wait(first, 0.0, 'min') == (1, 0.5, 1)
    assert best_and_wait(first + second, 0.0, 'min') == (1, 0.5, 3)             # patience 3 stops here, two epochs into the second call
    assert best_and_wait(second, 0.0, 'min') == (1, 0.65, 0)                    # (what forgetting the first call would give)
    assert best_and_wait(first + [0.45], 0.0, 'min') == (3, 0.45, 0)


# -- the keywords -----------------------------------------------------------------------------------------------------------------
def test_train_has_the_new_keywords_with_their_defaults():
    from model.mpnnlstm import NextFramePredictorS2S as P
    params = inspect.signature(P.train).parameters
    want = dict(test_graph=False, patience=None, min_delta=0.0, restore_best=False, keep_best=None, monitor='loss')
    for name, default in want.items():
        assert params[name].default == default and type(params[name].default) is type(default), name
    # what was there keeps its place: the new keywords stand between pos_weight and the two weights that close the list
    names = list(params)
    assert names[:17] == ['self', 'loader_train', 'loader_test', 'climatology', 'n_epochs', 'lr', 'lr_decay', 'mask',
                          'high_interest_region', 'truncated_backprop', 'graph_structure', 'use_graph', 'accumulate', 'pos_weight',
                          'test_graph', 'patience', 'min_delta']
    assert names[-2:] == ['loss_weights', 'lead_weights'] and len(names) == 22
    inf = inspect.signature(P._inference).parameters
    assert inf['graphed'].default is None
    from model import mpnnlstm
    assert list(inspect.signature(mpnnlstm.loss_product).parameters) == ['mask', 'lw', 'binary', 'fused']


def test_abi_and_product_table_are_what_they_were():
    from model.mpnnlstm import DEFAULT_PRODUCTS, PRODUCTS
    from qtmpnn import _lib
    assert len(_lib.exported_names()) == 91
    assert tuple(PRODUCTS) == ('predict', 'score', 'score_maps', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')
    assert DEFAULT_PRODUCTS == ('score', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')
    assert not any('loss' in name for name in PRODUCTS)


@pytest.fixture
def cpu_predictor(monkeypatch, tmp_path):
    """A predictor without a device that records what would run: train_step, _inference, the model's forward, a library call."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    monkeypatch.chdir(tmp_path)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    nfp.ran = []
    record = lambda what: lambda *a, **k: nfp.ran.append(what)
    monkeypatch.setattr(nfp, 'train_step', record('train_step'))
    monkeypatch.setattr(nfp, '_inference', record('_inference'))
    monkeypatch.setattr(Seq2Seq, 'forward', record('forward'))
    monkeypatch.setattr(_lib, 'call', record('call'))
    return nfp


def _loader(n=2):
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    return TinyLoader([(x[None], y[None], torch.zeros(1))] * n, (64, 64))


class _Fspath:
    def __fspath__(self):
        return 'best.pt'


REFUSALS = [
    ('patience', 0, ValueError), ('patience', -3, ValueError), ('patience', 2.0, TypeError), ('patience', '2', TypeError),
    ('patience', True, TypeError), ('patience', [2], TypeError),
    ('min_delta', -0.1, ValueError), ('min_delta', NAN, ValueError), ('min_delta', float('inf'), ValueError),
    ('min_delta', None, TypeError), ('min_delta', '0.1', TypeError), ('min_delta', [0.0, 0.1], TypeError), ('min_delta', True, TypeError),
    ('restore_best', 1, TypeError), ('restore_best', None, TypeError), ('restore_best', 'yes', TypeError),
    ('test_graph', 1, TypeError), ('test_graph', None, TypeError), ('test_graph', 'True', TypeError),
    ('keep_best', 3, TypeError), ('keep_best', b'best.pt', TypeError), ('keep_best', True, TypeError), ('keep_best', '', ValueError),
    ('monitor', 'iiee', TypeError), ('monitor', None, TypeError), ('monitor', ('extent',), TypeError),
    ('monitor', lambda v: 0.0, TypeError),
]


@pytest.mark.parametrize('name,bad,error', REFUSALS, ids=[f'{n}-{i}' for i, (n, _, _) in enumerate(REFUSALS)])
def test_refusals_name_the_keyword_and_come_before_any_launch(cpu_predictor, name, bad, error):
    nfp = cpu_predictor
    with pytest.raises(error, match=f'^{name}: '):
        nfp.train(_loader(), _loader(), n_epochs=1, **{name: bad})
    assert nfp.ran == [] and not nfp.training_initiated


def test_a_monitor_is_checked_when_made_and_again_by_train(cpu_predictor):
    from qtmpnn.validation import Monitor
    nfp = cpu_predictor
    with pytest.raises(ValueError, match='^monitor: mode'):
        Monitor(('extent',), lambda v: 0.0, mode='lower')
    with pytest.raises(ValueError, match='^monitor: mode'):
        Monitor(('extent',), lambda v: 0.0, mode=None)
    with pytest.raises(TypeError, match='^monitor: value'):
        Monitor(('extent',), 0.5)
    with pytest.raises(TypeError, match='^monitor: value'):
        Monitor(('extent',), 'iiee', 'max')
    good = Monitor(('extent',), lambda v: 0.0, 'max')
    assert good.mode == 'max' and good.products == ('extent',) and 'extent' in repr(good)
    for attr, bad, error in (('mode', 'sideways', ValueError), ('value', None, TypeError)):
        m = Monitor(('extent',), lambda v: 0.0)
        setattr(m, attr, bad)               # (changed after it was made)
        with pytest.raises(error, match=f'^monitor: {attr}'):
            nfp.train(_loader(), _loader(), n_epochs=1, monitor=m)
    # the monitor's products are make_products' to check, under the name `train`, before the first training batch
    for products, match in (((), 'train: products is empty'), (('iiee',), "train: unknown product 'iiee'"),
                            ({'extent': {'bins': 3}}, "train: product 'extent' takes no keyword 'bins'"),
                            (('score', 'score'), "train: product 'score' is given twice")):
        with pytest.raises(ValueError, match=match):
            nfp.train(_loader(), _loader(), n_epochs=1, monitor=Monitor(products, lambda v: 0.0))
    with pytest.raises(ValueError, match='reliability: bins must be'):
        nfp.train(_loader(), _loader(), n_epochs=1, monitor=Monitor({'reliability': {'bins': 1}}, lambda v: 0.0))
    assert nfp.ran == [] and not nfp.training_initiated


def test_good_values_of_the_keywords_pass_the_checks():
    from qtmpnn import validation as V
    assert V.check_patience(None) is None and V.check_patience(1) == 1 and type(V.check_patience(np.int64(4))) is int
    assert V.check_min_delta(0) == 0.0 and V.check_min_delta(np.float32(0.5)) == 0.5 and type(V.check_min_delta(1)) is float
    assert V.check_flag('restore_best', np.bool_(True)) is True and V.check_flag('test_graph', False) is False
    p = pathlib.Path('a') / 'best.pt'
    assert V.check_keep_best(None) is None and V.check_keep_best('best.pt') == 'best.pt' and V.check_keep_best(p) is p
    assert isinstance(V.check_keep_best(_Fspath()), _Fspath)
    assert V.check_monitor('loss') == 'loss'
    assert V.monitored_value(np.float32(0.5), 0) == 0.5 and V.monitored_value(3, 0) == 3.0 and V.monitored_value(np.array([0.25]), 0) == 0.25
    for bad, error in ((NAN, ValueError), (float('inf'), ValueError), (np.float64('nan'), ValueError), (None, TypeError),
                       ('0.5', TypeError), (np.array([0.1, 0.2]), TypeError), (True, TypeError), ([0.5], TypeError)):
        with pytest.raises(error, match='^monitor: value'):
            V.monitored_value(bad, 3)


# -- train()'s bookkeeping around a scripted test pass ----------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append(value)

    def flush(self):
        pass


def _scripted(monkeypatch, tmp_path, losses, lr=0.01):
    """A predictor on the CPU whose training step adds 1 to every parameter and whose test pass returns the scripted sums (one
    test batch: running_test = sum / 2); the parameters start at 0, so after epoch e (two steps each) they are 2 (e + 1)."""
    from model.mpnnlstm import NextFramePredictorS2S
    monkeypatch.chdir(tmp_path)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.zero_()
    script, nfp.passes = iter(losses), []

    def train_step(*a, **k):
        with torch.no_grad():
            for p in nfp.model.parameters():
                p.add_(1.0)
        return torch.tensor(0.5)

    def test_pass(loader, climatology, loss_reduce, made, use_graph, graphed, **fwd):
        nfp.passes.append((use_graph, None if graphed is None else id(graphed), sorted(fwd)))
        for p in made.values():
            p.reset()
            p.collect(torch.zeros(T_, 1, 2, 8, dtype=torch.float64), None)
        return 2 * next(script), 1
    monkeypatch.setattr(nfp, 'train_step', train_step)
    monkeypatch.setattr(nfp, '_test_pass', test_pass)
    nfp.initiate_training(lr, 0.5)
    nfp.writer = _Recorder()
    return nfp


def _run(nfp, n_test=1, **kw):
    nfp.train(_loader(), _loader(n_test), truncated_backprop=0, **kw)


def _level(nfp):
    values = {float(v) for p in nfp.model.parameters() for v in p.detach().reshape(-1)[:2]}
    assert len(values) == 1
    return values.pop()


def test_no_keyword_no_bookkeeping(monkeypatch, tmp_path, capsys):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.75])
    _run(nfp, n_epochs=3)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 4 and out[-1].startswith('Finished in') and all('| Epoch' in line for line in out[:3])
    assert nfp.test_loss == [0.5, 0.25, 0.75] and _level(nfp) == 6.0
    assert nfp.best_epoch is None and nfp.best_value is None and nfp.stopped_epoch is None and nfp.monitor_history == []
    assert sorted(nfp.writer.scalars) == ['Loss/test', 'Loss/train']
    assert nfp.passes == [(False, None, ['graph_structure', 'high_interest_region', 'mask'])] * 3
    assert list(nfp.loss.test_loss) == nfp.test_loss


def test_patience_stops_where_the_rule_says(monkeypatch, tmp_path, capsys):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375, 0.25, 0.125])
    _run(nfp, n_epochs=5, patience=2)
    assert nfp.test_loss == [0.5, 0.25, 0.375, 0.25] and (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (1, 0.25, 3)
    assert _level(nfp) == 8.0 and len(nfp.loss) == 4            # the last epoch's weights: restore_best was not asked for
    assert 'Stopped after epoch 3' in capsys.readouterr().out
    # a second call goes on from the whole history: one more epoch without improvement is already two too many at patience 2 ...
    nfp2 = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375, 0.3125, 0.3125])
    _run(nfp2, n_epochs=3)
    assert nfp2.stopped_epoch is None and nfp2.best_epoch is None
    _run(nfp2, n_epochs=3, patience=3)
    assert nfp2.test_loss == [0.5, 0.25, 0.375, 0.3125, 0.3125] and (nfp2.best_epoch, nfp2.stopped_epoch) == (1, 4)
    # ... and min_delta decides what an improvement is
    nfp3 = _scripted(monkeypatch, tmp_path, [0.5, 0.4375, 0.375, 0.125])
    _run(nfp3, n_epochs=4, patience=2, min_delta=0.125)
    assert nfp3.test_loss == [0.5, 0.4375, 0.375] and (nfp3.best_epoch, nfp3.best_value, nfp3.stopped_epoch) == (0, 0.5, 2)
    # a run that never waits long enough does not stop
    nfp4 = _scripted(monkeypatch, tmp_path, [0.5, 0.625, 0.25])
    _run(nfp4, n_epochs=3, patience=2)
    assert (nfp4.best_epoch, nfp4.best_value, nfp4.stopped_epoch) == (2, 0.25, None) and len(nfp4.test_loss) == 3


def test_restore_best_and_keep_best(monkeypatch, tmp_path):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375, 0.3125])
    path = tmp_path / 'best.pt'
    saves, save = [], nfp.save_checkpoint
    monkeypatch.setattr(nfp, 'save_checkpoint', lambda p: (saves.append((p, list(nfp.test_loss), nfp.scheduler.last_epoch, _level(nfp))), save(p)))
    _run(nfp, n_epochs=4, restore_best=True, keep_best=path)
    # written on the improving epochs 0 and 1, after the histories were appended and the scheduler stepped
    assert saves == [(path, [0.5], 1, 2.0), (path, [0.5, 0.25], 2, 4.0)]
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (1, 0.25, None) and len(nfp.test_loss) == 4
    assert _level(nfp) == 4.0, 'the weights of epoch 1, not those of epoch 3 (8.0)'
    assert nfp.scheduler.last_epoch == 4, 'the schedule stays the last epoch\'s'
    from model.mpnnlstm import NextFramePredictorS2S
    other = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                  model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    other.load_checkpoint(path)
    assert other.test_loss == [0.5, 0.25] and other.monitor_history == []
    for (k, p), (_, q) in zip(nfp.model.state_dict().items(), other.model.state_dict().items()):
        assert torch.equal(p, q), k


def test_monitor_feeds_the_rule_and_its_value_is_checked(monkeypatch, tmp_path):
    from qtmpnn.validation import Monitor
    from qtmpnn.verify import Verification
    values, seen = iter([0.25, 0.5, 0.375, 0.4375, 0.75]), []

    def value(v):
        seen.append(v)
        return next(values)
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.125, 0.0625, 0.03125])
    _run(nfp, n_epochs=5, patience=2, restore_best=True, monitor=Monitor(('score',), value, 'max'))
    # the loss falls all the way, the monitored score peaks at epoch 1: that is what stops the run and whose weights come back
    assert nfp.test_loss == [0.5, 0.25, 0.125, 0.0625] and nfp.monitor_history == [0.25, 0.5, 0.375, 0.4375]
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (1, 0.5, 3) and _level(nfp) == 4.0
    assert nfp.writer.scalars['Monitor/test'] == nfp.monitor_history and nfp.writer.scalars['Loss/test'] == nfp.test_loss
    assert all(isinstance(v, Verification) and v.products == ('score',) and v.sources == ('model', 'persistence') for v in seen)
    assert all(v.score.sums.shape == (1, T_, 2, 8) for v in seen), 'every epoch sees its own pass, not the passes so far'
    for bad, error in ((NAN, ValueError), (None, TypeError), ('0.5', TypeError)):
        nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25])
        with pytest.raises(error, match='^monitor: value.*epoch 0'):
            _run(nfp, n_epochs=2, monitor=Monitor(('score',), lambda v: bad))
        assert len(nfp.passes) == 1 and nfp.test_loss == [] and nfp.monitor_history == []
    # initiate_training and load_checkpoint empty the history, as they replace test_loss
    nfp.monitor_history = [1.0]
    nfp.initiate_training(0.01, 0.5)
    assert nfp.monitor_history == []


def test_every_call_starts_its_own_selection(monkeypatch, tmp_path):
    """best_epoch / best_value / stopped_epoch of an earlier call do not survive into a call without the keywords, and a Monitor's
    history is its call's: a second call, which may monitor another quantity in another mode, does not read on in the first one's;
    test_loss goes on across the calls."""
    from qtmpnn.validation import Monitor
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375, 0.3125, 0.28125, 0.265625, 0.2578125])
    values = iter([3.0, 2.0, 1.0, 10.0, 20.0])
    _run(nfp, n_epochs=3, patience=1, monitor=Monitor(('score',), lambda v: next(values), 'min'))
    assert nfp.monitor_history == [3.0, 2.0, 1.0] and (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (2, 1.0, None)
    # the same predictor, now maximising something else: 10.0 is epoch 0 of a new history, not "worse than 1.0" of the old one
    _run(nfp, n_epochs=2, patience=1, monitor=Monitor(('score',), lambda v: next(values), 'max'))
    assert nfp.monitor_history == [10.0, 20.0] and (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (1, 20.0, None)
    assert nfp.test_loss == [0.5, 0.25, 0.375, 0.3125, 0.28125]
    # a call without the keywords leaves None, and leaves the last monitor's history alone
    _run(nfp, n_epochs=1)
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (None, None, None) and nfp.monitor_history == [10.0, 20.0]
    # on the loss the history is the predictor's: the sixth epoch is measured against 0.25 of the first call
    _run(nfp, n_epochs=1, patience=5)
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (1, 0.25, 6) and len(nfp.test_loss) == 7


def test_the_test_pass_gets_one_dict_of_captures_for_all_epochs(monkeypatch, tmp_path):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.125])
    _run(nfp, n_epochs=3, test_graph=True)
    assert [u for u, _, _ in nfp.passes] == [True] * 3 and len({g for _, g, _ in nfp.passes}) == 1 and nfp.passes[0][1] is not None
    assert nfp.best_epoch is None, 'test_graph alone selects nothing'
