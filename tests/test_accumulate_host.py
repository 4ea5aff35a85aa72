"""Gradient accumulation, host side: the signatures, the refusals (by name, before anything reaches a device) and the two pure
rules -- the micro-batch weights w_i = B_i / sum B and the scale 1 / (j * world) of a graphed group."""
import inspect

import numpy as np
import pytest
import torch

from helpers import TinyLoader

T_ = 3


@pytest.fixture
def cpu_predictor(monkeypatch):
    """A predictor without a device whose first launch of any kind fails the test: the model's forward and the library call."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(Seq2Seq, 'forward', launched)
    monkeypatch.setattr(_lib, 'call', launched)
    monkeypatch.setattr(nfp, 'zero_grad', launched)
    return nfp


def test_signatures():
    from model.mpnnlstm import NextFramePredictorS2S as P
    for meth, before in (('train', 'use_graph'), ('make_graphed_step', 'force_multi')):
        params = inspect.signature(getattr(P, meth)).parameters
        names = list(params)
        assert params['accumulate'].default == 1, meth
        assert names.index('accumulate') == names.index(before) + 1 == names.index('pos_weight') - 1, (meth, names)
    for meth in ('forward_loss', 'train_step', 'truncated_backward', 'make_graphed_step', 'train', 'accumulated_step'):
        names = list(inspect.signature(getattr(P, meth)).parameters)
        assert names[-2:] == ['loss_weights', 'lead_weights'], (meth, names)
    assert list(inspect.signature(P.accumulated_step).parameters) == [
        'self', 'batches', 'mask', 'high_interest_region', 'graph_structure', 'max_norm', 'fused', 'pos_weight', 'loss_weights',
        'lead_weights']
    sig = inspect.signature(P.accumulated_step).parameters
    assert sig['max_norm'].default == 10.0 and sig['fused'].default is False and sig['mask'].default is None
    # train_step is what it was
    assert list(inspect.signature(P.train_step).parameters) == [
        'self', 'x', 'y', 'concat_layers', 'mask', 'high_interest_region', 'graph_structure', 'max_norm', 'fused', 'pos_weight',
        'loss_weights', 'lead_weights']


def test_accumulated_step_refusals_come_before_any_launch(cpu_predictor):
    nfp = cpu_predictor
    x, y, c = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    with pytest.raises(ValueError, match='batches is empty'):
        nfp.accumulated_step([])
    with pytest.raises(ValueError, match='batches is empty'):
        nfp.accumulated_step(iter(()))
    for other in ((torch.zeros(2, 64, 32, 1), torch.zeros(T_, 64, 32, 1)),              # another frame
                  (torch.zeros(1, 2, 32, 64, 1), torch.zeros(1, T_, 32, 64, 1)),
                  (torch.zeros(3, 64, 64, 1), y),                                       # another T_in
                  (x, torch.zeros(T_ + 1, 64, 64, 1)),                                  # another T_out
                  (torch.zeros(2, 64, 64, 2), y)):                                      # another channel count
        with pytest.raises(ValueError, match=r'batches\[1\] has another frame shape'):
            nfp.accumulated_step([(x, y), other])
    with pytest.raises(ValueError, match='concat_layers is given for some micro-batches and not for others'):
        nfp.accumulated_step([(x, y, c), (x, y)])
    with pytest.raises(ValueError, match='concat_layers is given for some micro-batches and not for others'):
        nfp.accumulated_step([(x, y), (x, y), (x, y, c)])
    with pytest.raises(ValueError, match=r'batches\[1\] must be'):
        nfp.accumulated_step([(x, y), (x,)])
    with pytest.raises(ValueError, match='batches must be a sequence'):
        nfp.accumulated_step(x)
    # the loss weights are checked once, before the first rollout
    with pytest.raises(ValueError, match='loss_weights'):
        nfp.accumulated_step([(x, y), (x, y)], loss_weights=np.ones((64, 63), np.float32))
    with pytest.raises(ValueError, match='lead_weights'):
        nfp.accumulated_step([(x, y), (x, y)], lead_weights=[1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match='pos_weight'):
        nfp.accumulated_step([(x, y)], pos_weight=2.0)
    with pytest.raises(ValueError, match='fused'):
        nfp.accumulated_step([(x, y)], fused=True)
    # a clip count may differ: that is no refusal, the call goes on to zero_grad (which the fixture turns into a failure)
    with pytest.raises(AssertionError, match='a launch was reached'):
        nfp.accumulated_step([(x, y), (torch.zeros(2, 2, 64, 64, 1), torch.zeros(2, T_, 64, 64, 1))])


@pytest.mark.parametrize('bad', [0, -1, 1.0, 2.5, '2', None, True])
def test_accumulate_must_be_a_positive_integer(cpu_predictor, bad):
    nfp = cpu_predictor
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    loader = TinyLoader([(x[None], y[None], torch.zeros(1))], (64, 64))
    with pytest.raises(ValueError, match='accumulate'):
        nfp.train(loader, loader, n_epochs=1, accumulate=bad)
    with pytest.raises(ValueError, match='accumulate'):
        nfp.make_graphed_step(x, y, accumulate=bad)
    assert not nfp.training_initiated


def test_train_refuses_a_real_truncation_under_accumulation(cpu_predictor):
    nfp = cpu_predictor
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    loader = TinyLoader([(x[None], y[None], torch.zeros(1))] * 2, (64, 64))
    for tb in (1, T_ - 1):
        with pytest.raises(ValueError, match='accumulate.*truncated_backprop'):
            nfp.train(loader, loader, n_epochs=1, accumulate=2, truncated_backprop=tb)
    assert not nfp.training_initiated
    # a truncation that covers every output step, or none, is no refusal: the call goes on to the first step
    for tb in (0, None, T_, 45):
        with pytest.raises(AssertionError, match='a launch was reached'):
            nfp.train(loader, loader, n_epochs=1, accumulate=2, truncated_backprop=tb)


def test_micro_weights_and_group_scale_are_exact():
    from model.mpnnlstm import check_accumulate, group_scale, micro_weights
    assert micro_weights([1]) == [1.0] and micro_weights([7]) == [1.0]
    assert micro_weights([1, 1]) == [0.5, 0.5]
    assert micro_weights([4, 4, 4, 4]) == [0.25] * 4
    assert micro_weights([1, 2]) == [1 / 3, 2 / 3]
    assert micro_weights([2, 1, 1]) == [0.5, 0.25, 0.25]
    assert micro_weights([32, 32, 5]) == [32 / 69, 32 / 69, 5 / 69]
    assert micro_weights(iter([3, 1])) == [0.75, 0.25]
    for bad in ([], [0, 1], [2, -1]):
        with pytest.raises(ValueError, match='batches'):
            micro_weights(bad)
    # the form the sum takes them in: integer multiples and one scale, n_i * scale = w_i; equal clip counts are plain sums
    from model.mpnnlstm import micro_multipliers
    assert micro_multipliers([1, 1, 1]) == ([1, 1, 1], 1 / 3) and micro_multipliers([32, 32]) == ([1, 1], 0.5)
    assert micro_multipliers([1, 2]) == ([1, 2], 1 / 3) and micro_multipliers([4, 2, 2]) == ([2, 1, 1], 0.25)
    assert micro_multipliers([6, 9]) == ([2, 3], 0.2) and micro_multipliers([5]) == ([1], 1.0)
    for clips in ([1, 1, 1], [3, 5, 2], [32, 32, 5], [4, 4]):
        mult, scale = micro_multipliers(clips)
        assert all(isinstance(n, int) for n in mult) and scale == group_scale(sum(mult))
        np.testing.assert_allclose([n * scale for n in mult], micro_weights(clips), rtol=1e-15)
    with pytest.raises(ValueError, match='batches'):
        micro_multipliers([])
    assert group_scale(1) == 1.0 and group_scale(2) == 0.5 and group_scale(3) == 1 / 3 and group_scale(4) == 0.25
    assert group_scale(1, 2) == 0.5 and group_scale(3, 2) == 1 / 6 and group_scale(2, 8) == 1 / 16
    # a short last group replays with its own scale: j of the k = 3 graphs
    assert [group_scale(j, 1) for j in (3, 2, 1)] == [1 / 3, 0.5, 1.0]
    for bad in ((0, 1), (1, 0)):
        with pytest.raises(ValueError, match='batches'):
            group_scale(*bad)
    assert check_accumulate(1) == 1 and check_accumulate(np.int64(4)) == 4 and type(check_accumulate(np.int64(4))) is int


def test_micro_groups_are_consecutive_and_the_last_may_be_short(cpu_predictor):
    nfp = cpu_predictor
    items = [(torch.full((1, 2, 4, 4, 1), float(i)), torch.full((1, T_, 4, 4, 1), float(i)), torch.zeros(1)) for i in range(5)]
    loader = TinyLoader(items, (4, 4))
    for k, want in ((1, [[0], [1], [2], [3], [4]]), (2, [[0, 1], [2, 3], [4]]), (3, [[0, 1, 2], [3, 4]]), (5, [[0, 1, 2, 3, 4]]),
                    (8, [[0, 1, 2, 3, 4]])):
        groups = list(nfp._micro_groups(loader, None, k))
        assert [[int(x[0, 0, 0, 0]) for x, _, _ in g] for g in groups] == want
        assert all(tuple(x.shape) == (2, 4, 4, 1) and tuple(y.shape) == (T_, 4, 4, 1) and c is None for g in groups for x, y, c in g)
