"""set_recompute / recomputing, host side: the switch, its refusals (by name, before anything reaches a device), the signatures and
the entry-point count it must leave alone, and the bookkeeping of qtmpnn.recompute on plain CPU tensors."""
import inspect

import pytest
import torch

T_ = 3


def _predictor(**kw):
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kw)


def test_default_and_round_trip():
    nfp = _predictor()
    assert nfp.recompute is None and nfp.model.recompute is None
    nfp.set_recompute('step')
    assert nfp.recompute == 'step' and nfp.model.recompute == 'step'
    nfp.set_recompute(None)
    assert nfp.recompute is None and nfp.model.recompute is None
    with pytest.raises(AttributeError):
        nfp.recompute = 'step'                # read-only: set_recompute is the way in


@pytest.mark.parametrize('bad', ['steps', True, 1, 'Step', 0, False])
def test_other_values_are_refused_by_name(bad):
    nfp = _predictor()
    with pytest.raises(ValueError, match='set_recompute'):
        nfp.set_recompute(bad)
    with pytest.raises(ValueError, match='set_recompute'):
        with nfp.recomputing(bad):
            raise AssertionError('the block ran')
    assert nfp.recompute is None and not nfp.training_initiated


def test_recomputing_restores_the_mode():
    nfp = _predictor()
    with nfp.recomputing('step') as inside:
        assert inside is nfp and nfp.recompute == 'step'
        with nfp.recomputing(None):
            assert nfp.recompute is None
        assert nfp.recompute == 'step'
    assert nfp.recompute is None
    nfp.set_recompute('step')
    with pytest.raises(KeyError):
        with nfp.recomputing(None):
            assert nfp.recompute is None
            raise KeyError('x')
    assert nfp.recompute == 'step'


def test_signatures_and_entry_points_are_what_they_were():
    from model.mpnnlstm import NextFramePredictorS2S as P
    from qtmpnn import _lib
    for meth, before in (('train', 'use_graph'), ('make_graphed_step', 'force_multi')):
        params = inspect.signature(getattr(P, meth)).parameters
        names = list(params)
        assert params['accumulate'].default == 1, meth
        assert names.index('accumulate') == names.index(before) + 1 == names.index('pos_weight') - 1, (meth, names)
    for meth in ('forward_loss', 'train_step', 'truncated_backward', 'make_graphed_step', 'train', 'accumulated_step'):
        names = list(inspect.signature(getattr(P, meth)).parameters)
        assert names[-2:] == ['loss_weights', 'lead_weights'], (meth, names)
        assert not any('recompute' in n for n in names), (meth, names)
    assert list(inspect.signature(P.accumulated_step).parameters) == [
        'self', 'batches', 'mask', 'high_interest_region', 'graph_structure', 'max_norm', 'fused', 'pos_weight', 'loss_weights',
        'lead_weights']
    assert list(inspect.signature(P.train_step).parameters) == [
        'self', 'x', 'y', 'concat_layers', 'mask', 'high_interest_region', 'graph_structure', 'max_norm', 'fused', 'pos_weight',
        'loss_weights', 'lead_weights']
    assert list(inspect.signature(P.set_recompute).parameters) == ['self', 'mode']
    assert len(_lib.exported_names()) == 91


def test_remesh_input_is_refused_before_any_launch(monkeypatch):
    from qtmpnn import _lib

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(_lib, 'call', launched)
    nfp = _predictor(remesh_input=True)
    nfp.set_recompute('step')                                       # the switch itself is no refusal
    x = torch.zeros(3, 64, 64, 1)
    with pytest.raises(NotImplementedError, match=r"set_recompute\('step'\).*remesh_input=True"):
        nfp.model.process_inputs(x)
    with pytest.raises(NotImplementedError, match='set_recompute'):
        nfp.model(x, None)
    # without autograd the mode is a no-op: the call goes on to the mesh build (which wants a device here)
    with torch.no_grad(), pytest.raises(RuntimeError, match='must live on the GPU'):
        nfp.model.process_inputs(x)
    assert not nfp.training_initiated


def test_checkpoint_fields_do_not_know_the_mode():
    nfp = _predictor()
    before = nfp._description()
    nfp.set_recompute('step')
    assert nfp._description() == before and 'recompute' not in str(before)


def test_segment_bookkeeping_on_cpu_tensors():
    """qtmpnn.recompute.segment with a step made of torch ops: same values and gradients as the plain call, the GradAcc use
    indices of the first run are the replay's (and `uses` counts each use once), a shared tensor is one leaf of the replay, and
    without autograd it is the plain call."""
    from qtmpnn import ops, recompute

    @recompute.register_record
    class Rec:
        __slots__ = ('W', 'acc')

        def __init__(self, W, acc):
            self.W, self.acc = W, acc

    seen = []

    def step(x, h, pk, scale):
        seen.append((pk['cell'].acc.enter(), recompute.replaying(), torch.is_grad_enabled()))
        hn = torch.tanh(x @ pk['cell'].W + (h if h is not None else 0) * pk['b']) * scale
        return hn[:, :2], [hn, None]

    def run(seg):
        torch.manual_seed(0)
        W, b = torch.randn(3, 3, requires_grad=True), torch.randn(3, requires_grad=True)
        Wp = W * 1.0
        acc = ops.GradAcc()
        pk = {'cell': Rec(Wp, acc), 'b': b, 'same': [Wp, b]}
        xs = torch.randn(2, 4, 3)
        h, outs = None, []
        for t in range(2):
            y, (h, none) = seg(step, xs[t], h, pk, 0.5) if seg else step(xs[t], h, pk, 0.5)
            assert none is None
            outs.append(y)
        loss = sum(o.sum() for o in outs) + h.sum()
        loss.backward()
        return loss.detach(), W.grad, b.grad, acc

    plain = run(None)
    assert [s[0] for s in seen] == [0, 1]
    del seen[:]
    seg = run(recompute.segment)
    # first pass: uses 0, 1 without autograd; replays, last step first, with autograd and the same indices
    assert seen == [(0, False, False), (1, False, False), (1, True, True), (0, True, True)]
    assert seg[3].uses == 2 and seg[3].cursor is None
    for a, b in zip(plain[:3], seg[:3]):
        assert torch.equal(a, b)
    del seen[:]
    with torch.no_grad():
        y, (h, _) = recompute.segment(step, torch.ones(4, 3), None, {'cell': Rec(torch.ones(3, 3), ops.GradAcc()), 'b': torch.ones(3)}, 1.0)
    assert seen == [(0, False, False)] and not y.requires_grad
    for bad in ('steps', True, 1):
        with pytest.raises(ValueError, match='set_recompute'):
            recompute.check_mode(bad)
    # an object that carries tensors and is no registered record is refused, not passed through without gradients

    class Loose:
        def __init__(self):
            self.W = torch.ones(3, 3, requires_grad=True)
    with pytest.raises(TypeError, match='register_record'):
        recompute.segment(lambda x, o: x @ o.W, torch.ones(2, 3, requires_grad=True), Loose())
    recompute._RECORDS.remove(Rec)
    assert recompute.check_mode(None) is None and recompute.check_mode('step') == 'step'
