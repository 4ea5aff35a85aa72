"""Trainable selections on the host (set_trainable, training_only, train(trainable=)): the pure resolution, every refusal that
needs no device, and the parameter-list form of the step against torch's own rule for requires_grad=False parameters -- a deep
copy of the model under torch.optim.Adam over the trainable parameters alone, fed the same gradients."""
import copy
import inspect
import os

import pytest
import torch

from helpers import ROOT, TinyLoader
from qtmpnn.trainable import check_patterns, encoder_frozen, flat_mask, resolve_trainable

NAMES = ['encoder.rnns.0.b_i', 'encoder.norm_h.weight', 'decoder.rnns.0.b_i', 'decoder.fc_out1.lins.0.weight',
         'decoder.fc_out2.bias', 'decoder.norm_o.weight']
T_ = 2


# -- the pure parts ---------------------------------------------------------------------------------------------------------------
def test_resolve_keeps_the_order_of_the_names_and_takes_the_union_of_the_patterns():
    assert resolve_trainable(NAMES, None) == (True,) * 6
    assert resolve_trainable(NAMES, ('decoder.*',)) == (False, False, True, True, True, True)
    assert resolve_trainable(NAMES, ['decoder.fc_out*']) == (False, False, False, True, True, False)
    # overlapping patterns, given in another order than the names: a union, in the order of the names
    assert resolve_trainable(NAMES, ('decoder.norm_o.*', 'decoder.*', 'encoder.norm_h.weight')) == (False, True, True, True, True, True)
    assert resolve_trainable(NAMES, ('*.b_i',)) == (True, False, True, False, False, False)
    assert resolve_trainable(NAMES, ('decoder.fc_out[12].*',)) == (False, False, False, True, True, False)
    assert resolve_trainable(reversed(NAMES), ('encoder.*',)) == (False, False, False, False, True, True)
    assert check_patterns(None) is None and check_patterns(['a', 'b']) == ('a', 'b')


def test_the_cut_applies_only_to_a_wholly_frozen_encoder():
    assert encoder_frozen(NAMES, resolve_trainable(NAMES, ('decoder.*',)))
    assert not encoder_frozen(NAMES, resolve_trainable(NAMES, ('decoder.fc_out*', 'encoder.norm_h.weight')))
    assert not encoder_frozen(NAMES, resolve_trainable(NAMES, None))
    assert not encoder_frozen(NAMES[2:], (True, False, False, True)), 'no encoder, no cut'


def test_the_mask_covers_the_flat_vector_by_the_name_table():
    table = [('a', 0, (2, 3)), ('b', 6, (4,)), ('c', 10, ()), ('d', 11, (1, 2))]
    m = flat_mask(table, (True, False, True, False))
    assert m.dtype == torch.float32 and m.tolist() == [1.0] * 6 + [0.0] * 4 + [1.0] + [0.0] * 2
    g = torch.arange(13.0) - 6.5
    assert torch.equal((g * m)[m == 1], g[m == 1]) and not bool((g * m)[m == 0].any())


BAD = [('decoder.*', TypeError, 'plain string'), (b'decoder.*', TypeError, 'plain string'), ((), ValueError, 'empty'),
       ([], ValueError, 'empty'), (('decoder.*', 3), TypeError, 'every pattern must be a string'), (7, TypeError, 'sequence'),
       ({'decoder.*'}, TypeError, 'sequence'), (('decode.*',), ValueError, r"'decode\.\*' matches no parameter name.*'encoder', 'decoder'"),
       (('decoder.*', 'Decoder.*'), ValueError, r"'Decoder\.\*' matches no parameter name")]


@pytest.mark.parametrize('bad,error,match', BAD, ids=[repr(b) for b, _, _ in BAD])
def test_resolve_refuses_by_name(bad, error, match):
    with pytest.raises(error, match='^trainable: .*' + match):
        resolve_trainable(NAMES, bad)


# -- the predictor ----------------------------------------------------------------------------------------------------------------
def _predictor(monkeypatch, tmp_path, **kwargs):
    """A predictor without a device that records what would run (tests/test_ema_host.py's)."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kwargs)
    nfp.ran = []
    record = lambda what: lambda *a, **k: nfp.ran.append(what)
    monkeypatch.setattr(nfp, 'train_step', record('train_step'))
    monkeypatch.setattr(nfp, '_inference', record('_inference'))
    monkeypatch.setattr(Seq2Seq, 'forward', record('forward'))
    monkeypatch.setattr(_lib, 'call', record('call'))
    monkeypatch.setattr(_lib, 'load', record('load'))
    return nfp


@pytest.fixture
def cpu_predictor(monkeypatch, tmp_path):
    return _predictor(monkeypatch, tmp_path)


def _loader(n=2):
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    return TinyLoader([(x[None], y[None], torch.zeros(1))] * n, (64, 64))


def _state(nfp):
    """Everything a refusal must leave alone: the selection, requires_grad, the parameters' bits, the cut."""
    return (nfp._trainable, [p.requires_grad for p in nfp.model.parameters()], [p.detach().clone() for p in nfp.model.parameters()],
            nfp.model.encoder_cut)


def _same_state(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and a[3] == b[3]


@pytest.mark.parametrize('bad,error,match', BAD, ids=[repr(b) for b, _, _ in BAD])
def test_a_bad_selection_is_refused_by_name_before_anything_runs(cpu_predictor, bad, error, match):
    nfp = cpu_predictor
    with pytest.raises(error, match='^trainable: '):
        nfp.train(_loader(), _loader(), n_epochs=1, trainable=bad)
    assert nfp.ran == [] and not nfp.training_initiated
    with pytest.raises(error, match='^trainable: '):
        nfp.set_trainable(bad)                      # (before the complaint about the missing optimiser)
    nfp.initiate_training(0.01, 0.5)
    nfp.set_trainable(('decoder.*',))
    before = _state(nfp)
    for refused in (lambda: nfp.set_trainable(bad), lambda: nfp.training_only(bad).__enter__(),
                    lambda: nfp.train(_loader(), _loader(), n_epochs=1, trainable=bad)):
        with pytest.raises(error, match='^trainable: '):
            refused()
    assert _same_state(before, _state(nfp)) and nfp.ran == []


def test_the_selection_follows_the_optimiser(cpu_predictor):
    nfp = cpu_predictor
    everything = tuple(n for n, _ in nfp.model.named_parameters())
    assert nfp.trainable_names == everything
    nfp.set_trainable(None)                         # all-trainable on what is all-trainable needs no optimiser
    with pytest.raises(ValueError, match='^trainable: .*initiate_training'):
        nfp.set_trainable(('decoder.*',))
    assert not nfp.training_initiated and nfp.ran == []
    nfp.initiate_training(0.01, 0.5)
    nfp.set_trainable(('decoder.*',))
    assert nfp.trainable_names == tuple(n for n in everything if n.startswith('decoder.')) and nfp.model.encoder_cut
    assert [p.requires_grad for p in nfp.model.parameters()] == [n.startswith('decoder.') for n in everything]
    nfp.set_trainable(('decoder.fc_out*', 'encoder.norm_h.weight'))
    assert not nfp.model.encoder_cut, 'a partly frozen encoder keeps its graph'
    assert nfp.trainable_names == tuple(n for n in everything if n.startswith('decoder.fc_out') or n == 'encoder.norm_h.weight')
    nfp.initiate_training(0.01, 0.5)
    assert nfp.trainable_names == everything and not nfp.model.encoder_cut and all(p.requires_grad for p in nfp.model.parameters())
    assert nfp.ran == []


def test_the_block_restores_nests_and_survives_an_exception(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    with nfp.training_only(('decoder.*',)) as inside:
        assert inside is nfp and nfp._trainable == ('decoder.*',) and nfp.model.encoder_cut
        with nfp.training_only(['decoder.fc_out*']):
            assert nfp._trainable == ('decoder.fc_out*',)
            with nfp.training_only(None):
                assert nfp._trainable is None and not nfp.model.encoder_cut
            assert nfp._trainable == ('decoder.fc_out*',)
        assert nfp._trainable == ('decoder.*',)
        with pytest.raises(KeyError, match='inside'):
            with nfp.training_only(('encoder.*',)):
                assert not nfp.model.encoder_cut
                raise KeyError('inside')
        assert nfp._trainable == ('decoder.*',) and nfp.model.encoder_cut
        assert [p.requires_grad for n, p in nfp.model.named_parameters()] == [n.startswith('decoder.') for n, _ in nfp.model.named_parameters()]
    assert nfp._trainable is None and all(p.requires_grad for p in nfp.model.parameters()) and not nfp.model.encoder_cut


def test_remesh_input_models_refuse_the_cut_and_allow_masking(monkeypatch, tmp_path):
    nfp = _predictor(monkeypatch, tmp_path, remesh_input=True)
    nfp.initiate_training(0.01, 0.5)
    before = _state(nfp)
    with pytest.raises(NotImplementedError, match='^trainable: .*remesh_input=True'):
        nfp.set_trainable(('decoder.*',))
    with pytest.raises(NotImplementedError, match='^trainable: .*remesh_input=True'):
        nfp.train(_loader(), _loader(), n_epochs=1, trainable=('decoder.*',))
    assert _same_state(before, _state(nfp)) and nfp.ran == []
    nfp.set_trainable(('decoder.*', 'encoder.norm_c.bias'))
    assert not nfp.model.encoder_cut and len(nfp.trainable_names) == 1 + sum(n.startswith('decoder.') for n, _ in nfp.model.named_parameters())


def _stepper(nfps):
    """One optimiser step on every predictor of `nfps` with the same fixed random gradients, through _clip_and_step; a frozen
    parameter is handed a gradient all the same, as a backward that knows nothing of the selection would leave one."""
    g = torch.Generator().manual_seed(4)

    def step(max_norm=1.0):
        grads = [torch.randn(p.shape, generator=g) for p in nfps[0].model.parameters()]
        for nfp in nfps:
            for p, gr in zip(nfp.model.parameters(), grads):
                p.grad = gr.clone() if p.requires_grad else None
            nfp._clip_and_step(nfp._grads_ready(), max_norm)
        return grads
    return step


def test_the_step_is_torchs_rule_for_frozen_parameters(cpu_predictor):
    """The parameter-list form against the oracle itself: a copy of the model whose frozen parameters have requires_grad=False,
    under torch's clip_grad_norm_ and Adam over the trainable ones."""
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    twin = copy.deepcopy(nfp.model)
    sel = ('decoder.fc_out*', 'decoder.norm_o.*', 'encoder.rnns.0.b_i')
    nfp.set_trainable(sel)
    flags = resolve_trainable([n for n, _ in twin.named_parameters()], sel)
    chosen = [p for p, f in zip(twin.parameters(), flags) if f]
    for p, f in zip(twin.parameters(), flags):
        p.requires_grad_(f)
    opt = torch.optim.Adam(chosen, lr=0.01)
    start = [p.detach().clone() for p in nfp.model.parameters()]
    step = _stepper([nfp])
    for _ in range(3):
        grads = step(max_norm=1.0)              # (a norm small enough that the clipping acts: the norm over the trainable ones)
        for p, gr, f in zip(twin.parameters(), grads, flags):
            p.grad = gr.clone() if f else None
        assert float(torch.nn.utils.clip_grad_norm_(chosen, max_norm=1.0)) > 1.0
        opt.step()
    moved = 0
    for (k, p), q, s, f in zip(nfp.model.named_parameters(), twin.parameters(), start, flags):
        assert torch.equal(p, q), k
        assert f or torch.equal(p, s), k
        moved += int(f and not torch.equal(p, s))
        if f:
            for key in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(nfp.optimizer.state[p][key], opt.state[q][key]), (k, key)
        else:
            assert not nfp.optimizer.state.get(p), k
    assert moved == sum(flags)


def test_the_moments_rule_and_the_one_step_count(cpu_predictor, tmp_path):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    step = _stepper([nfp])
    step(), step()
    named = dict(nfp.model.named_parameters())
    kept = {k: (nfp.optimizer.state[p]['exp_avg'].clone(), nfp.optimizer.state[p]['exp_avg_sq'].clone()) for k, p in named.items()}
    assert all(bool(m.any()) and bool(v.any()) for m, v in kept.values())
    nfp.set_trainable(('decoder.*',))
    for k, p in named.items():
        st = nfp.optimizer.state[p]
        if k.startswith('decoder.'):
            assert torch.equal(st['exp_avg'], kept[k][0]) and torch.equal(st['exp_avg_sq'], kept[k][1]), k
        else:
            assert not bool(st['exp_avg'].any()) and not bool(st['exp_avg_sq'].any()), k
    frozen = {k: p.detach().clone() for k, p in named.items() if k.startswith('encoder.')}
    step()
    assert all(torch.equal(named[k], v) for k, v in frozen.items())
    # torch's Adam leaves a skipped parameter's count behind; the file holds one count, and a thawed entry continues under it
    nfp.save_checkpoint(tmp_path / 'c.pt')
    assert torch.load(tmp_path / 'c.pt', weights_only=True)['optimizer']['step'] == 3
    nfp.set_trainable(None)
    assert {float(nfp.optimizer.state[p]['step']) for p in named.values()} == {3.0}
    thawed = named['encoder.norm_h.weight']
    assert not bool(nfp.optimizer.state[thawed]['exp_avg'].any()), 'a thawed entry restarts from zero moments'
    step()
    assert not torch.equal(thawed, frozen['encoder.norm_h.weight'])
    assert {float(nfp.optimizer.state[p]['step']) for p in named.values()} == {4.0}


def test_inside_averaged_weights_the_selection_is_refused(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    nfp.set_ema(0.9)
    _stepper([nfp])()
    with nfp.averaged_weights():
        before = _state(nfp)
        for refused in (lambda: nfp.set_trainable(('decoder.*',)), lambda: nfp.set_trainable(None),
                        lambda: nfp.training_only(('decoder.*',)).__enter__()):
            with pytest.raises(RuntimeError, match=r'^trainable: set_trainable\(\) inside averaged_weights'):
                refused()
        assert _same_state(before, _state(nfp))
    nfp.set_trainable(('decoder.*',))
    assert nfp.ema is not None and nfp.ema.updates == 1, 'the average is untouched by the selection'


def test_train_holds_the_selection_for_the_call(cpu_predictor, monkeypatch):
    nfp = cpu_predictor
    seen = []
    monkeypatch.setattr(nfp, 'train_step', lambda *a, **k: seen.append((nfp._trainable, nfp.model.encoder_cut)) or torch.zeros(()))
    monkeypatch.setattr(nfp, '_test_pass', lambda *a, **k: (0.0, 1))
    nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0, trainable=("decoder.*",))       # (it makes the optimiser, then applies the selection)
    assert seen == [(('decoder.*',), True)] * 2 and nfp._trainable is None and not nfp.model.encoder_cut
    nfp.set_trainable(('decoder.fc_out*',))
    nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0)            # left out: the predictor's selection stays
    assert seen[2:] == [(('decoder.fc_out*',), True)] * 2 and nfp._trainable == ('decoder.fc_out*',)
    nfp.train(_loader(1), _loader(), n_epochs=1, truncated_backprop=0, trainable=None)                  # None: everything, for the call
    assert seen[4:] == [(None, False)] and nfp._trainable == ('decoder.fc_out*',)

    def fails(*a, **k):
        raise KeyError('inside')
    monkeypatch.setattr(nfp, 'train_step', fails)
    with pytest.raises(KeyError, match='inside'):
        nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0, trainable=('decoder.*',))
    assert nfp._trainable == ('decoder.fc_out*',) and nfp.model.encoder_cut


def test_a_captured_step_is_held_to_its_selection(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    nfp.set_trainable(['decoder.*'])
    nfp._trainable_guard(('decoder.*',))
    for now in (None, ('decoder.fc_out*',)):
        nfp.set_trainable(now)
        with pytest.raises(RuntimeError, match=r"^trainable: this step was captured under trainable=\('decoder\.\*',\)"):
            nfp._trainable_guard(('decoder.*',))
    nfp.set_trainable(('decoder.*',))
    nfp._trainable_guard(('decoder.*',))


def test_the_surface_is_what_it_was():
    from model.mpnnlstm import NextFramePredictorS2S as P
    from qtmpnn import _lib
    names = list(inspect.signature(P.train).parameters)
    assert names == ['self', 'loader_train', 'loader_test', 'climatology', 'n_epochs', 'lr', 'lr_decay', 'mask', 'high_interest_region',
                     'truncated_backprop', 'graph_structure', 'use_graph', 'accumulate', 'pos_weight', 'test_graph', 'patience',
                     'min_delta', 'restore_best', 'keep_best', 'monitor', 'loss_weights', 'lead_weights']
    assert list(inspect.signature(P.set_trainable).parameters) == ['self', 'patterns']
    assert list(inspect.signature(P.training_only).parameters) == ['self', 'patterns']
    assert isinstance(P.trainable_names, property) and 'trainable=patterns' in P.train.__doc__
    assert len(_lib.exported_names()) == 91
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'set_trainable' in readme and '(91 entry points)' in readme
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'set_trainable' in design and 'zero moments' in design


def test_an_unknown_keyword_is_still_a_type_error(cpu_predictor):
    with pytest.raises(TypeError, match='trainables'):
        cpu_predictor.train(_loader(), _loader(), n_epochs=1, trainables=('decoder.*',))
    assert cpu_predictor.ran == []
