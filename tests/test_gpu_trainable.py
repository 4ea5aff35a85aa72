"""Trainable selections on the GPU (set_trainable, training_only, train(trainable=)).  The oracle is torch's own rule for
requires_grad=False parameters, stated on this project's step: the TWIN is a deep copy of the same predictor that knows nothing
of the selection and runs the plain step -- forward, loss, backward -- after which the test itself zeroes the frozen gradient
entries (a mask it builds from named_parameters()), clips over the rest and takes the same Adam step.  Loss, parameters and both
Adam moments are compared with torch.equal; so are torch's generator and the attention-dropout call counter afterwards, since the
no-grad encoder of the cut must draw the masks of the plain step (the models run in train() mode with dropout 0.1 where no
capture is involved: torch's generator replays differently inside a capture, as tests/test_gpu_ema.py notes).

64 x 64 frames, 2 clips, 3 in / 2 out, hidden 8, one conv layer: ChebConv, GCNConv, TransformerConv and MHTransformerConv.  The
first and the third train on the flat vector under FlatAdam (one mask multiplication), the other two on a parameter list under
torch's Adam (requires_grad_(False))."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

from helpers import TinyLoader, dev, grad_close

pytestmark = pytest.mark.gpu

T_IN, T_OUT, NORM = 3, 2, 0.05          # (a clipping norm far below the gradients' so that the norm itself is compared)
CONVS = ['ChebConv', 'GCNConv', 'TransformerConv', 'MHTransformerConv']
DECODER = ('decoder.*',)
MASKING = ('decoder.fc_out*', 'encoder.norm_h.weight')          # one encoder parameter stays trainable: no cut, masking only
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 58:] = True


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)             # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _clips():
    """Eight clips (x (8, T_IN, 64, 64, 1), y (8, T_OUT, 64, 64, 1)) on the device, made once, not modified."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(7, 0, 8, T_IN, T_OUT, n_digits=1, pixel_noise=0.02)
    return torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())


def _batch(i):
    x, y = _clips()
    return x[2 * (i % 4):2 * (i % 4) + 2], y[2 * (i % 4):2 * (i % 4) + 2]


def _loaders(n=2):
    x, y = (t.cpu() for t in _clips())
    item = lambda a: (x[a:a + 2], y[a:a + 2], torch.zeros(1))
    return TinyLoader([item(2 * i) for i in range(n)], (64, 64)), TinyLoader([item(6)], (64, 64))


def _pair(conv, capturable=False, static=False, train_mode=True, n=2, **kwargs):
    """n predictors with the same weights: one is made, the others are deep copies; each then gets its own optimiser."""
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(5)
    first = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                  model_kwargs=dict(hidden_size=8, dropout=0.1, n_layers=1, n_conv_layers=1, convolution_type=conv),
                                  **kwargs)
    with torch.no_grad():
        for p in first.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    first.model.train(train_mode)
    made = [first] + [copy.deepcopy(first) for _ in range(n - 1)]
    for nfp in made:
        nfp.initiate_training(lr=0.01, lr_decay=0.5, capturable=capturable)
        nfp.model.static_shapes = static
    assert all((nfp.flat is not None) == (conv in ('ChebConv', 'TransformerConv')) for nfp in made)
    return made


def _flags(nfp, patterns):
    from qtmpnn.trainable import resolve_trainable
    return resolve_trainable([n for n, _ in nfp.model.named_parameters()], patterns)


def _mask_gradients(twin, patterns):
    """What the test does to the twin's gradient after its plain backward: the frozen entries become zero (the flat vector) or
    None (the parameter list).  Returns the tensors the norm is taken over."""
    flags = _flags(twin, patterns)
    if twin.flat is not None:
        clip = twin._grads_ready()
        mask = torch.cat([torch.full((p.numel(),), float(f), device=dev()) for p, f in zip(twin.model.parameters(), flags)])
        twin.flat.param.grad.mul_(mask)
        return clip
    for p, f in zip(twin.model.parameters(), flags):
        if not f:
            p.grad = None
    return [p for p, f in zip(twin.model.parameters(), flags) if f]


def _twin_step(twin, patterns, backward, max_norm=NORM):
    """The oracle's step: backward() is the plain form's forward + loss + backward on the twin -> its loss."""
    loss = backward()
    twin._clip_and_step(_mask_gradients(twin, patterns), max_norm)
    return loss


def _plain_backward(twin, i):
    def run():
        twin.zero_grad()
        loss = twin.forward_loss(*_batch(i), None, MASK)
        loss.backward()
        return loss.detach()
    return run


def _seeded(run):
    """run() from fixed seeds of everything a step draws from -> (its result, torch's generator state and the attention-dropout
    state afterwards)."""
    from qtmpnn import ops
    torch.manual_seed(11)
    random.seed(3)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())
    out = run()
    return out, (torch.cuda.get_rng_state(dev()), torch.get_rng_state(), ops.dropout_state(dev()), random.getstate())


def _same_draws(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "torch's generators differ after the steps"
    assert a[2] == b[2], f'attention-dropout state {a[2]} != {b[2]}'
    assert a[3] == b[3]


def _adam(nfp):
    """{'exp_avg' / 'exp_avg_sq': {name: host tensor}, 'step': int} of either optimiser.  Under torch's Adam a frozen parameter has
    no state, or one whose count stands still: its moments read as what they are (zeros without a state) and the count is the
    largest, the one a checkpoint stores."""
    from qtmpnn.optim import adam_state
    if nfp.flat is not None:
        return adam_state(nfp.optimizer, nfp.model)
    out, steps = {'exp_avg': {}, 'exp_avg_sq': {}}, [0]
    for k, p in nfp.model.named_parameters():
        st = nfp.optimizer.state.get(p)
        for key in out:
            out[key][k] = st[key].detach().cpu().clone() if st else torch.zeros(p.shape)
        if st:
            steps.append(int(float(st['step'])))
    return dict(out, step=max(steps))


def _same_training_state(a, b, start=None, frozen=()):
    """Parameters and both Adam moments, by name, bit for bit; `frozen` names equal their start values."""
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    sa, sb = _adam(a), _adam(b)
    assert sa['step'] == sb['step']
    for key in ('exp_avg', 'exp_avg_sq'):
        for k in sa[key]:
            assert torch.equal(sa[key][k], sb[key][k]), (key, k)
    for k in frozen:
        assert torch.equal(dict(a.model.named_parameters())[k], start[k]), f'{k} is frozen and moved'
        assert not bool(sa['exp_avg'][k].any()) and not bool(sa['exp_avg_sq'][k].any()), k


def _start(nfp):
    return {k: p.detach().clone() for k, p in nfp.model.named_parameters()}


def _frozen_names(nfp, patterns):
    return [n for (n, _), f in zip(nfp.model.named_parameters(), _flags(nfp, patterns)) if not f]


def _against_the_twin(conv, patterns, cut):
    a, twin = _pair(conv)
    start = _start(a)
    a.set_trainable(patterns)
    assert a.model.encoder_cut == cut
    got, draws = _seeded(lambda: [a.train_step(*_batch(i), None, MASK, max_norm=NORM) for i in range(3)])
    want, twin_draws = _seeded(lambda: [_twin_step(twin, patterns, _plain_backward(twin, i)) for i in range(3)])
    for i, (l, w) in enumerate(zip(got, want)):
        assert torch.equal(l, w) and bool(torch.isfinite(l)), (i, l, w)
    frozen = _frozen_names(a, patterns)
    assert frozen and len(frozen) < len(start)
    _same_training_state(a, twin, start, frozen)
    moved = [k for k, p in a.model.named_parameters() if not torch.equal(p, start[k])]
    assert set(moved) == set(start) - set(frozen), 'every trainable parameter moves'
    _same_draws(draws, twin_draws)
    if a.flat is not None:
        assert float(a.optimizer.last_norm[0]) > NORM, 'the clipping does not act: the norm is not compared'
        assert torch.equal(a.optimizer.last_norm[0], twin.optimizer.last_norm[0]), 'the norm over the trainable entries'
    return a


# -- case 1: the encoder cut against the twin --------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_frozen_encoder_steps_are_the_twins(conv):
    a = _against_the_twin(conv, DECODER, cut=True)
    assert a.trainable_names == tuple(n for n, _ in a.model.named_parameters() if n.startswith('decoder.'))


# -- case 2: masking only ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_masked_steps_with_a_live_encoder_are_the_twins(conv):
    _against_the_twin(conv, MASKING, cut=False)


# -- case 3: eager = captured --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_captured_step_gives_the_eager_bits_and_keeps_its_selection(conv):
    eager, graphed = _pair(conv, capturable=True, static=True, train_mode=False)
    for nfp in (eager, graphed):
        nfp.set_trainable(DECODER)
    start = _start(eager)
    step = graphed.make_graphed_step(*_batch(0), None, MASK, warmup=1, max_norm=NORM)
    assert step.trainable == DECODER
    eager.train_step(*_batch(0), None, MASK, max_norm=NORM)
    for i in (1, 2):
        le, lg = eager.train_step(*_batch(i), None, MASK, max_norm=NORM), step(*_batch(i))
        assert torch.equal(le, lg), (i, le, lg)
    _same_training_state(graphed, eager, start, _frozen_names(eager, DECODER))
    before = _start(graphed)
    for other in (None, MASKING):
        graphed.set_trainable(other)
        with pytest.raises(RuntimeError, match=r"^trainable: this step was captured under trainable=\('decoder\.\*',\)"):
            step(*_batch(0))
    assert all(torch.equal(p, before[k]) for k, p in graphed.model.named_parameters()), 'a refused replay changes nothing'
    graphed.set_trainable(DECODER)          # the selection it was captured under again: it runs
    assert bool(torch.isfinite(step(*_batch(3))))
    step.check()


def test_captured_accumulation_keeps_its_selection():
    eager, graphed = _pair('ChebConv', capturable=True, static=True, train_mode=False)
    for nfp in (eager, graphed):
        nfp.set_trainable(DECODER)
    start = _start(eager)
    group = [_batch(0), _batch(1)]
    step = graphed.make_graphed_step(*group[0], None, MASK, warmup=1, max_norm=NORM, accumulate=2)
    eager.accumulated_step([group[0]], MASK, max_norm=NORM)
    assert torch.equal(eager.accumulated_step(group, MASK, max_norm=NORM), step(group))
    _same_training_state(graphed, eager, start, _frozen_names(eager, DECODER))
    graphed.set_trainable(None)
    with pytest.raises(RuntimeError, match='^trainable: this step was captured under'):
        step(group)


# -- case 4: the other step forms, each against its own plain twin with masked gradients ---------------------------------------------
def _accumulated(nfp):
    return lambda: nfp.accumulate_gradients([_batch(0), _batch(1)], MASK)


def _truncated(nfp):
    return lambda: nfp.truncated_backward(*_batch(0), None, MASK, truncated_backprop=1)[-1]


FORMS = {
    'accumulated': (None, lambda a: a.accumulated_step([_batch(0), _batch(1)], MASK, max_norm=NORM), _accumulated, NORM),
    'truncated': (None, lambda a: (a.truncated_backward(*_batch(0), None, MASK, truncated_backprop=1)[-1],
                                   a._clip_and_step(a._grads_ready(), None))[0], _truncated, None),
    'step': ('step', lambda a: a.train_step(*_batch(0), None, MASK, max_norm=NORM), lambda t: _plain_backward(t, 0), NORM),
    'stream': ('stream', lambda a: a.train_step(*_batch(0), None, MASK, max_norm=NORM), lambda t: _plain_backward(t, 0), NORM),
    'horizon1': (None, lambda a: a.train_step(*_batch(0), None, MASK, max_norm=NORM), lambda t: _plain_backward(t, 0), NORM),
}


@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
@pytest.mark.parametrize('form', list(FORMS))
def test_the_other_step_forms_are_their_twins(form, conv):
    mode, run, backward, max_norm = FORMS[form]
    a, twin = _pair(conv)
    start = _start(a)
    a.set_trainable(DECODER)
    under = (lambda nfp: nfp.horizon(1)) if form == 'horizon1' else (lambda nfp: nfp.recomputing(mode))
    with under(a):
        got, draws = _seeded(lambda: [run(a) for _ in range(2)])
    with under(twin):
        want, twin_draws = _seeded(lambda: [_twin_step(twin, DECODER, backward(twin), max_norm) for _ in range(2)])
    assert all(torch.equal(l, w) for l, w in zip(got, want)), (got, want)
    _same_training_state(a, twin, start, _frozen_names(a, DECODER))
    _same_draws(draws, twin_draws)


@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_stream_gradients_under_the_cut_are_the_plain_ones_up_to_rounding(conv):
    """'stream' sums the weight gradients in another order: against the PLAIN rollout (mode None, no selection) the trainable
    gradients are held to helpers.grad_close, as tests/test_gpu_stream.py holds them; the loss stays bit for bit."""
    a, plain = _pair(conv)
    a.set_trainable(DECODER)
    a.set_recompute('stream')

    def grads(nfp):
        loss = _plain_backward(nfp, 0)()
        return loss, {k: None if p.grad is None else p.grad.detach().clone() for k, p in nfp.model.named_parameters()}
    (la, ga), _ = _seeded(lambda: grads(a))
    (lp, gp), _ = _seeded(lambda: grads(plain))
    assert torch.equal(la, lp)
    names = [k for k in gp if k.startswith('decoder.')]
    assert names and all(gp[k] is not None and bool(gp[k].any()) for k in names if 'lin_key.bias' not in k)
    for k in names:
        grad_close(ga[k], gp[k], msg=k)


# -- case 5: the cut is real -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_the_cut_saves_nothing_while_the_encoder_runs(conv):
    a, plain = _pair(conv)
    a.set_trainable(DECODER)
    saved, encoder_calls, loss = {}, {}, {}
    for name, nfp in (('cut', a), ('plain', plain)):
        count, calls, at_handover = [0], [0], []
        inputs = nfp.model.process_inputs

        def process_inputs(*args, **kw):        # the encoder phase: everything up to the hand-over of the state to the decoder
            out = inputs(*args, **kw)
            at_handover.append(calls[0])
            return out

        def pack(t):
            count[0] += t.numel() * t.element_size()
            calls[0] += 1
            return t
        nfp.model.process_inputs = process_inputs
        nfp.zero_grad()
        try:
            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                (l, _) = _seeded(lambda: nfp.forward_loss(*_batch(0), None, MASK))
        finally:
            del nfp.model.process_inputs
        l.backward()
        saved[name], encoder_calls[name], loss[name] = count[0], at_handover[0], l.detach()
    print(f"{conv}: bytes saved for the backward: plain {saved['plain']}, frozen encoder {saved['cut']}; tensors saved while the "
          f"encoder phase ran: plain {encoder_calls['plain']}, frozen encoder {encoder_calls['cut']}")
    assert torch.equal(loss['cut'], loss['plain'])
    assert encoder_calls['plain'] > 0, 'the count sees the encoder phase'
    assert encoder_calls['cut'] == 0
    assert saved['cut'] < saved['plain']


# -- case 6: the moments rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_freezing_zeroes_the_moments_and_the_next_step_leaves_the_bits(conv):
    from qtmpnn.optim import adam_state
    (a,) = _pair(conv, n=1)
    for i in range(2):
        a.train_step(*_batch(i), None, MASK)
    before = adam_state(a.optimizer, a.model)
    assert all(bool(before[key][k].any()) for key in ('exp_avg', 'exp_avg_sq') for k in before[key] if 'lin_key.bias' not in k)
    a.set_trainable(DECODER)
    after = adam_state(a.optimizer, a.model)
    for key in ('exp_avg', 'exp_avg_sq'):
        for k, t in after[key].items():
            if k.startswith('decoder.'):
                assert torch.equal(t, before[key][k]), (key, k)
            else:
                assert not bool(t.any()), (key, k)
    held = _start(a)
    a.train_step(*_batch(2), None, MASK)
    for k, p in a.model.named_parameters():
        assert torch.equal(p, held[k]) == k.startswith('encoder.'), k


# -- case 7: resume ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_a_resumed_run_under_the_same_selection_ends_in_the_same_bits(conv, tmp_path):
    whole, first, resumed = _pair(conv, n=3)
    train, test = _loaders()
    kw = dict(n_epochs=1, mask=MASK, truncated_backprop=0)
    for nfp in (whole, first):
        nfp.set_trainable(DECODER)
    _, _ = _seeded(lambda: [whole.train(train, test, **kw) for _ in range(2)])

    def interrupted():
        first.train(train, test, **kw)
        first.save_checkpoint(tmp_path / 'c.pt')
        resumed.load_checkpoint(tmp_path / 'c.pt')
        assert resumed._trainable is None, 'the selection is no training state'
        resumed.set_trainable(DECODER)
        resumed.train(train, test, **kw)
    _seeded(interrupted)
    assert resumed.train_loss == whole.train_loss and resumed.test_loss == whole.test_loss and len(whole.train_loss) == 2
    _same_training_state(resumed, whole)
    ckpt = torch.load(tmp_path / 'c.pt', weights_only=True)
    assert ckpt['format'] == 1 and not any(bool(t.any()) for k, t in ckpt['optimizer']['exp_avg'].items() if k.startswith('encoder.'))


# -- case 8: None is a no-op -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_trainable_none_is_the_call_without_the_keyword(conv):
    with_none, without = _pair(conv)
    train, test = _loaders()
    kw = dict(n_epochs=2, mask=MASK, truncated_backprop=0)
    _, da = _seeded(lambda: with_none.train(train, test, trainable=None, **kw))
    _, db = _seeded(lambda: without.train(train, test, **kw))
    assert with_none.train_loss == without.train_loss and with_none.test_loss == without.test_loss
    _same_training_state(with_none, without)
    _same_draws(da, db)
    assert with_none._train_mask is None and not with_none.model.encoder_cut


# -- case 9: train(trainable=) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_train_with_a_selection_eager_and_graphed_end_in_equal_bits(conv):
    from model.mpnnlstm import NextFramePredictorS2S
    made = []
    for use_graph in (False, True):
        torch.manual_seed(5)
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                    model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=1, convolution_type=conv))
        nfp.model.eval()
        # a captured step runs in static mode and on a capturable optimiser: its bits are those of the eager step in that mode
        # (tests/test_gpu_ema.py).  The ChebConv predictors leave the optimiser to train(), which then applies the selection
        # after making it; torch's Adam is made here, in the mode both runs share
        nfp.model.static_shapes = True
        if conv != 'ChebConv':
            nfp.initiate_training(lr=0.01, lr_decay=0.95, capturable=True)
        start = _start(nfp)
        train, test = _loaders()
        nfp.train(train, test, n_epochs=2, mask=MASK, truncated_backprop=0, use_graph=use_graph, trainable=DECODER)
        assert nfp._trainable is None and not nfp.model.encoder_cut, 'the selection held for the call only'
        assert all(torch.equal(p, start[k]) == k.startswith('encoder.') for k, p in nfp.model.named_parameters())
        made.append(nfp)
    eager, graphed = made
    assert eager.train_loss == graphed.train_loss and eager.test_loss == graphed.test_loss
    _same_training_state(graphed, eager)


def test_the_block_restores_the_selection_after_an_exception():
    (a,) = _pair('ChebConv', n=1)
    a.set_trainable(MASKING)
    mask = a._train_mask
    with pytest.raises(KeyError, match='inside'):
        with a.training_only(DECODER):
            assert a.model.encoder_cut and a._train_mask is not mask
            a.train_step(*_batch(0), None, MASK)
            raise KeyError('inside')
    assert a._trainable == MASKING and not a.model.encoder_cut
    assert torch.equal(a._train_mask, mask)


# -- case 10: the refusals that need a device --------------------------------------------------------------------------------------
def test_device_side_refusals():
    (remesh,) = _pair('ChebConv', n=1, remesh_input=True)
    start = _start(remesh)
    with pytest.raises(NotImplementedError, match='^trainable: .*remesh_input=True'):
        remesh.set_trainable(DECODER)
    assert remesh._trainable is None and remesh._train_mask is None and not remesh.model.encoder_cut
    remesh.set_trainable(MASKING)           # masking alone is allowed on them
    assert remesh._train_mask is not None and not remesh.model.encoder_cut
    assert all(torch.equal(p, start[k]) for k, p in remesh.model.named_parameters())

    (a,) = _pair('ChebConv', n=1)
    a.set_ema(0.9)
    a.train_step(*_batch(0), None, MASK)
    moments = a.optimizer.state[a.flat.param]['exp_avg'].clone()
    with a.averaged_weights():
        with pytest.raises(RuntimeError, match=r'^trainable: set_trainable\(\) inside averaged_weights'):
            a.set_trainable(DECODER)
    assert a._trainable is None and a._train_mask is None and torch.equal(a.optimizer.state[a.flat.param]['exp_avg'], moments)


# -- sensitivity does not look at the selection ------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', ['ChebConv', 'MHTransformerConv'])
def test_sensitivity_ignores_the_selection_and_restores_requires_grad(conv):
    a, plain = _pair(conv, train_mode=False)
    a.set_trainable(DECODER)
    required = [p.requires_grad for p in a.model.parameters()]
    x = _batch(0)[0]
    got, want = a.sensitivity(x, mask=MASK, leads=[1]), plain.sensitivity(x, mask=MASK, leads=[1])
    assert np.array_equal(got.maps, want.maps) and bool(np.any(got.maps)), 'the maps are gradients through the frozen encoder'
    assert [p.requires_grad for p in a.model.parameters()] == required and a.model.encoder_cut
