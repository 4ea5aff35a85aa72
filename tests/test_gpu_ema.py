"""Averaged weights on the GPU (set_ema, averaged_weights, train(ema=)): the shadow of eager and captured steps against the
float64 recurrence of tests/ema_restated.py over the recorded iterates, the block that swaps the weights in place under eager and
captured rollouts, train()'s test pass on the averaged weights, and resuming across a checkpoint.  Every case on a ChebConv and on
a TransformerConv model (both one flat vector under FlatAdam: the single-head attention stack is packed as well) and on a
MHTransformerConv model (a parameter list under torch's Adam: the other form of the shadow).  64 x 64 frames, hidden 8, 2 in /
2 out, 2 clips a batch, 4 to 6 steps; eval() mode, so no run draws a dropout mask."""
import functools

import numpy as np
import pytest
import torch

import ema_restated as R
from helpers import TinyLoader, dev

pytestmark = pytest.mark.gpu

T, D = 2, 0.9
FLAT = {'ChebConv': True, 'TransformerConv': True, 'MHTransformerConv': False}       # the flat path; torch's Adam per tensor
PATHS = list(FLAT)
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 60:] = True


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)             # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _clips():
    """Eight clips (x (8, T, 64, 64, 1), y) on the device, made once, not modified."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(7, 0, 8, T, T, n_digits=1, pixel_noise=0.02)
    return torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())


def _batch(i):
    x, y = _clips()
    return x[i:i + 2], y[i:i + 2]


def _loaders():
    """(train: 2 batches of 2 clips, test: 2 batches of 2 clips) on the host."""
    x, y = (t.cpu() for t in _clips())
    item = lambda a: (x[a:a + 2], y[a:a + 2], torch.zeros(1))
    return TinyLoader([item(0), item(2)], (64, 64)), TinyLoader([item(4), item(6)], (64, 64))


def _fresh(conv, capturable=False, static=False, ema=None, seed=5, initiate=True):
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T, output_timesteps=T, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=1, convolution_type=conv))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    nfp.model.eval()
    if initiate:
        nfp.initiate_training(lr=0.01, lr_decay=0.5, capturable=capturable)
        assert (nfp.flat is not None) == FLAT[conv]
        nfp.set_ema(ema)
        assert ema is None or nfp.ema.flat == FLAT[conv]
    nfp.model.static_shapes = static
    return nfp


def _vec(ts):
    """One tensor or a list of them as one device vector (a copy)."""
    return ts.detach().reshape(-1).clone() if torch.is_tensor(ts) else torch.cat([t.detach().reshape(-1) for t in ts])


def _params(nfp):
    return _vec(list(nfp.model.parameters()))


def _shadow(nfp):
    return _vec(nfp.ema.shadow)


def _averaged(nfp):
    out = torch.empty_like(nfp.ema.shadow) if nfp.ema.flat else [torch.empty_like(s) for s in nfp.ema.shadow]
    return _vec(nfp.ema.averaged(out))


def _same_params(a, b):
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k


# -- case 1: eager steps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', PATHS)
def test_eager_steps_keep_the_bound_and_leave_training_alone(conv):
    plain, avg = _fresh(conv), _fresh(conv, ema=D)
    iterates, got = [], []
    for i in range(5):
        lp, la = plain.train_step(*_batch(i), None, MASK), avg.train_step(*_batch(i), None, MASK)
        assert torch.equal(lp, la) and bool(torch.isfinite(la)), (i, lp, la)
        iterates.append(_params(avg).cpu().numpy())
        got.append((_shadow(avg).cpu().numpy(), _averaged(avg).cpu().numpy()))
        assert avg.ema.updates == i + 1
    _same_params(plain, avg)
    assert not np.array_equal(iterates[0], iterates[-1]), 'the weights move'
    ref = R.model64(iterates, D)
    worst = [R.worst(s, m, r) for (s, m), r in zip(got, ref)]
    print(f'{conv}: {iterates[0].size} parameters; worst error / bound of (shadow, average) per update: {worst}')
    assert all(R.holds(s, m, r) for (s, m), r in zip(got, ref))
    # the checker can fail here too: the shadow is not the average, and the average is not the last iterate
    assert not R.holds(None, got[-1][0], ref[-1]) and not R.holds(None, iterates[-1], ref[-1])
    if avg.flat is not None:
        assert avg.ema.shadow.numel() == avg.flat.n and not bool(avg.flat.buffer[avg.flat.n:].any())


@pytest.mark.parametrize('conv', PATHS)
def test_accumulated_and_truncated_steps_update_once_per_optimiser_step(conv):
    nfp = _fresh(conv, ema=D)
    nfp.accumulated_step([_batch(0), _batch(2), _batch(4)], MASK)
    assert nfp.ema.updates == 1, 'one update per optimiser step, none per micro-batch'
    first = _params(nfp).cpu().numpy()
    assert R.holds(_shadow(nfp).cpu().numpy(), _averaged(nfp).cpu().numpy(), R.model64([first], D)[0])
    nfp.truncated_backward(*_batch(0), None, MASK, truncated_backprop=1)
    nfp._clip_and_step(nfp._grads_ready(), None)            # (train()'s truncated branch)
    assert nfp.ema.updates == 2
    assert R.holds(_shadow(nfp).cpu().numpy(), None, R.model64([first, _params(nfp).cpu().numpy()], D)[1])


# -- case 2: captured steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', PATHS)
def test_captured_step_gives_the_eager_shadow_and_count(conv):
    eager, graphed = _fresh(conv, True, True, ema=D), _fresh(conv, True, True, ema=D)
    step = graphed.make_graphed_step(*_batch(0), None, MASK, warmup=1)
    assert step.ema is graphed.ema and graphed.ema.updates == 1, 'the warm-up step counts, the capture does not'
    eager.train_step(*_batch(0), None, MASK)
    for i in range(1, 5):
        le, lg = eager.train_step(*_batch(i), None, MASK), step(*_batch(i))
        assert torch.equal(le, lg), (i, le, lg)
    assert eager.ema.updates == graphed.ema.updates == 5
    assert torch.equal(_shadow(eager), _shadow(graphed)) and torch.equal(_averaged(eager), _averaged(graphed))
    _same_params(eager, graphed)
    # the step keeps the setting it was captured under: off, another decay and the same decay set anew are all refused
    before = _shadow(graphed)
    kept = graphed.ema
    for other in (None, 0.5):
        graphed.set_ema(other)
        with pytest.raises(RuntimeError, match='^ema: this step was captured under ema=0.9'):
            step(*_batch(0))
    graphed.set_ema(D)
    with pytest.raises(RuntimeError, match='^ema: .*set anew'):
        step(*_batch(0))
    assert torch.equal(_vec(kept.shadow), before) and kept.updates == 5
    _same_params(eager, graphed)
    with pytest.raises(ValueError, match='^ema: no optimiser step has been averaged yet'):      # (the new average has seen none)
        with graphed.averaged_weights():
            pass


@pytest.mark.parametrize('conv', PATHS)
def test_captured_accumulated_step_gives_the_eager_shadow_and_count(conv):
    eager, graphed = _fresh(conv, True, True, ema=D), _fresh(conv, True, True, ema=D)
    step = graphed.make_graphed_step(*_batch(0), None, MASK, warmup=1, accumulate=2)
    assert step.ema is graphed.ema and graphed.ema.updates == 1
    eager.accumulated_step([_batch(0)], MASK)
    for group in ([_batch(1), _batch(3)], [_batch(2)], [_batch(4), _batch(5)]):
        le, lg = eager.accumulated_step(group, MASK), step(group)
        assert torch.equal(le, lg), (le, lg)
    assert eager.ema.updates == graphed.ema.updates == 4, 'once per call of step, not per micro-batch'
    assert torch.equal(_shadow(eager), _shadow(graphed))
    _same_params(eager, graphed)
    graphed.set_ema(None)
    with pytest.raises(RuntimeError, match='^ema: this step was captured under ema=0.9 and the predictor is now at ema=None'):
        step([_batch(0)])


@pytest.mark.parametrize('conv', PATHS)
def test_a_step_captured_without_the_average_refuses_to_run_with_one(conv):
    nfp = _fresh(conv, True, True)
    step = nfp.make_graphed_step(*_batch(0), None, MASK, warmup=1)
    assert step.ema is None
    step(*_batch(1))
    nfp.set_ema(D)
    before = _params(nfp)
    with pytest.raises(RuntimeError, match='^ema: this step was captured under ema=None and the predictor is now at ema=0.9'):
        step(*_batch(2))
    assert torch.equal(_params(nfp), before) and nfp.ema.updates == 0
    nfp.set_ema(None)
    step(*_batch(2))
    assert not torch.equal(_params(nfp), before)


def test_an_eager_optimiser_becomes_capturable_with_the_average_it_had():
    """make_graphed_step on a predictor whose optimiser is not capturable initiates training again; the average set before goes
    with it (no step was taken yet)."""
    nfp = _fresh('ChebConv', capturable=False, ema=D)
    step = nfp.make_graphed_step(*_batch(0), None, MASK, warmup=1)
    assert nfp.ema is not None and nfp.ema.decay == D and nfp.ema.updates == 1 and step.ema is nfp.ema
    step(*_batch(1))
    assert nfp.ema.updates == 2 and bool(_shadow(nfp).any())


# -- case 3: the block ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('conv', PATHS)
def test_the_block_swaps_the_weights_in_place_under_eager_and_captured_rollouts(conv):
    nfp = _fresh(conv, ema=D)
    for i in range(4):
        nfp.train_step(*_batch(i), None, MASK)
    x, _ = _batch(4)
    loader = TinyLoader([(x.cpu(), torch.zeros(2, T, 64, 64, 1), torch.zeros(1))], (64, 64))
    rollout = nfp.make_graphed_rollout(x)           # made before entering, on the live weights
    nfp.model.static_shapes = False
    outside, outside_r = nfp.predict(loader), rollout(x).cpu().numpy()
    live = _params(nfp)
    buffer = nfp.flat.buffer.clone() if nfp.flat is not None else None
    want = _averaged(nfp)
    with nfp.averaged_weights():
        assert torch.equal(_params(nfp), want)
        if buffer is not None:
            assert nfp.flat.intact(nfp.model) and not bool(nfp.flat.buffer[nfp.flat.n:].any()), 'the views and the zero pad tail'
        inside = nfp.predict(loader)
        nfp.model.static_shapes = True
        inside_static = nfp.predict(loader)
        nfp.model.static_shapes = False
        inside_graph = nfp.predict(loader, use_graph=True)
        inside_r = rollout(x).cpu().numpy()
        weights = {k: v.detach().clone() for k, v in nfp.model.state_dict().items()}
    assert torch.equal(_params(nfp), live), 'bit for bit what they were'
    if buffer is not None:
        assert torch.equal(nfp.flat.buffer, buffer) and not bool(buffer[nfp.flat.n:].any())
    assert np.isfinite(inside).all() and not np.array_equal(inside, outside) and not np.array_equal(inside_r, outside_r)
    other = _fresh(conv, seed=99, initiate=False)
    other.model.load_state_dict(weights)
    assert _same(other.predict(loader), inside), 'a second predictor with those weights'
    # captured rollouts read the parameters by pointer: the eager static-mode call's bits, the dynamic one's to 1e-6 (the figures
    # tests/test_gpu_predict_graph.py holds a capture to)
    print(f'{conv}: captured vs eager dynamic inside the block: {float(np.abs(inside_graph - inside).max()):.3g}; averaged vs live '
          f'forecast: {float(np.abs(inside - outside).max()):.3g}')
    assert _same(inside_graph, inside_static) and _same(inside_r, inside_static)
    np.testing.assert_allclose(inside_graph, inside, rtol=0, atol=1e-6)
    assert _same(nfp.predict(loader), outside) and _same(rollout(x).cpu().numpy(), outside_r), 'and the live weights\' again afterwards'
    # after an exception raised inside, too
    with pytest.raises(KeyError, match='inside'):
        with nfp.averaged_weights():
            assert torch.equal(_params(nfp), want)
            raise KeyError('inside')
    assert torch.equal(_params(nfp), live)
    if buffer is not None:
        assert torch.equal(nfp.flat.buffer, buffer)
    # no optimiser step inside, eager or captured; no nesting
    with nfp.averaged_weights():
        with pytest.raises(RuntimeError, match='^ema: an optimiser step inside averaged_weights'):
            nfp.train_step(*_batch(0), None, MASK)
        with pytest.raises(RuntimeError, match='^ema: .*re-entrant'):
            with nfp.averaged_weights():
                pass
        assert torch.equal(_params(nfp), want)
    assert torch.equal(_params(nfp), live) and nfp.ema.updates == 4
    nfp.apply_ema()
    assert torch.equal(_params(nfp), want)


# -- case 4: train(ema=) ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """A SummaryWriter stand-in that calls `after_test()` right after every test pass (train() reports 'Loss/test' next)."""

    def __init__(self, after_test):
        self.after_test = after_test

    def add_scalar(self, tag, value, step):
        if tag == 'Loss/test':
            self.after_test()

    def flush(self):
        pass


def _train(nfp, n_epochs, **kw):
    train, test = _loaders()
    nfp.train(train, test, n_epochs=n_epochs, lr=0.01, lr_decay=0.5, mask=MASK, truncated_backprop=0, **kw)
    return nfp


def _by_hand(nfp, static):
    """train()'s test pass by hand on the weights as they are: the sum of forward_loss(...).item() under no_grad over the test
    loader / (steps + 1), in static or dynamic mode."""
    static0, total, steps = nfp.model.static_shapes, 0.0, 0
    nfp.model.static_shapes = static
    try:
        for x, y, _ in _loaders()[1]:
            with torch.no_grad():
                total += nfp.forward_loss(x.to(dev()), y.to(dev()), None, MASK).item()
            steps += 1
    finally:
        nfp.model.static_shapes = static0
    return total / (steps + 1)


@pytest.mark.parametrize('test_graph', [False, True])
@pytest.mark.parametrize('conv', PATHS)
def test_train_evaluates_the_averaged_weights_and_trains_the_live_ones(conv, test_graph):
    plain = _train(_fresh(conv), 2, test_graph=test_graph)
    nfp, by_hand, live_hand, averaged = _fresh(conv), [], [], []

    def after_test():
        live_hand.append(_by_hand(nfp, test_graph))
        with nfp.averaged_weights():
            by_hand.append(_by_hand(nfp, test_graph))
        averaged.append(_averaged(nfp))
    nfp.writer = _Recorder(after_test)
    _train(nfp, 2, test_graph=test_graph, ema=D)
    print(f'{conv} test_graph={test_graph}: test_loss {nfp.test_loss} by hand on the averaged weights {by_hand}, on the live ones '
          f'{live_hand}; without ema {plain.test_loss}')
    assert nfp.ema.updates == 4 and len(by_hand) == 2 and np.isfinite(by_hand).all()
    assert nfp.test_loss == by_hand and nfp.test_loss != live_hand
    assert plain.test_loss == live_hand, 'the hand-made pass is the one train() runs'
    assert nfp.train_loss == plain.train_loss
    _same_params(nfp, plain)
    assert nfp.model.static_shapes is False
    # ema_eval=False only maintains the average
    quiet = _train(_fresh(conv), 2, test_graph=test_graph, ema=D, ema_eval=False)
    assert quiet.test_loss == plain.test_loss and quiet.train_loss == plain.train_loss and quiet.ema.updates == 4
    assert torch.equal(_shadow(quiet), _shadow(nfp))
    _same_params(quiet, plain)
    # restore_best: the parameters end as the averaged weights of the best epoch
    best = _fresh(conv)
    _train(best, 2, test_graph=test_graph, ema=D, restore_best=True)
    assert best.test_loss == nfp.test_loss and best.best_epoch in (0, 1)
    assert torch.equal(_params(best), averaged[best.best_epoch])
    assert not torch.equal(_params(best), _params(plain))
    if best.flat is not None:
        assert best.flat.intact(best.model) and not bool(best.flat.buffer[best.flat.n:].any())


# -- case 5: resume ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('conv', PATHS)
def test_resumed_run_ends_in_the_same_average(conv, use_graph, tmp_path):
    whole = _train(_fresh(conv, initiate=False), 4, use_graph=use_graph, ema=D)
    half = _train(_fresh(conv, initiate=False), 2, use_graph=use_graph, ema=D)
    half.save_checkpoint(tmp_path / 'half.pt')
    assert torch.load(tmp_path / 'half.pt', weights_only=True)['format'] == 2
    resumed = _fresh(conv, seed=99, initiate=False)
    resumed.load_checkpoint(tmp_path / 'half.pt')
    assert resumed.ema is not None and resumed.ema.updates == 4 and torch.equal(_shadow(resumed), _shadow(half))
    _train(resumed, 2, use_graph=use_graph, ema=D)
    print(f'{conv} use_graph={use_graph}: whole {whole.train_loss} {whole.test_loss}\nresumed {resumed.train_loss} {resumed.test_loss}')
    assert resumed.ema.updates == whole.ema.updates == 8
    assert torch.equal(_shadow(resumed), _shadow(whole))
    assert resumed.train_loss == whole.train_loss and resumed.test_loss == whole.test_loss and len(whole.test_loss) == 4
    _same_params(resumed, whole)


@pytest.mark.parametrize('conv', PATHS)
def test_load_switches_the_average_off_and_a_conversion_keeps_it(conv, tmp_path):
    on = _train(_fresh(conv, initiate=False), 1, ema=D)
    off = _train(_fresh(conv, initiate=False), 1)
    on.save_checkpoint(tmp_path / 'on.pt')
    off.save_checkpoint(tmp_path / 'off.pt')
    assert torch.load(tmp_path / 'off.pt', weights_only=True)['format'] == 1
    shadow = _shadow(on)
    other = _fresh(conv, seed=99, ema=0.5)
    other.load_checkpoint(tmp_path / 'on.pt', capturable=True)           # (eager file, capturable optimiser: initiated again)
    assert other.optimizer.param_groups[0]['capturable'] and other.ema.decay == D and other.ema.updates == 2
    assert torch.equal(_shadow(other), shadow)
    kept, ptr = other.ema, _first_ptr(other)
    other.load_checkpoint(tmp_path / 'on.pt', capturable=True)           # (the same mode and decay: in place)
    assert other.ema is kept and _first_ptr(other) == ptr and torch.equal(_shadow(other), shadow)
    other.load_checkpoint(tmp_path / 'off.pt')
    assert other.ema is None
    _same_params(other, off)
    # the flat shadow and the per-parameter one read each other's layout: the names and shapes are the model's either way
    st = torch.load(tmp_path / 'on.pt', weights_only=True)['ema']
    assert list(st['shadow']) == [n for n, _ in on.model.named_parameters()]
    assert torch.equal(torch.cat([t.reshape(-1) for t in st['shadow'].values()]).to(dev()), shadow)


def _first_ptr(nfp):
    s = nfp.ema.shadow
    return (s if torch.is_tensor(s) else s[0]).data_ptr()
