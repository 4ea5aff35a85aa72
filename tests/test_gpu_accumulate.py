"""Gradient accumulation on the GPU: accumulated_step / make_graphed_step(accumulate=) / train(accumulate=) on the flat path
(ChebConv and TransformerConv: one gradient vector, FlatAdam) and the per-tensor path (MHTransformerConv: torch's Adam).  One micro-batch is train_step
bit for bit; k micro-batches give the gradient and loss of the one batch of their clips under the project's bound for
gradients; a group is one optimiser step; the two captured graphs replay to the eager accumulated step."""
import numpy as np
import pytest
import torch

from helpers import TinyLoader, close, dev, grad_close

pytestmark = pytest.mark.gpu

T, H = 3, 8
FLAT = {'ChebConv': True, 'TransformerConv': True, 'MHTransformerConv': False}       # the flat path; torch's Adam per tensor
PATHS = list(FLAT)
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 52:] = True
MASK[40:, :9] = True


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    """initiate_training()'s SummaryWriter writes under the working directory; attention dropout off (TransformerConv's default
    and MHTransformerConv's default is 0.1, and two predictors draw different masks)."""
    from model.model import CONVOLUTION_KWARGS
    monkeypatch.chdir(tmp_path)
    for conv in ('TransformerConv', 'MHTransformerConv'):
        monkeypatch.setitem(CONVOLUTION_KWARGS[conv], 'dropout', 0.0)


_DATA = {}


def _clips(binary=False):
    """Five clips (x (5, T, 64, 64, 1), y) on the device, made once."""
    if binary not in _DATA:
        from qtmpnn import synthetic
        x, y = synthetic.make_batch(7, 0, 5, T, T, n_digits=1, pixel_noise=0.02)
        if binary:
            y = (y > 0.3).astype(np.float32)
        _DATA[binary] = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    return _DATA[binary]


def _batches(sizes, binary=False):
    """Consecutive micro-batches of the given clip counts, and the one batch of all their clips."""
    x, y = _clips(binary)
    out, lo = [], 0
    for b in sizes:
        out.append((x[lo:lo + b], y[lo:lo + b]))
        lo += b
    return out, (x[:lo], y[:lo])


def _fresh(conv, binary=False, capturable=False, static=False, initiate=True):
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(5)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T, output_timesteps=T, device=dev(), binary=binary,
                                model_kwargs=dict(hidden_size=H, dropout=0.0, n_layers=1, n_conv_layers=2, convolution_type=conv))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    if initiate:
        nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=capturable)
        assert (nfp.flat is not None) == FLAT[conv]
    nfp.model.static_shapes = static
    nfp.model.train()
    return nfp


def _state(nfp):
    """Parameters, Adam moments per parameter name, and the step count, on the host."""
    from qtmpnn.optim import adam_state
    st = adam_state(nfp.optimizer, nfp.model)
    return {k: p.detach().cpu().clone() for k, p in nfp.model.named_parameters()}, st['exp_avg'], st['exp_avg_sq'], st['step']


def _assert_same_bits(a, b):
    (pa, ma, va, sa), (pb, mb, vb, sb) = _state(a), _state(b)
    assert sa == sb, (sa, sb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), f'parameter {k}'
        assert torch.equal(ma[k], mb[k]), f'exp_avg {k}'
        assert torch.equal(va[k], vb[k]), f'exp_avg_sq {k}'


def _grad_vector(nfp):
    """The gradient _grads_ready hands to the optimiser, as one host vector in module.parameters() order."""
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in nfp._grads_ready()]).cpu()


_BIG = {}


def _big_batch(conv, n, binary=False, **kw):
    """Loss and gradient of ONE batch of the first n clips at the seeded weights (once per configuration)."""
    key = (conv, n, binary, tuple(sorted(kw)))
    if key not in _BIG:
        nfp = _fresh(conv, binary)
        x, y = _batches([n], binary)[1]
        nfp.zero_grad()
        loss = nfp.forward_loss(x, y, None, MASK, **kw)
        loss.backward()
        _BIG[key] = float(loss.detach()), _grad_vector(nfp)
    return _BIG[key]


def _assert_accumulates_to(conv, sizes, binary=False, **kw):
    """accumulate_gradients over micro-batches of `sizes` clips against the one batch of those clips: the loss (helpers.close) and
    the gradient, parameter by parameter (helpers.grad_close at its defaults; the key bias of a softmax attention is an exact zero
    in exact arithmetic, held with the floor the golden tests give it)."""
    from qtmpnn.flat import name_table
    loss_big, g_big = _big_batch(conv, sum(sizes), binary, **kw)
    nfp = _fresh(conv, binary)
    loss = nfp.accumulate_gradients(_batches(sizes, binary)[0], MASK, **kw)
    g = _grad_vector(nfp)
    assert g.shape == g_big.shape and bool(g_big.any())
    print(f'{conv} {sizes} {sorted(kw)}: loss {float(loss):.8f} big batch {loss_big:.8f}; '
          f'max |g - g_big| / max |g_big| = {float((g - g_big).abs().max() / g_big.abs().max()):.3e}')
    close(loss, loss_big, msg='loss')
    grad_close(g, g_big, msg='gradient vector')
    for name, off, shape in name_table(nfp.model):
        n = int(np.prod(shape))
        grad_close(g[off:off + n], g_big[off:off + n], msg=name, floor=0.05 if name.endswith('lin_key.bias') else 1e-3)


@pytest.mark.parametrize('conv', PATHS)
def test_one_micro_batch_is_train_step_bit_for_bit(conv):
    (b0, b1), _ = _batches([2, 1])
    a, b = _fresh(conv), _fresh(conv)
    for x, y in (b0, b1, b0):             # (the second and third steps start from non-zero moments)
        la, lb = a.accumulated_step([(x, y)], MASK), b.train_step(x, y, None, MASK)
        assert torch.equal(la, lb) and np.isfinite(float(la))
    _assert_same_bits(a, b)
    assert _state(a)[3] == 3


@pytest.mark.parametrize('conv', PATHS)
def test_same_inputs_give_the_same_bits(conv):
    batches, _ = _batches([1, 2, 1])
    a, b = _fresh(conv), _fresh(conv)
    for _ in range(2):
        assert torch.equal(a.accumulated_step(batches, MASK), b.accumulated_step(batches, MASK))
    _assert_same_bits(a, b)


@pytest.mark.parametrize('sizes', [(1, 1), (1, 1, 1), (1, 2), (2, 1, 2)], ids=str)
@pytest.mark.parametrize('conv', PATHS)
def test_micro_batches_accumulate_to_the_big_batch(conv, sizes):
    _assert_accumulates_to(conv, list(sizes))


@pytest.mark.parametrize('conv', PATHS)
def test_weighted_loss_accumulates_to_the_big_batch(conv):
    rng = np.random.default_rng(91)
    w = (0.25 + rng.random((64, 64))).astype(np.float32)
    w[:8] = 0.0
    _assert_accumulates_to(conv, [2, 1], loss_weights=w, lead_weights=np.array([0.5, 2.0, 1.0], np.float32))


def test_weighted_binary_loss_accumulates_to_the_big_batch():
    rng = np.random.default_rng(92)
    w = (0.25 + rng.random((64, 64))).astype(np.float32)
    _assert_accumulates_to('ChebConv', [1, 2], binary=True, loss_weights=w, lead_weights=np.array([1.0, 0.5, 1.5], np.float32),
                           pos_weight=3.0)
    _assert_accumulates_to('ChebConv', [1, 1], binary=True, pos_weight=2.0)


def _loaders(n=5):
    x, y = _clips()
    items = [(x[i:i + 1].cpu(), y[i:i + 1].cpu(), torch.zeros(1)) for i in range(n)]
    return TinyLoader(items, (64, 64)), TinyLoader(items[:1], (64, 64))


@pytest.mark.parametrize('conv', PATHS)
def test_a_group_is_one_optimiser_step(conv):
    batches, _ = _batches([1, 1, 1])
    nfp = _fresh(conv)
    assert np.isfinite(float(nfp.accumulated_step(batches, MASK))) and _state(nfp)[3] == 1
    nfp = _fresh(conv, initiate=False)
    train, test = _loaders(5)
    nfp.train(train, test, n_epochs=1, lr=1e-3, mask=MASK, truncated_backprop=0, accumulate=2)
    assert _state(nfp)[3] == 3                                      # groups of 2, 2 and 1
    assert len(nfp.train_loss) == 1 and np.isfinite(nfp.train_loss + nfp.test_loss).all()


def test_train_steps_the_groups_accumulated_step_would():
    """train(accumulate=2) over 5 items is accumulated_step on (0, 1), (2, 3), (4): the same bits, and `running` counts micro-batches."""
    train, test = _loaders(5)
    a, b = _fresh('ChebConv'), _fresh('ChebConv')
    a.train(train, test, n_epochs=1, mask=MASK, truncated_backprop=0, accumulate=2)
    items = [(a._clip(x), a._clip(y)) for x, y, _ in train]
    losses = [float(b.accumulated_step(items[lo:lo + 2], MASK)) for lo in (0, 2, 4)]
    _assert_same_bits(a, b)
    assert a.train_loss[0] == (losses[0] + losses[0] + losses[1] + losses[1] + losses[2]) / (5 + 1)        # (+1 as the reference)


@pytest.mark.parametrize('conv', PATHS)
def test_graphed_accumulated_step_matches_the_eager_one(conv):
    """make_graphed_step(accumulate=3) against eager static-mode accumulated_step from the same state, a full group and then a
    short one of 2 through the same two graphs: held as tests/test_gpu_rollout.py::test_graphed_step_matches_eager_steps holds a
    replay to its eager twin (losses 1e-6 relative, parameters rtol 1e-6 / atol 1e-7), and beyond that to the bit: for micro-batches
    of one shape the eager step sums the gradients and scales once, which is what the two graphs do."""
    x, y = _clips()
    group = [(x[0:2], y[0:2]), (x[2:4], y[2:4]), (x[1:3], y[1:3])]
    eager, graphed = _fresh(conv, capturable=True, static=True), _fresh(conv, capturable=True, static=True)
    step = graphed.make_graphed_step(*group[1], None, MASK, warmup=1, accumulate=3)
    assert step.accumulate == 3
    lw = eager.accumulated_step([group[1]], MASK)                  # the warm-up: one eager step of the batch given
    assert torch.equal(lw, graphed.last_warmup_loss)
    _assert_same_bits(eager, graphed)
    for batches in (group, group[1:], group[:1], group):
        le, lg = float(eager.accumulated_step(batches, MASK)), float(step(batches))
        print(f'{conv} {len(batches)} micro-batches: eager {le:.8f} graphed {lg:.8f}')
        assert np.isfinite(le) and abs(le - lg) <= 1e-6 * abs(le), (le, lg)
        assert le == lg, (le, lg)
    assert _state(eager)[3] == _state(graphed)[3] == 5
    for (k, p), (_, q) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
    _assert_same_bits(eager, graphed)
    for bad in ([], group + group[:1], [(x[0:1], y[0:1])]):
        with pytest.raises(ValueError, match='batches'):
            step(bad)
    assert _state(graphed)[3] == 5


def test_accumulate_1_returns_todays_step():
    x, y = _clips()
    eager, graphed = _fresh('ChebConv', capturable=True, static=True), _fresh('ChebConv', capturable=True, static=True)
    step = graphed.make_graphed_step(x[0:2], y[0:2], None, MASK, warmup=1, accumulate=1)
    assert not hasattr(step, 'accumulate')
    eager.train_step(x[0:2], y[0:2], None, MASK)
    for lo in (2, 0):
        le, lg = eager.train_step(x[lo:lo + 2], y[lo:lo + 2], None, MASK), step(x[lo:lo + 2], y[lo:lo + 2], None)
        assert torch.equal(le, lg)
    _assert_same_bits(eager, graphed)


@pytest.mark.parametrize('conv', PATHS)
def test_trainer_accumulates_as_a_captured_graph(conv):
    nfp = _fresh(conv, initiate=False)
    train, test = _loaders(5)
    nfp.train(train, test, n_epochs=2, lr=1e-3, mask=MASK, truncated_backprop=0, use_graph=True, accumulate=2)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
    assert _state(nfp)[3] == 6                                      # per epoch groups of 2, 2 and 1


def test_one_all_reduce_per_accumulated_step(monkeypatch):
    """Under two ranks (the world size faked, the collective replaced by a counter that sums over one rank) an accumulated step
    of three micro-batches hands its gradient over once and issues one collective."""
    import model.mpnnlstm as M
    batches, _ = _batches([1, 1, 1])
    calls = {'all_reduce': 0, 'ready': 0}

    def counted(t, group=None):
        calls['all_reduce'] += 1
        return t
    monkeypatch.setattr(M, 'all_reduce_sum', counted)
    nfp = _fresh('ChebConv')
    ready = nfp._grads_ready

    def counting_ready(*a, **k):
        calls['ready'] += 1
        return ready(*a, **k)
    monkeypatch.setattr(nfp, '_grads_ready', counting_ready)
    monkeypatch.setattr(nfp, '_world', lambda: 2)
    nfp.accumulated_step(batches, MASK)
    assert calls == {'all_reduce': 1, 'ready': 1}
    nfp.accumulated_step(batches[:2], MASK)
    assert calls == {'all_reduce': 2, 'ready': 2} and _state(nfp)[3] == 2
    # the per-tensor path hands its gradients over once per step too
    other = _fresh('MHTransformerConv')
    ready2, n = other._grads_ready, [0]

    def counting_ready2(*a, **k):
        n[0] += 1
        return ready2(*a, **k)
    monkeypatch.setattr(other, '_grads_ready', counting_ready2)
    other.accumulated_step(batches, MASK)
    assert n[0] == 1


def test_resumed_run_accumulates_bit_for_bit(tmp_path):
    """train(accumulate=2) for 2 epochs against 1 epoch, save_checkpoint, a fresh predictor, load_checkpoint and 1 more epoch: the
    accumulator is zero between steps, so the checkpoint (unchanged) carries everything."""
    train, test = _loaders(5)
    kw = dict(lr=1e-3, lr_decay=0.5, mask=MASK, truncated_backprop=0, accumulate=2)
    a = _fresh('ChebConv', initiate=False)
    a.train(train, test, n_epochs=2, **kw)
    b = _fresh('ChebConv', initiate=False)
    b.train(train, test, n_epochs=1, **kw)
    b.save_checkpoint(tmp_path / 'b.ckpt')
    c = _fresh('ChebConv', initiate=False)
    c.load_checkpoint(tmp_path / 'b.ckpt')
    c.train(train, test, n_epochs=1, **kw)
    _assert_same_bits(a, c)
    assert c.train_loss == a.train_loss and c.test_loss == a.test_loss
