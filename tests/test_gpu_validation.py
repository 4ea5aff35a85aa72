"""Validation in train() on the GPU: the default call is what it was; the graphed test pass gives the eager static-mode losses
bit for bit, replays in the second epoch and captures once per batch shape; early stopping, best weights, resuming across a
checkpoint; selecting on verification products from the one rollout per test batch.  64 x 64 frames, hidden 8, 3 in / 3 out,
4 clips a batch; the test loader's last batch has 2 clips (a second shape)."""
import functools

import numpy as np
import pytest
import torch

from helpers import TinyLoader, close, dev

pytestmark = pytest.mark.gpu

T = 3
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 56:] = True
N_TRAIN, N_TEST, SHAPES = 2, 3, 2           # batches of the two loaders; distinct batch shapes of the test loader


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)             # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _loaders():
    """(train: 2 batches of 4 clips, test: batches of 4, 4 and 2 clips) on the host; made once, not modified."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(7, 0, 18, T, T, n_digits=1, pixel_noise=0.02)
    y = np.clip(y, 0.0, 1.0)        # (targets of a binary head are probabilities: torch's BCE kernel traps on one outside [0, 1])
    item = lambda a, b: (torch.from_numpy(x[a:b]), torch.from_numpy(y[a:b]), torch.zeros(1))
    return (TinyLoader([item(0, 4), item(4, 8)], (64, 64)), TinyLoader([item(8, 12), item(12, 16), item(16, 18)], (64, 64)))


def _weights():
    w = np.ones((64, 64), np.float32)
    w[20:40, 10:50] = 3.0
    return dict(loss_weights=w, lead_weights=[1.0, 2.0, 0.5])


CASES = {'cheb': dict(conv='ChebConv'),
         'transformer_eval': dict(conv='TransformerConv', eval_mode=True),
         'binary': dict(conv='ChebConv', binary=True),
         'weighted': dict(conv='ChebConv', weights=True),
         'weighted_binary': dict(conv='ChebConv', binary=True, weights=True)}


def _predictor(conv='ChebConv', binary=False, eval_mode=False, seed=3, **_):
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T, output_timesteps=T, device=dev(), binary=binary,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=1, convolution_type=conv))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    nfp.model.eval() if eval_mode else nfp.model.train()
    return nfp


def _train(nfp, n_epochs, lr=0.01, weights=False, conv=None, binary=None, eval_mode=None, **kw):
    """train() on the two loaders; a CASES row may be passed along (only its `weights` matters here)."""
    train, test = _loaders()
    nfp.train(train, test, n_epochs=n_epochs, lr=lr, lr_decay=0.5, mask=MASK, truncated_backprop=0, **(_weights() if weights else {}), **kw)
    return nfp


def _by_hand(nfp, static, fused, weights=False):
    """The test pass as the parent commit's train() wrote it: the Python sum of forward_loss(...).item() under no_grad over the
    test loader, divided by steps + 1 -- in static or dynamic mode, on the weights as they are."""
    static0, total, steps = nfp.model.static_shapes, 0.0, 0
    nfp.model.static_shapes = static
    try:
        for x, y, _ in _loaders()[1]:
            with torch.no_grad():
                total += nfp.forward_loss(x.to(dev()), y.to(dev()), None, MASK, fused=fused, **(_weights() if weights else {})).item()
            steps += 1
    finally:
        nfp.model.static_shapes = static0
    return total / (steps + 1)


class _Recorder:
    """A SummaryWriter stand-in that keeps what train() reports and, right after every test pass (train() reports 'Loss/test'
    next), calls `after_test()`: the weights are then the ones the pass ran on."""

    def __init__(self, after_test=None):
        self.scalars, self.after_test = {}, after_test

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append(value)
        if tag == 'Loss/test' and self.after_test is not None:
            self.after_test()

    def flush(self):
        pass


def _count_graphs(monkeypatch):
    made, real = [0], torch.cuda.CUDAGraph

    def counting(*a, **k):
        made[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', counting)
    return made


def _same_run(a, b):
    assert a.test_loss == b.test_loss and a.train_loss == b.train_loss, (a.train_loss, b.train_loss, a.test_loss, b.test_loss)
    for (k, p), (_, q) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert torch.equal(p, q), k


@pytest.mark.parametrize('use_graph', [False, True])
def test_the_default_call_is_unchanged(use_graph):
    """train() as it was called before against train(patience=100) -- the bookkeeping of the new keywords, an eager test pass, never
    stopping: the same losses and parameters, and the same generator state afterwards.  The eager pass itself against the parent
    commit's loop is test_eager_pass_is_the_python_sum_of_items."""
    a = _train(_predictor(), 2, use_graph=use_graph)
    rng_a = torch.get_rng_state()
    b = _train(_predictor(), 2, use_graph=use_graph, patience=100)
    assert torch.equal(rng_a, torch.get_rng_state())
    assert len(a.test_loss) == 2 and np.isfinite(a.test_loss + a.train_loss).all()
    _same_run(a, b)
    assert (a.best_epoch, a.stopped_epoch) == (None, None) and b.stopped_epoch is None
    from qtmpnn.validation import best_and_wait
    assert (b.best_epoch, b.best_value) == best_and_wait(b.test_loss, 0.0, 'min')[:2]


@pytest.mark.parametrize('case', ['cheb', 'binary', 'weighted'])
def test_eager_pass_is_the_python_sum_of_items(case):
    """The default test pass adds the batches' losses as float64s on the device and reads the sum once; that is the parent commit's
    Python sum of .item()s to the bit (dynamic mode, the unfused BCE on a binary head), every epoch, on moving weights."""
    cfg = CASES[case]
    nfp, refs = _predictor(**cfg), []
    nfp.initiate_training(0.01, 0.5)
    nfp.writer = _Recorder(lambda: refs.append(_by_hand(nfp, False, False, cfg.get('weights', False))))
    _train(nfp, 2, **cfg)
    print(f'{case}: test_loss {nfp.test_loss} by hand {refs}')
    assert len(refs) == 2 and refs[0] != refs[1] and nfp.test_loss == refs
    assert nfp.writer.scalars['Loss/test'] == refs and 'Monitor/test' not in nfp.writer.scalars


def _dated_loaders():
    """_loaders() with launch dates, one per clip (int64 ns, consecutive days from 1 March 2010), and (1, 366, 64, 64) normals."""
    import datetime
    from helpers import climatology_from_base
    t0 = int(datetime.datetime(2010, 3, 1, 12, tzinfo=datetime.timezone.utc).timestamp()) * 10 ** 9
    clip0, out = 0, []
    for loader in _loaders():
        items = []
        for x, y, _ in loader:
            items.append((x, y, torch.tensor([t0 + 86400 * 10 ** 9 * (clip0 + c) for c in range(x.shape[0])], dtype=torch.int64)))
            clip0 += x.shape[0]
        out.append(TinyLoader(items, (64, 64)))
    clim = climatology_from_base(np.random.default_rng(11).random((64, 64), dtype=np.float32))
    return out[0], out[1], torch.from_numpy(np.concatenate([clim, clim[:, :1]], axis=1)).to(dev())


def _generators():
    """Everything a run draws from, as it stands: torch's CPU and GPU generators, Python's `random`, the attention-dropout counters."""
    import random
    from qtmpnn import ops
    return torch.get_rng_state(), torch.cuda.get_rng_state(dev()), random.getstate(), ops.dropout_state(dev())


def _same_generators(a, b):
    assert torch.equal(a[0], b[0]), "torch's CPU generator"
    assert torch.equal(a[1], b[1]), "torch's GPU generator"
    assert a[2] == b[2], "Python's random"
    assert a[3] == b[3], (a[3], b[3])


def _parent_epochs(nfp, train, test, clim, n_epochs):
    """The parent commit's train() for these arguments (eager, truncated_backprop=0, no weights), written out: per batch train_step
    and .item(), then the test loop -- forward_loss, which hands y to the model, under no_grad and one .item() per batch -- and the
    schedule.  -> (train_loss, test_loss)."""
    from qtmpnn.mesh import check_tile_errors
    nfp.initiate_training(0.01, 0.5)
    train_loss, test_loss = [], []
    for _ in range(n_epochs):
        running, steps = 0.0, 0
        for x, y, date in train:
            x, y = nfp._clip(x), nfp._clip(y)
            concat = nfp.get_climatology_array(clim, date) if clim is not None else None
            running += nfp.train_step(x, y, concat, MASK, None, None, loss_weights=None).item()
            steps += 1
        running_test, steps_test = 0.0, 0
        for x, y, date in test:
            x, y = nfp._clip(x), nfp._clip(y)
            concat = nfp.get_climatology_array(clim, date) if clim is not None else None
            with torch.no_grad():
                running_test += nfp.forward_loss(x, y, concat, MASK, None, None, loss_weights=None).item()
            steps_test += 1
        check_tile_errors(always=True)
        nfp.scheduler.step()
        train_loss.append(running / (steps + 1))
        test_loss.append(running_test / (steps_test + 1))
    return train_loss, test_loss


@pytest.mark.parametrize('case', ['transformer_dropout', 'cheb_dropout_climatology'])
def test_default_call_equals_the_parent_loop_under_dropout(case):
    """Where the runs draw random numbers -- attention dropout and decoder dropout in train() mode, with and without a climatology
    -- train() as it was called before equals the parent commit's loop written out by hand from the same seed: losses, parameters,
    and the state of every generator afterwards.  The test pass no longer hands y to the model; at teacher forcing 0 that changes
    neither a value nor a draw."""
    import random
    from model.mpnnlstm import NextFramePredictorS2S
    conv = 'TransformerConv' if case == 'transformer_dropout' else 'ChebConv'
    train, test, clim = _dated_loaders()
    clim = clim if case.endswith('climatology') else None

    def fresh():
        from qtmpnn import ops
        torch.manual_seed(3)
        random.seed(3)
        ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T, output_timesteps=T, device=dev(),
                                    model_kwargs=dict(hidden_size=8, dropout=0.1, n_layers=1, n_conv_layers=1, convolution_type=conv))
        nfp.model.train()
        return nfp
    a = fresh()
    a.train(train, test, clim, n_epochs=2, lr=0.01, lr_decay=0.5, mask=MASK, truncated_backprop=0)
    gen_a = _generators()
    b = fresh()
    train_loss, test_loss = _parent_epochs(b, train, test, clim, 2)
    gen_b = _generators()
    print(f'{case}: train() {a.train_loss} {a.test_loss}\n{case}: by hand {train_loss} {test_loss}')
    assert np.isfinite(a.train_loss + a.test_loss).all() and a.test_loss[0] != a.test_loss[1]
    assert a.train_loss == train_loss and a.test_loss == test_loss
    for (k, p), (_, q) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert torch.equal(p, q), k
    _same_generators(gen_a, gen_b)
    # the control: the draws matter -- the same loop from the same seed in eval() mode ends somewhere else
    c = fresh()
    c.model.eval()
    assert _parent_epochs(c, train, test, clim, 1)[1][0] != test_loss[0]


@pytest.mark.parametrize('case', list(CASES))
def test_graphed_test_pass_equals_the_eager_static_pass(case, monkeypatch):
    """test_graph=True: every epoch's test loss == the float64 in-order sum of forward_loss(fused=self.binary) under no_grad in
    static mode over the loader / (steps + 1), computed by hand on the epoch's weights.  Epoch 0 is two warm-ups and a replay,
    epoch 1 three replays; two graphs are made (batches of 4 and of 2 clips) and no third.  The eager dynamic-mode pass (the
    default one) is close, and whether it is bit-equal is printed."""
    cfg = CASES[case]
    nfp, refs, dyn = _predictor(**cfg), [], []
    nfp.initiate_training(0.01, 0.5)

    def after_test():
        refs.append(_by_hand(nfp, True, nfp.binary, cfg.get('weights', False)))
        dyn.append(_by_hand(nfp, False, False, cfg.get('weights', False)))
    nfp.writer = _Recorder(after_test)
    made = _count_graphs(monkeypatch)
    _train(nfp, 2, test_graph=True, **cfg)
    print(f'{case}: graphed {nfp.test_loss} static by hand {refs} dynamic by hand {dyn}; graphed == dynamic (default pass): '
          f'{nfp.test_loss == dyn}')
    assert made[0] == SHAPES, 'one capture per batch shape, replayed in the second epoch'
    assert len(refs) == 2 and refs[0] != refs[1] and np.isfinite(refs).all()
    assert nfp.test_loss == refs
    close(np.array(nfp.test_loss), np.array(dyn))
    assert nfp.model.static_shapes is False, 'static mode is left after every test pass'
    assert nfp.best_epoch is None


def test_graphed_test_pass_under_a_graphed_step(monkeypatch):
    """use_graph=True and test_graph=True together: one capture per training shape and per test shape, the losses those of the
    run whose test pass is eager (static mode, which the captured steps leave on), bit for bit."""
    made = _count_graphs(monkeypatch)
    a = _train(_predictor(), 2, use_graph=True)
    assert made[0] == 1
    b = _train(_predictor(), 2, use_graph=True, test_graph=True)
    assert made[0] == 2 + SHAPES
    print(f'eager test pass {a.test_loss}, graphed {b.test_loss}')
    _same_run(a, b)


@pytest.mark.parametrize('test_graph', [False, True])
def test_early_stop_is_deterministic(test_graph):
    """lr = 0 and eval(): the parameters never move, the test loss is constant, every epoch after the first is a tie and
    patience=2 ends the run after exactly 3 of 6 epochs.  (On the parent commit: TypeError, unexpected keyword 'patience'.)"""
    nfp = _predictor(eval_mode=True)
    before = {k: v.clone() for k, v in nfp.model.state_dict().items()}
    _train(nfp, 6, lr=0.0, patience=2, test_graph=test_graph)
    print(f'test_graph={test_graph}: {nfp.test_loss}')
    assert len(nfp.test_loss) == 3 and len(set(nfp.test_loss)) == 1 and len(nfp.loss) == 3
    assert (nfp.stopped_epoch, nfp.best_epoch, nfp.best_value) == (2, 0, nfp.test_loss[0])
    assert all(torch.equal(v, before[k]) for k, v in nfp.model.state_dict().items())
    assert nfp.test_loss[0] == _by_hand(nfp, test_graph, False)


def test_best_weights_are_restored_and_kept(tmp_path):
    """Four epochs at a large learning rate with restore_best and keep_best: whatever the history is, the best epoch is the rule's,
    the file is the checkpoint of that epoch and its parameters are the restored ones."""
    from qtmpnn.validation import best_and_wait
    path = tmp_path / 'best.pt'
    nfp = _train(_predictor(), 4, lr=0.03, restore_best=True, keep_best=path)
    plain = _train(_predictor(), 4, lr=0.03)
    print(f'test_loss {nfp.test_loss}: best epoch {nfp.best_epoch}')
    assert nfp.test_loss == plain.test_loss and nfp.train_loss == plain.train_loss, 'the keywords do not touch the run itself'
    best, value, _ = best_and_wait(nfp.test_loss, 0.0, 'min')
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (best, value, None) and len(nfp.test_loss) == 4
    other = _predictor(seed=99)
    other.load_checkpoint(path)
    assert other.test_loss == nfp.test_loss[:best + 1] and other.train_loss == nfp.train_loss[:best + 1]
    assert other.scheduler.last_epoch == best + 1
    for (k, p), (_, q) in zip(nfp.model.state_dict().items(), other.model.state_dict().items()):
        assert torch.equal(p, q), k
    last = all(torch.equal(p, q) for p, q in zip(nfp.model.state_dict().values(), plain.model.state_dict().values()))
    assert last == (best == 3), 'the last epoch\'s parameters exactly when the last epoch is the best one'
    if nfp.flat is not None:
        assert nfp.flat.intact(nfp.model) and not bool(nfp.flat.buffer[nfp.flat.n:].any())
    # the restored predictor trains on: the parameters were written in place
    _train(nfp, 1, lr=0.03)
    assert len(nfp.test_loss) == 5 and np.isfinite(nfp.test_loss[-1])


def test_patience_counts_across_a_checkpoint(tmp_path):
    """lr = 0: two epochs, a checkpoint, a fresh predictor that loads it and trains with patience=3 stops after 2 more epochs --
    the two epochs of the file count."""
    a = _train(_predictor(eval_mode=True), 2, lr=0.0)
    a.save_checkpoint(tmp_path / 'a.pt')
    b = _predictor(eval_mode=True, seed=99)
    b.load_checkpoint(tmp_path / 'a.pt')
    _train(b, 6, lr=0.0, patience=3)
    print(f'{a.test_loss} -> {b.test_loss}')
    assert len(b.test_loss) == 4 and len(set(b.test_loss)) == 1 and (b.stopped_epoch, b.best_epoch) == (3, 0)


@pytest.mark.parametrize('test_graph', [False, True])
def test_monitor_selects_on_verification_products(test_graph, monkeypatch):
    """Monitor(('score', 'extent'), value), lr = 0: every epoch's monitored value == value(verify(...)) called by hand on the same
    weights in the same mode; test_loss is still the loss; eagerly the model's forward runs once per test batch, graphed there is
    one capture per shape."""
    from qtmpnn.validation import Monitor
    products = {'score': None, 'extent': {'regions': None}}
    value = lambda v: float(v.extent.by_lead('model')['iiee'].mean() + v.score.by_lead('model')['rmse'].mean())
    nfp = _predictor(eval_mode=True)
    calls, forward = [0], nfp.model.forward

    def counting(*a, **k):
        calls[0] += 1
        return forward(*a, **k)
    monkeypatch.setattr(nfp.model, 'forward', counting)
    made = _count_graphs(monkeypatch)
    nfp.initiate_training(0.0, 0.5)
    nfp.writer = _Recorder()
    _train(nfp, 2, lr=0.0, monitor=Monitor(products, value), test_graph=test_graph)
    if test_graph:
        assert made[0] == SHAPES and calls[0] == 2 * N_TRAIN + 2 * SHAPES        # (a warm-up and a capture per shape, then replays)
    else:
        assert made[0] == 0 and calls[0] == 2 * (N_TRAIN + N_TEST), 'one forward per test batch: the products share the loss\'s rollout'
    by_hand = value(nfp.verify(_loaders()[1], mask=MASK, products=products, use_graph=test_graph))
    print(f'test_graph={test_graph}: monitor {nfp.monitor_history} by hand {by_hand}; loss {nfp.test_loss}')
    assert nfp.monitor_history == [by_hand, by_hand] and np.isfinite(by_hand) and by_hand > 0
    assert nfp.writer.scalars['Monitor/test'] == nfp.monitor_history
    assert nfp.test_loss == [_by_hand(nfp, test_graph, False)] * 2 and nfp.writer.scalars['Loss/test'] == nfp.test_loss
    assert (nfp.best_epoch, nfp.best_value, nfp.stopped_epoch) == (0, by_hand, None)
