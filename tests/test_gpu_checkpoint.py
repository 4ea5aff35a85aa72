"""save_checkpoint() / load_checkpoint() on the GPU: a run that is interrupted, saved and resumed in a fresh predictor ends in the
parameters and losses of the run that was not, bit for bit -- FlatAdam eager and as a captured graph, attention dropout, the binary
head -- while the weights alone (save() / load()) do not; a flat checkpoint loads into torch's Adam; a captured step survives a
load; an eager checkpoint resumes as a captured graph."""
import numpy as np
import pytest
import torch

from helpers import TinyLoader, dev

pytestmark = pytest.mark.gpu

LR, DECAY, SEED = 0.01, 0.5, 11
# The largest elementwise difference, after ONE step from identical mid-training state (6 steps in) without any checkpoint,
# between the flat path (FlatAdam: qt_flat_adam) and the same model on torch's fused Adam with per-tensor packing: the figure of
# test_flat_checkpoint_loads_into_torch_adam's control, recorded on an MI355X in profiles/checkpoint.txt.  The two Adam
# implementations round differently; four times the figure is allowed.
FLAT_VS_TORCH_ONE_STEP = 2.0 ** -23        # 1.1920928955078125e-07: one ulp of a weight in [1, 2)
CONFIGS = {'cheb_eager': dict(conv='ChebConv', use_graph=False, binary=False),
           'cheb_graph': dict(conv='ChebConv', use_graph=True, binary=False),
           'transformer_eager': dict(conv='TransformerConv', use_graph=False, binary=False),      # its default attention dropout 0.1
           'binary_graph': dict(conv='ChebConv', use_graph=True, binary=True)}


def _loaders():
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(5, 0, 6, 3, 3, n_digits=1, pixel_noise=0.0)
    items = [(torch.from_numpy(x[i:i + 2]), torch.from_numpy(y[i:i + 2]), torch.zeros(1)) for i in (0, 2, 4)]
    return TinyLoader(items, (64, 64)), TinyLoader(items[:1], (64, 64)), items


MASK = np.zeros((64, 64), dtype=bool)


def _seed(seed):
    """Everything a run's dropout masks come from: torch's generators (CPU and GPU) and the attention kernels' counters."""
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())


def _predictor(conv='ChebConv', binary=False, **_):
    """Built in train() mode (nn.Module's default, what ice_exp.py trains in): decoder dropout 0.1 and the attention dropout are on."""
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=3, device=dev(), binary=binary,
                                model_kwargs=dict(hidden_size=8, dropout=0.1, n_layers=1, n_conv_layers=1, convolution_type=conv))
    nfp.model.train()
    return nfp


def _train(nfp, n_epochs, use_graph=False, **_):
    train, test, _items = _loaders()
    nfp.train(train, test, n_epochs=n_epochs, lr=LR, lr_decay=DECAY, mask=MASK, truncated_backprop=0, use_graph=use_graph)


def _params(nfp):
    return {k: p.detach().clone() for k, p in nfp.model.named_parameters()}


_RUNS = {}


def _runs(name, tmp_path_factory):
    """Per configuration, once: run A (4 epochs, never interrupted) and run B (2 epochs from the same seed, then a checkpoint and
    the weights file, then deleted) -> A's parameters and histories, the checkpoint's path, the weights' directory."""
    if name not in _RUNS:
        cfg, d = CONFIGS[name], tmp_path_factory.mktemp(name)
        _seed(SEED)
        a = _predictor(**cfg)
        _train(a, 4, **cfg)
        _seed(SEED)
        b = _predictor(**cfg)
        _train(b, 2, **cfg)
        b.save_checkpoint(d / 'b.ckpt')
        b.save(str(d))
        assert b.train_loss == a.train_loss[:2] and b.test_loss == a.test_loss[:2], 'two runs from one seed differ before any checkpoint'
        _RUNS[name] = dict(params=_params(a), train_loss=list(a.train_loss), test_loss=list(a.test_loss), loss=a.loss.copy(),
                           flat=a.flat is not None, ckpt=d / 'b.ckpt', dir=str(d))
        del a, b
    return _RUNS[name]


@pytest.mark.parametrize('name', list(CONFIGS))
def test_interrupted_run_equals_uninterrupted_run(name, tmp_path_factory, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg, ref = CONFIGS[name], _runs(name, tmp_path_factory)
    _seed(97)                               # another seed: whatever C's masks need comes from the file
    c = _predictor(**cfg)
    c.load_checkpoint(ref['ckpt'])
    assert (c.flat is not None) == ref['flat'] and bool(c.optimizer.param_groups[0]['capturable']) == cfg['use_graph']
    assert c.scheduler.last_epoch == 2 and c.train_loss == ref['train_loss'][:2]
    if c.flat is not None:
        assert not bool(c.flat.buffer[c.flat.n:].any()), 'the pad tail of the flat buffer'
    _train(c, 2, **cfg)
    print(f'{name}: A train {ref["train_loss"]} test {ref["test_loss"]}\n{name}: C train {c.train_loss} test {c.test_loss}')
    assert c.train_loss == ref['train_loss'] and c.test_loss == ref['test_loss']
    assert np.isfinite(c.train_loss + c.test_loss).all()
    for k, p in c.model.named_parameters():
        assert torch.equal(p, ref['params'][k]), k
    # the frame train() leaves covers the restored epochs and the new ones
    assert len(c.loss) == 4 and c.loss.equals(ref['loss'])
    assert float(c.optimizer.param_groups[0]['lr']) == pytest.approx(LR * DECAY, rel=1e-6)        # (the schedule moved at epoch 3)


def test_weights_alone_do_not_resume_the_run(tmp_path_factory, tmp_path, monkeypatch):
    """The negative control: the same procedure with save() / load() in place of the checkpoint ends somewhere else."""
    monkeypatch.chdir(tmp_path)
    cfg, ref = CONFIGS['cheb_eager'], _runs('cheb_eager', tmp_path_factory)
    _seed(97)
    c = _predictor(**cfg)
    c.load(ref['dir'])
    _train(c, 2, **cfg)
    assert len(c.train_loss) == 2 and np.isfinite(c.train_loss + c.test_loss).all()
    assert not all(torch.equal(p, ref['params'][k]) for k, p in c.model.named_parameters())
    assert c.train_loss != ref['train_loss'][2:]


def _one_step(nfp, item):
    _seed(5)                                # (the same dropout masks on both sides)
    return float(nfp.train_step(item[0].to(dev()), item[1].to(dev()), None, MASK))


def _max_diff(a, b):
    return max(float((p.detach() - q.detach()).abs().max()) for (_, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()))


def test_flat_checkpoint_loads_into_torch_adam(tmp_path, monkeypatch):
    """Cross layout: the checkpoint of the flat ChebConv predictor (FlatAdam, one vector) loads into the same model with the flat
    path off (torch's fused Adam, one state per tensor), and one further step on each side agrees within four times what the two
    paths differ by on one step from identical state without a checkpoint (FLAT_VS_TORCH_ONE_STEP).  The control hands the flat
    predictor's state to the torch one tensor by tensor, through FlatParams' own offsets."""
    from model.seq2seq import Decoder, Encoder
    monkeypatch.chdir(tmp_path)
    item = _loaders()[2][1]
    _seed(SEED)
    flat0 = _predictor()
    _train(flat0, 2)
    assert flat0.flat is not None
    flat0.save_checkpoint(tmp_path / 'flat.ckpt')
    flat1 = _predictor()
    flat1.load_checkpoint(tmp_path / 'flat.ckpt')
    with monkeypatch.context() as mp:       # the same model where the layers are not plannable: per-tensor packing, torch's Adam
        mp.setattr(Encoder, 'plannable', property(lambda self: False))
        mp.setattr(Decoder, 'plannable', property(lambda self: False))
        _seed(3)
        torch0, torch1 = _predictor(), _predictor()
        torch0.initiate_training(LR, DECAY)
        assert torch0.flat is None and type(torch0.optimizer) is torch.optim.Adam
        fp, st = flat0.flat, flat0.optimizer.state[flat0.flat.param]
        with torch.no_grad():               # the control: no checkpoint, the state copied by hand
            for p, q, o, n in zip(torch0.model.parameters(), fp.params, fp.offs, fp.sizes):
                p.copy_(q)
                torch0.optimizer.state[p] = {'step': st['step'].float().reshape(()).clone(),
                                             'exp_avg': st['exp_avg'][o:o + n].view_as(p).clone(),
                                             'exp_avg_sq': st['exp_avg_sq'][o:o + n].view_as(p).clone()}
        torch0.optimizer.param_groups[0]['lr'] = flat0.optimizer.param_groups[0]['lr']
        torch1.load_checkpoint(tmp_path / 'flat.ckpt')
        assert torch1.flat is None and type(torch1.optimizer) is torch.optim.Adam
        assert _max_diff(torch0, torch1) == 0 and _max_diff(flat0, torch1) == 0
        for p, q in zip(torch0.model.parameters(), torch1.model.parameters()):
            for k in ('step', 'exp_avg', 'exp_avg_sq'):
                assert torch.equal(torch0.optimizer.state[p][k], torch1.optimizer.state[q][k]), k
        losses = [_one_step(nfp, item) for nfp in (torch0, torch1)]
    losses += [_one_step(nfp, item) for nfp in (flat0, flat1)]
    control, loaded = _max_diff(flat0, torch0), _max_diff(flat1, torch1)
    print(f'flat vs torch, one step from identical state, no checkpoint: max |diff| = {control:.3e}; through the checkpoint: '
          f'{loaded:.3e}; losses torch {losses[0]!r} {losses[1]!r} flat {losses[2]!r} {losses[3]!r}; lr {float(flat0.optimizer.param_groups[0]["lr"])}')
    assert np.isfinite(losses).all()
    assert _max_diff(flat0, flat1) == 0, 'flat -> flat through the checkpoint is exact'
    assert loaded <= 4 * FLAT_VS_TORCH_ONE_STEP, (loaded, control, FLAT_VS_TORCH_ONE_STEP)
    # the other way round: what torch's Adam wrote loads into the flat optimiser
    torch1.save_checkpoint(tmp_path / 'torch.ckpt')
    flat1.load_checkpoint(tmp_path / 'torch.ckpt')
    assert _max_diff(flat1, torch1) == 0 and int(flat1.optimizer.state[flat1.flat.param]['step']) == 7
    assert not bool(flat1.flat.buffer[flat1.flat.n:].any())
    for q, o, n in zip(torch1.model.parameters(), flat1.flat.offs, flat1.flat.sizes):
        assert torch.equal(flat1.optimizer.state[flat1.flat.param]['exp_avg_sq'][o:o + n], torch1.optimizer.state[q]['exp_avg_sq'].reshape(-1))


def test_captured_step_survives_a_load(tmp_path_factory, tmp_path, monkeypatch):
    """A make_graphed_step object captured BEFORE load_checkpoint() replays from the loaded state: the load writes into the
    buffers the graph holds pointers to.  Its replays equal eager static-mode train_steps of a second predictor that loaded the
    same file, bit for bit."""
    monkeypatch.chdir(tmp_path)
    ref, items = _runs('cheb_graph', tmp_path_factory), _loaders()[2]
    t = lambda a: a.to(dev())
    _seed(41)
    graphed = _predictor()
    graphed.initiate_training(LR, DECAY, capturable=True)
    step = graphed.make_graphed_step(t(items[2][0]), t(items[2][1]), None, MASK, warmup=1)
    st = graphed.optimizer.state[graphed.flat.param]
    held = (graphed.flat.buffer, graphed.flat.param, st['exp_avg'], st['exp_avg_sq'], st['step'], graphed.optimizer.param_groups[0]['lr'])
    ptrs = [h.data_ptr() for h in held]
    eager = _predictor()
    eager.model.static_shapes = True
    graphed.load_checkpoint(ref['ckpt'])
    st = graphed.optimizer.state[graphed.flat.param]
    now = (graphed.flat.buffer, graphed.flat.param, st['exp_avg'], st['exp_avg_sq'], st['step'], graphed.optimizer.param_groups[0]['lr'])
    assert all(a is b for a, b in zip(held, now)) and ptrs == [h.data_ptr() for h in now]
    assert int(st['step']) == 6 and not bool(graphed.flat.buffer[graphed.flat.n:].any())
    lg = [float(step(t(x), t(y))) for x, y, _ in items[:2]]
    eager.load_checkpoint(ref['ckpt'])      # (puts the generators back where the file has them, as the first load did)
    le = [float(eager.train_step(t(x), t(y), None, MASK)) for x, y, _ in items[:2]]
    print(f'replayed after the load {lg}, eager from the same file {le}')
    assert np.isfinite(lg).all() and lg == le
    for (k, p), (_, q) in zip(graphed.model.named_parameters(), eager.model.named_parameters()):
        assert torch.equal(p, q), k
    assert int(st['step']) == 8


class _Recorder:
    """A SummaryWriter stand-in that keeps what train() reports."""

    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append(value)

    def flush(self):
        pass


def test_eager_checkpoint_resumes_as_a_captured_graph(tmp_path_factory, tmp_path, monkeypatch):
    """load_checkpoint(capturable=True) of a file an eager run wrote, then train(use_graph=True): finite losses, and the steps'
    losses -- the eager one the capture starts with and the first replayed one -- equal those of the eager continuation (static
    mode, as a captured step runs)."""
    monkeypatch.chdir(tmp_path)
    cfg, ref, items = CONFIGS['cheb_eager'], _runs('cheb_eager', tmp_path_factory), _loaders()[2]
    _seed(43)
    g = _predictor(**cfg)
    g.load_checkpoint(ref['ckpt'], capturable=True)
    group = g.optimizer.param_groups[0]
    assert group['capturable'] is True and torch.is_tensor(group['lr']) and group['lr'].is_cuda
    assert float(group['lr']) == np.float32(LR) and int(g.optimizer.state[g.flat.param]['step']) == 6
    g.writer = _Recorder()
    _train(g, 1, use_graph=True)
    steps = g.writer.scalars['Loss/train']
    assert len(steps) == 3 and np.isfinite(steps).all()
    assert len(g.train_loss) == 3 and np.isfinite(g.train_loss + g.test_loss).all() and len(g.loss) == 3
    assert float(group['lr']) == np.float32(LR) * np.float32(DECAY)          # the schedule moved at epoch 3, in the device tensor
    e = _predictor(**cfg)
    e.load_checkpoint(ref['ckpt'])
    assert e.optimizer.param_groups[0]['capturable'] is False
    e.model.static_shapes = True
    le = [float(e.train_step(x.to(dev()), y.to(dev()), None, MASK)) for x, y, _ in items]
    print(f'resumed as a graph {steps}, eager continuation {le}')
    assert steps[1] == le[1], 'the first replayed step'
    assert steps == le
    # and back: the graphed run's checkpoint resumes eagerly
    g.save_checkpoint(tmp_path / 'g.ckpt')
    back = _predictor(**cfg)
    back.load_checkpoint(tmp_path / 'g.ckpt', capturable=False)
    assert back.optimizer.param_groups[0]['capturable'] is False and isinstance(back.optimizer.param_groups[0]['lr'], float)
    _train(back, 1)
    assert len(back.train_loss) == 4 and np.isfinite(back.train_loss + back.test_loss).all()
