"""set_recompute('step') on the GPU: every path that builds an autograd graph through the rollout gives the plain path's bits --
losses, gradients, parameters, optimiser moments, the attention-dropout masks of later steps -- and keeps less memory.  Each case
runs twice from the same seeds (torch's generator, Python's `random`, the attention-dropout counters), once plain and once under
'step'; equal means torch.equal."""
import random

import numpy as np
import pytest
import torch

from helpers import TinyLoader, dev

pytestmark = pytest.mark.gpu

T, H = 3, 8
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 52:] = True
MASK[40:, :9] = True
HIR = np.zeros((64, 64), dtype=bool)
HIR[10:30, 10:40] = True


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)           # (initiate_training()'s SummaryWriter writes under the working directory)


_DATA = {}


def _clips(shape=(64, 64), t_out=T, n=4, ice=False):
    key = (shape, t_out, n, ice)
    if key not in _DATA:
        from qtmpnn import synthetic
        if ice:
            clips = [synthetic.make_ice_like(40 + i, shape=shape, channels=1, n_frames=T + t_out) for i in range(n)]
            x, y = np.stack([c[0][:T] for c in clips]), np.stack([c[0][T:, ..., :1] for c in clips])
            _DATA[key] = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()), clips[0][1]
        else:
            x, y = synthetic.make_batch(7, 0, n, T, t_out, n_digits=1, pixel_noise=0.02, canvas=shape[::-1])
            _DATA[key] = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()), None
    return _DATA[key]


def _seed():
    from qtmpnn import ops
    torch.manual_seed(5)
    random.seed(5)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())


def _fresh(mode, conv='ChebConv', binary=False, capturable=False, static=False, initiate=True, t_out=T, thresh=0.1, tf=None, **kw):
    from model.mpnnlstm import NextFramePredictorS2S
    _seed()
    mk = dict(hidden_size=H, dropout=0.0, n_layers=1, n_conv_layers=2, convolution_type=conv)
    mk.update(kw)
    if tf is not None:
        mk['transform_func'] = tf
    nfp = NextFramePredictorS2S(thresh=thresh, input_features=1, input_timesteps=T, output_timesteps=t_out, device=dev(),
                                binary=binary, transform_func=tf, model_kwargs=mk)
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    if initiate:
        nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=capturable)
    nfp.model.static_shapes = static
    nfp.model.train()
    nfp.set_recompute(mode)
    assert nfp.recompute == mode
    _seed()
    return nfp


def _state(nfp):
    from qtmpnn.optim import adam_state
    st = adam_state(nfp.optimizer, nfp.model)
    out = {'p ' + k: p.detach().cpu().clone() for k, p in nfp.model.named_parameters()}
    out.update({'m ' + k: v for k, v in st['exp_avg'].items()})
    out.update({'v ' + k: v for k, v in st['exp_avg_sq'].items()})
    return out


def _grads(nfp):
    return {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in nfp.model.named_parameters()}


def _same(a, b, what=''):
    """Nested lists / dicts of tensors and numbers: the same bits."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f'{what} {k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f'{what}[{i}]')
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), what
    else:
        assert a == b or (a is None and b is None), (what, a, b)


def _both(body, **kw):
    """body(predictor) under None and under 'step' from the same seeds: the two results must be the same bits, and not empty."""
    plain, step = body(_fresh(None, **kw)), body(_fresh('step', **kw))
    _same(plain, step)
    return plain


def _one_step(x, y, concat=None, mask=MASK, steps=1, **kw):
    def body(nfp):
        losses = [nfp.train_step(x, y, concat, mask, **kw).detach().cpu() for _ in range(steps)]
        assert all(np.isfinite(float(l)) for l in losses)
        g = _grads(nfp)
        assert any(v is not None and bool(v.any()) for v in g.values())
        return losses, g, _state(nfp)
    return body


CASES = {
    'cheb': dict(conv='ChebConv'),
    'cheb_2_layers': dict(conv='ChebConv', n_layers=2, n_conv_layers=2),
    'gcn': dict(conv='GCNConv'),
    'transformer_dropout': dict(conv='TransformerConv'),            # (the attention convolutions' own dropout = 0.1, train mode)
    'mh_transformer_dropout': dict(conv='MHTransformerConv'),
    'cheb_decoder_dropout': dict(conv='ChebConv', dropout=0.2),
    'transformer_decoder_dropout': dict(conv='TransformerConv', dropout=0.2),
}


@pytest.mark.parametrize('case', list(CASES))
def test_train_step_same_bits(case):
    x, y, _ = _clips()
    _both(_one_step(x[:2], y[:2]), **CASES[case])


def test_three_steps_with_attention_dropout_same_bits():
    """A dropout counter left at another value after a replay would change the second step's masks."""
    x, y, _ = _clips()
    losses, _, _ = _both(_one_step(x[:2], y[:2], steps=3), conv='TransformerConv')
    assert len({float(l) for l in losses}) == 3


def test_mask_hir_and_concat_layers_same_bits():
    x, y, _ = _clips()
    concat = torch.linspace(0, 1, 2 * T * 64 * 64, device=dev()).view(2, T, 64, 64, 1)
    _both(_one_step(x[:2], y[:2], concat, MASK, high_interest_region=HIR))


def test_48x64_frame_same_bits():
    x, y, _ = _clips((48, 64))
    _both(_one_step(x[:2], y[:2], None, MASK[:48]))


def test_96x128_masked_tile_resident_same_bits():
    from qtmpnn.mesh import tile_error_word
    x, y, mask = _clips((96, 128), ice=True, n=2)
    tf = lambda a: abs(abs(a - 0.5) - 0.5)
    _both(_one_step(x, y, None, mask), thresh=0.15, tf=tf)
    assert tile_error_word() == 0


def test_teacher_forcing_through_forward_same_bits():
    from model.mpnnlstm import masked_mse
    x, y, _ = _clips()

    def body(nfp):
        outs, meshes = nfp.model(x[:2], y[:2], None, teacher_forcing_ratio=1, mask=MASK)
        loss = masked_mse(outs, meshes, y[:2], MASK)
        nfp.zero_grad()
        loss.backward()
        return loss.detach(), [o.detach() for o in outs], _grads(nfp)
    _both(body)


def test_binary_fused_and_weighted_loss_same_bits():
    x, y, _ = _clips()
    yb = (y > 0.3).float()
    _both(_one_step(x[:2], yb[:2], fused=True), binary=True)
    w = np.linspace(0.5, 2.0, 64 * 64, dtype=np.float32).reshape(64, 64)
    _both(_one_step(x[:2], y[:2], loss_weights=w, lead_weights=[1.0, 2.0, 0.5]))


def test_truncated_backward_same_bits():
    x, y, _ = _clips()

    def body(nfp):
        losses = nfp.truncated_backward(x[:2], y[:2], None, MASK, truncated_backprop=2)
        assert len(losses) == 2
        return [l.cpu() for l in losses], _grads(nfp)
    _both(body)


def test_accumulated_step_same_bits():
    x, y, _ = _clips()

    def body(nfp):
        loss = nfp.accumulated_step([(x[0:2], y[0:2]), (x[2:4], y[2:4])], MASK)
        return loss.detach(), _grads(nfp), _state(nfp)
    _both(body)


@pytest.mark.parametrize('accumulate', [1, 2])
def test_captured_step_same_bits_and_keeps_its_mode(accumulate):
    x, y, _ = _clips()
    groups = [[(x[0:2], y[0:2]), (x[2:4], y[2:4])], [(x[1:3], y[1:3]), (x[0:2], y[0:2])], [(x[2:4], y[2:4]), (x[1:3], y[1:3])]]

    def body(nfp):
        step = nfp.make_graphed_step(x[0:2], y[0:2], None, MASK, warmup=1, accumulate=accumulate)
        nfp.set_recompute(None)             # the captured step keeps the mode it was captured under
        if accumulate == 1:
            losses = [step(*g[0], None).detach().cpu() for g in groups]
        else:
            losses = [step(g).detach().cpu() for g in groups]
        return nfp.last_warmup_loss.detach().cpu(), losses, _state(nfp)
    _both(body, capturable=True, static=True)


@pytest.mark.parametrize('use_graph', [False, True])
def test_train_same_bits(use_graph):
    x, y, _ = _clips()
    items = [(x[i:i + 1].cpu(), y[i:i + 1].cpu(), torch.zeros(1)) for i in range(3)]
    train, test = TinyLoader(items, (64, 64)), TinyLoader(items[:1], (64, 64))

    def body(nfp):
        nfp.train(train, test, n_epochs=2, lr=1e-3, mask=MASK, truncated_backprop=0, use_graph=use_graph)
        assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all()
        return list(nfp.train_loss), list(nfp.test_loss), _state(nfp)
    _both(body, initiate=False)


def test_mode_is_no_training_state(tmp_path):
    x, y, _ = _clips()
    a = _fresh('step')
    a.train_step(x[:2], y[:2], None, MASK)
    a.save_checkpoint(tmp_path / 'a.ckpt')
    b = _fresh(None)
    b.load_checkpoint(tmp_path / 'a.ckpt')
    assert b.recompute is None and a.recompute == 'step'
    la, lb = a.train_step(x[2:4], y[2:4], None, MASK), b.train_step(x[2:4], y[2:4], None, MASK)
    assert torch.equal(la, lb)
    _same(_state(a), _state(b))


def _bench_model(mode, **kw):
    return _fresh(mode, hidden_size=16, n_layers=2, dropout=0.1, t_out=8, **kw)         # (bench.py's model: dropout 0.1)


def test_memory_eager():
    """The benchmark's 64x64 model (hidden 16) at 4 clips, 3 steps in and 8 out: fewer bytes are handed to autograd's
    saved-tensor hooks during the forward, and forward + backward peak lower.  Both follow from the construction; the ratios are
    printed, no target is set for them."""
    x, y, _ = _clips(t_out=8)
    saved, peak, loss = {}, {}, {}
    for mode in (None, 'step'):
        nfp = _bench_model(mode)
        count = [0]

        def pack(t):
            count[0] += t.numel() * t.element_size()
            return t
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        nfp.zero_grad()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            l = nfp.forward_loss(x, y, None, MASK)
        l.backward()
        torch.cuda.synchronize()
        saved[mode], peak[mode], loss[mode] = count[0], torch.cuda.max_memory_allocated(), l.detach()
        del nfp, l
    print(f"saved bytes: plain {saved[None]} step {saved['step']} ratio {saved['step'] / saved[None]:.3f}; "
          f"peak bytes: plain {peak[None]} step {peak['step']} ratio {peak['step'] / peak[None]:.3f}")
    assert torch.equal(loss[None], loss['step'])
    assert saved['step'] < saved[None]
    assert peak['step'] < peak[None]


def test_memory_captured():
    from qtmpnn import recompute
    x, y, _ = _clips(t_out=8)
    saved, peak, loss = {}, {}, {}
    for mode in (None, 'step'):
        nfp = _bench_model(mode, capturable=True, static=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        count = [0]

        def pack(t):            # (the first pass's: what a replay saves lives only until that step's backward ends)
            if not recompute.replaying():
                count[0] += t.numel() * t.element_size()
            return t
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):           # (the warm-up step and the capture)
            step = nfp.make_graphed_step(x, y, None, MASK, warmup=1)
        saved[mode] = count[0]
        loss[mode] = step(x, y, None).detach().cpu()
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated()
        del nfp, step
    print(f"captured: saved bytes: plain {saved[None]} step {saved['step']} ratio {saved['step'] / saved[None]:.3f}; "
          f"peak bytes: plain {peak[None]} step {peak['step']} ratio {peak['step'] / peak[None]:.3f}")
    assert torch.equal(loss[None], loss['step'])
    assert saved['step'] < saved[None]
    assert peak['step'] < peak[None]


def test_no_op_without_autograd():
    x, y, _ = _clips()
    items = [(x[i:i + 1].cpu(), y[i:i + 1].cpu(), torch.zeros(1)) for i in range(2)]
    loader = TinyLoader(items, (64, 64))

    def body(nfp):
        nfp.model.eval()
        pred = nfp.predict(loader, mask=MASK)
        score = nfp.verify(loader, mask=MASK, products=('score',))['score']
        return torch.as_tensor(np.asarray(pred)), torch.as_tensor(np.asarray(score.sums))
    pred, score = _both(body, initiate=False)
    assert pred.numel() and score.numel() and float(score[..., 0].min()) > 0
