"""GPU checks of MHTransformerConv: the fused multi-head kernel against the unfused composition, the convolution, a cell and a
rollout against the fixtures generated from the reference (tests/golden/make_golden_mh.py), batching, graph capture and the
trainer."""
import numpy as np
import pytest
import torch

from helpers import RTOL, close, dev, dist_from_05, golden, grad_close, load_state

pytestmark = pytest.mark.gpu


def _mesh_33():
    from qtmpnn import synthetic
    from qtmpnn.mesh import build_mesh
    c = synthetic.make_clip(33, canvas=(64, 64), n_digits=1, n_frames=1, pixel_noise=0.0)
    return build_mesh(src=torch.from_numpy(c[..., 0]).to(dev()), thresh=0.1)


def _check_mesh(mesh, g):
    assert np.array_equal(mesh.labels[0].cpu().numpy(), g['labels'])
    assert np.array_equal(mesh.edge_index(True).cpu().numpy(), g['edges'])
    close(mesh.edge_attrs(True), g['attrs'], atol=2e-5)


@pytest.mark.parametrize('C,c_real', [(4, 1), (8, 8), (16, 16), (32, 32)])
@pytest.mark.parametrize('keep', [1.0, 0.5])
def test_fused_equals_unfused_composition(C, c_real, keep):
    """qt_mhattn_fwd / qt_mhattn_bwd_merge against qt_attn_fwd with G = 3 heads + a GEMM for the head merge (and their autograd
    backward): same values at RTOL, forward and every gradient; with dropout (keep 0.5) under one seed both draw the same mask."""
    from qtmpnn import ops, synthetic
    from qtmpnn.mesh import build_mesh
    c = synthetic.make_clip(9, canvas=(64, 64), n_digits=2, n_frames=1, pixel_noise=0.0)
    mesh = build_mesh(src=torch.from_numpy(np.stack([c[0, ..., 0], c[0, ::-1, :, 0]])).to(dev()), thresh=0.1)
    N, H = mesh.N, 3
    g = torch.Generator(device=dev()).manual_seed(C + int(keep * 10))
    live = torch.zeros(C, device=dev())
    live[:c_real] = 1.0
    proj = (torch.randn(N, H, 4, C, device=dev(), generator=g) * live).view(N, H * 4 * C)
    We = torch.randn(H, C, 2, device=dev(), generator=g) * live.view(1, C, 1)
    Wt = (torch.randn(H, C, C, device=dev(), generator=g) * 0.3 * live.view(1, C, 1) * live.view(1, 1, C)).view(H * C, C)
    bl = torch.randn(C, device=dev(), generator=g) * live
    gy = torch.randn(N, C, device=dev(), generator=g) * live
    ins = [t.clone().requires_grad_(True) for t in (proj, We, Wt, bl)]
    ref = [t.clone().requires_grad_(True) for t in (proj, We, Wt, bl)]
    seed = 12345
    y = ops._MHAttention.apply(*ins, mesh, c_real, keep, seed, None, None, H)
    cat = ops._Attention.apply(ref[0], ref[1], mesh, c_real, keep, seed, None, H, 0)
    yr = cat @ ref[2] + ref[3]
    close(y, yr, rtol=RTOL, atol=1e-5, msg='y')
    assert not y[:, c_real:].any()
    gf = torch.autograd.grad(y, ins, gy)
    gu = torch.autograd.grad(yr, ref, gy)
    for a, b, name in zip(gf, gu, ('proj', 'We', 'Wt', 'blin')):
        grad_close(a, b, msg=name)
    if keep < 1.0:              # a mask that differed would move the outputs by O(1), far beyond RTOL; and it is a real mask
        y1 = ops._MHAttention.apply(proj, We, Wt, bl, mesh, c_real, 1.0, seed, None, None, H)
        assert (y1 - y.detach()).abs().max() > 0.1


def _conv(cin, cout):
    from model.model import CONVOLUTION_KWARGS, MHTransformerConv
    return MHTransformerConv(cin, cout, **CONVOLUTION_KWARGS['MHTransformerConv'])


def test_mh_conv_golden():
    """MHTransformerConv(6, 8) and (8, 1) against the reference's module on the restated PyG convolution: output, input and
    parameter gradients."""
    g = golden('mh_conv.npz')
    mesh = _mesh_33()
    _check_mesh(mesh, g)
    for name, cin, cout in (('a', 6, 8), ('b', 8, 1)):
        conv = _conv(cin, cout)
        load_state(conv, g, f'{name}/w/')
        conv.to(dev()).eval()
        x = torch.from_numpy(g[f'{name}/x']).to(dev()).requires_grad_(True)
        y = conv(x, mesh)
        close(y, g[f'{name}/y'], msg=f'{name} y')
        grads = torch.autograd.grad(y, [x] + list(conv.parameters()), torch.from_numpy(g[f'{name}/gy']).to(dev()))
        grad_close(grads[0], g[f'{name}/gx'], msg=f'{name} gx')
        wscale = float(np.abs(g[f'{name}/g/lin_key.weight']).max())
        for got, (k, _) in zip(grads[1:], conv.named_parameters()):
            if k == 'lin_key.bias':       # exactly zero in exact arithmetic (softmax shift invariance): rounding noise on both sides
                assert float(got.abs().max()) <= 1e-4 * wscale and float(np.abs(g[f'{name}/g/{k}']).max()) <= 1e-4 * wscale
                continue
            grad_close(got, g[f'{name}/g/{k}'], msg=f'{name} {k}')


def test_mh_gconvlstm_cell_golden():
    from model.model import GConvLSTM
    g = golden('mh_cell.npz')
    mesh = _mesh_33()
    _check_mesh(mesh, g)
    cell = GConvLSTM(4, 8, 2, 'MHTransformerConv')
    load_state(cell, g, 'w/')
    cell.to(dev()).eval()
    X, H, C = (torch.from_numpy(g[k]).to(dev()).requires_grad_(True) for k in 'XHC')
    Oo, Hn, Cn = cell(X, mesh, None, H, C)
    for got, name in ((Oo, 'O'), (Hn, 'Hn'), (Cn, 'Cn')):
        close(got, g[name], msg=name)
    grads = torch.autograd.grad([Oo, Hn, Cn], [X, H, C] + list(cell.parameters()),
                                [torch.from_numpy(g[k]).to(dev()) for k in ('gO', 'gH', 'gC')])
    for got, name in zip(grads[:3], ('gX', 'gHin', 'gCin')):
        grad_close(got, g[name], msg=name)
    for got, (k, _) in zip(grads[3:], cell.named_parameters()):
        grad_close(got, g['g/' + k], msg=k, floor=0.05 if k.endswith('lin_key.bias') else 1e-3)


def _rollout(g, batch):
    from model.mpnnlstm import masked_mse
    from model.seq2seq import Seq2Seq
    model = Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.15, input_timesteps=2, input_features=6, output_timesteps=3,
                    n_layers=1, n_conv_layers=2, transform_func=dist_from_05, convolution_type='MHTransformerConv')
    load_state(model, g, 'w/')
    model.to(dev()).eval()
    x, y, concat = (torch.from_numpy(np.stack([g[k]] * batch) if batch > 1 else g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
    loss = masked_mse(outs, meshes, y, g['mask'])
    loss.backward()
    return model, outs, meshes, loss


def _check_grads(model, g):
    for k, p in model.named_parameters():
        ref = g['g/' + k]
        if p.grad is None:
            assert not ref.any(), f'{k}: no gradient on the HIP path but the reference gradient is non-zero'
            continue
        grad_close(p.grad, ref, msg=k, floor=0.05 if k.endswith('lin_key.bias') else 1e-3)


def test_mh_rollout_golden():
    """Masked ice-like rollout with convolution_type='MHTransformerConv': the mesh of every step (labels bit-exact), outputs, loss
    and every gradient against the reference."""
    g = golden('mh_rollout.npz')
    model, outs, meshes, loss = _rollout(g, 1)
    # the input mesh, then one re-mesh per decoder step but the last (whose state update is deferred)
    for i, ms in enumerate(meshes):
        lab = ms.labels[0].cpu().numpy()
        assert np.array_equal(np.where(lab >= 0, lab, -1), g[f'labels_{i}']), f'mesh of step {i}'
    for i, o in enumerate(outs):
        assert o.shape[0] == g[f'out_{i}'].shape[0], f'mesh size of step {i}'
        close(o, g[f'out_{i}'], msg=f'step {i}')
    assert abs(float(loss) - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
    _check_grads(model, g)


def test_mh_rollout_batched_equals_single_and_is_deterministic():
    """A batch of 3 identical clips reproduces the single-clip trace clip by clip, with the same loss and gradients; two runs give
    bit-identical losses and gradients (no atomics in the merge or attention backward)."""
    g = golden('mh_rollout.npz')
    model, outs, meshes, loss = _rollout(g, 3)
    for i, (o, ms) in enumerate(zip(outs, meshes)):
        off = ms.node_off.cpu().numpy()
        for c in range(3):
            lab = ms.labels[c].cpu().numpy()
            assert np.array_equal(np.where(lab >= 0, lab - off[c], -1), g[f'labels_{i}']), f'mesh {i} clip {c}'
            close(o[off[c]:off[c + 1]], g[f'out_{i}'], msg=f'step {i} clip {c}')
    assert abs(float(loss.detach()) - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
    _check_grads(model, g)
    model2, _, _, loss2 = _rollout(g, 3)
    assert torch.equal(loss.detach(), loss2.detach())
    for a, b in zip(model.parameters(), model2.parameters()):
        assert (a.grad is None) == (b.grad is None) and (a.grad is None or torch.equal(a.grad, b.grad))


def test_graphed_mh_step_bit_identical_to_eager_and_replays_draw_new_masks():
    """A training step with MHTransformerConv captured into a hipGraph replays to the eager step's loss and weights, bit for bit
    (dropout off); with attention dropout on, two replays of a frozen model on the same batch draw different masks."""
    from model.model import CONVOLUTION_KWARGS
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(1, 0, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    x2, y2 = synthetic.make_batch(1, 50, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    t = lambda a: torch.from_numpy(a).to(dev())
    mask = np.zeros((64, 64), dtype=bool)
    concat = torch.zeros(2, 3, 64, 64, 1, device=dev())

    def fresh(lr):
        torch.manual_seed(5)
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=3, device=dev(),
                                    model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2,
                                                      convolution_type='MHTransformerConv'))
        nfp.initiate_training(lr=lr, lr_decay=0.95, capturable=True)
        nfp.model.static_shapes = True
        return nfp
    old = dict(CONVOLUTION_KWARGS['MHTransformerConv'])
    try:
        CONVOLUTION_KWARGS['MHTransformerConv']['dropout'] = 0.0
        eager, graphed = fresh(1e-3), fresh(1e-3)
        for _ in range(2):
            eager.train_step(t(x), t(y), concat, mask)
        step = graphed.make_graphed_step(t(x), t(y), concat, mask, warmup=2)
        for a, b in ((x2, y2), (x, y)):
            le, lg = float(eager.train_step(t(a), t(b), concat, mask)), float(step(t(a), t(b), concat))
            assert np.isfinite(le) and le == lg, (le, lg)
        for (k, p), (_, q) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
            assert torch.equal(p, q), k
        CONVOLUTION_KWARGS['MHTransformerConv']['dropout'] = 0.3
        drop = fresh(0.0)
        step = drop.make_graphed_step(t(x), t(y), concat, mask, warmup=2)
        l1, l2 = float(step(t(x), t(y), concat)), float(step(t(x), t(y), concat))
        assert np.isfinite(l1) and np.isfinite(l2) and l1 != l2, (l1, l2)
    finally:
        CONVOLUTION_KWARGS['MHTransformerConv'].update(old)


@pytest.mark.parametrize('use_graph', [False, True])
def test_trainer_runs_mh_model_and_round_trips_checkpoint(use_graph, tmp_path):
    """NextFramePredictorS2S(..., convolution_type='MHTransformerConv', hidden_size=16).train() on a tiny loader, eager and with
    the step replayed as a hipGraph, then predict(), save() and load() into a second instance (weights bit for bit)."""
    from helpers import TinyLoader
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(5, 0, 4, 3, 2, n_digits=1, pixel_noise=0.0)
    items = [(torch.from_numpy(x[i:i + 2]), torch.from_numpy(y[i:i + 2]), torch.zeros(1)) for i in (0, 2)]
    mask = np.zeros((64, 64), dtype=bool)
    mk = lambda: NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=2, device=dev(),
                                       experiment_name='mh', model_kwargs=dict(convolution_type='MHTransformerConv', hidden_size=16,
                                                                               dropout=0.1, n_layers=1))
    torch.manual_seed(3)
    nfp = mk()
    nfp.train(TinyLoader(items, (64, 64)), TinyLoader(items[:1], (64, 64)), n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask,
              truncated_backprop=0, use_graph=use_graph)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
    pred = nfp.predict(TinyLoader(items[:1], (64, 64)), mask=mask)
    assert pred.shape[-4:] == (2, 64, 64, 1) and np.isfinite(pred).all()
    nfp.save(str(tmp_path))
    other = mk()
    other.load(str(tmp_path))
    for (ka, a), (kb, b) in zip(nfp.model.state_dict().items(), other.model.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
