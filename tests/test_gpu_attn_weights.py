"""GPU checks of the attention coefficients (qt_attn_weights, return_attention_weights, Seq2Seq.record_attention): the convolutions
against the restatement of PyG (tests/attn_restated.py), batching, dropout, the model-level records against the reference's rollout
(tests/golden/attn_rollout.npz from tests/golden/make_golden_attn.py), selection, the dropout stream and graph capture."""
import random

import numpy as np
import pytest
import torch

from helpers import close, dev, golden, load_state

pytestmark = pytest.mark.gpu


def _quadtree(seeds=(33,)):
    from qtmpnn import synthetic
    from qtmpnn.mesh import build_mesh
    imgs = [synthetic.make_clip(s, canvas=(64, 64), n_digits=1, n_frames=1, pixel_noise=0.0)[0, ..., 0] for s in seeds]
    return build_mesh(src=torch.from_numpy(np.stack(imgs)).to(dev()), thresh=0.1)


def _pixelwise():
    from qtmpnn.mesh import build_pixel_mesh
    mask = np.zeros((24, 32), dtype=bool)
    mask[:5, :7] = True
    return build_pixel_mesh(1, 24, 32, mask, dev())


def _conv(kind, cin, cout, seed):
    from model.model import CONVOLUTION_KWARGS, MHTransformerConv, TransformerConv
    cls = TransformerConv if kind == 'T' else MHTransformerConv
    torch.manual_seed(seed)
    conv = cls(cin, cout, **CONVOLUTION_KWARGS[cls.__name__])
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randn(p.shape) * (0.5 if p.dim() > 1 else 0.2))
    return conv.to(dev()).eval()


def _restated(conv):
    """The restatement with the module's weights (CPU)."""
    import mh_restated
    H = getattr(conv, 'heads', 1)
    r = mh_restated.TransformerConv(conv.in_channels, conv.out_channels, heads=H, concat=H > 1 or hasattr(conv, 'lin'), edge_dim=2)
    r.load_state_dict({k: v.cpu() for k, v in conv.state_dict().items() if not k.startswith('lin.')})
    return r.eval()


CONVS = [('T', 6, 8), ('T', 8, 1), ('M', 6, 8), ('M', 8, 1)]


@pytest.mark.parametrize('kind,cin,cout', CONVS)
@pytest.mark.parametrize('mesh_kind', ['quadtree', 'pixelwise'])
def test_conv_weights_against_restatement(kind, cin, cout, mesh_kind):
    """edge_index = mesh.edge_index(True); alpha against the restatement; alpha sums to 1 per target; sum_j alpha (v_j + e) + skip
    (and the head merge) reproduces out; out is bit-identical with and without the flag, keyword or positional."""
    from attn_restated import coefficients
    from qtmpnn import ops
    mesh = _quadtree() if mesh_kind == 'quadtree' else _pixelwise()
    if mesh_kind == 'quadtree':
        assert bool((mesh.npix > 1).any()), 'the quadtree mesh must carry self pairs'
    conv = _conv(kind, cin, cout, 7 + cin + cout)
    H = getattr(conv, 'heads', 1)
    x = torch.randn(mesh.N, cin, device=dev(), generator=torch.Generator(device=dev()).manual_seed(3))
    calls = ops._ATTN_CALLS[0]
    out0 = conv(x, mesh)
    out1, (ei, alpha) = conv(x, mesh, return_attention_weights=True)
    out2, (ei2, alpha2) = conv(x, mesh, None, True)              # PyG's positional flag
    assert ops._ATTN_CALLS[0] == calls + 3
    assert torch.equal(out0, out1) and torch.equal(out0, out2)
    assert torch.equal(ei, mesh.edge_index(True)) and ei.dtype == torch.int64
    assert torch.equal(ei, ei2) and torch.equal(alpha, alpha2)
    assert alpha.shape == (ei.shape[1], H) and alpha.dtype == torch.float32 and not alpha.requires_grad
    ea = mesh.edge_attrs(True)
    r = _restated(conv)
    xc, eic, eac = x.cpu(), ei.cpu(), ea.cpu()
    close(alpha, coefficients(r, xc, eic, eac).detach(), rtol=1e-4, atol=1e-5, msg='alpha')
    src, dst = eic
    close(torch.zeros(mesh.N, H).index_add(0, dst, alpha.cpu()), np.ones((mesh.N, H)), rtol=1e-5, atol=1e-5, msg='sum')
    with torch.no_grad():
        v = r.lin_value(xc).view(-1, H, cout)
        e = r.lin_edge(eac).view(-1, H, cout)
        agg = torch.zeros(mesh.N, H, cout).index_add(0, dst, alpha.cpu().unsqueeze(-1) * (v[src] + e))
        rebuilt = agg.reshape(mesh.N, H * cout) + r.lin_skip(xc)
        if hasattr(conv, 'lin'):
            rebuilt = rebuilt @ conv.lin.weight.cpu().t() + conv.lin.bias.cpu()
    close(out0, rebuilt, rtol=1e-4, atol=1e-5, msg='out rebuilt from alpha')


def test_batched_mesh_and_dropout():
    """On a block-diagonal mesh of 3 clips alpha equals the per-clip results; in train() mode with dropout 0.1 alpha equals the
    eval-mode alpha, and out with the flag equals out without it for the same seed."""
    from qtmpnn import ops
    seeds = (33, 9, 21)
    big = _quadtree(seeds)
    conv = _conv('T', 6, 8, 5)
    x = torch.randn(big.N, 6, device=dev())
    _, (ei, alpha) = conv(x, big, return_attention_weights=True)
    off = big.node_off.cpu().tolist()
    for b, s in enumerate(seeds):
        one = _quadtree((s,))
        assert one.N == off[b + 1] - off[b]
        _, (ei1, a1) = conv(x[off[b]:off[b + 1]], one, return_attention_weights=True)
        sel = (ei[0] >= off[b]) & (ei[0] < off[b + 1])
        assert torch.equal(ei[:, sel] - off[b], ei1)
        close(alpha[sel], a1, rtol=1e-5, atol=1e-6, msg=f'clip {b}')
    conv.dropout = 0.1
    conv.train()
    calls = ops._ATTN_CALLS[0]
    out_plain = conv(x, big)
    ops._ATTN_CALLS[0] = calls                      # the same seed again
    out_flag, (ei_t, alpha_t) = conv(x, big, return_attention_weights=True)
    assert ops._ATTN_CALLS[0] == calls + 1
    assert torch.equal(out_plain, out_flag)
    assert torch.equal(ei_t, ei) and torch.equal(alpha_t, alpha)
    conv.eval()
    assert not torch.equal(conv(x, big), out_plain), 'dropout did not act'


def _fixture_model(g):
    from model.seq2seq import Seq2Seq
    model = Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.1, input_timesteps=2, input_features=4, output_timesteps=2, n_layers=1,
                    n_conv_layers=2, convolution_type='TransformerConv')
    load_state(model, g, 'w/')
    return model.to(dev()).eval()


def _check_records(records, g):
    n = int(g['n_records'])
    want = {(str(g[f'name_{i}']), int(g[f't_{i}'])): i for i in range(n)}
    got = {(r['name'], r['t']): r for r in records}
    assert len(got) == len(records) == n and set(got) == set(want)
    for key, i in want.items():
        r = got[key]
        assert r['phase'] == key[0].split('.')[0]
        assert np.array_equal(r['edge_index'].cpu().numpy(), g[f'edges_{i}']), key
        assert torch.equal(r['edge_index'], r['mesh'].edge_index(True))
        close(r['alpha'], g[f'alpha_{i}'], rtol=0, atol=1e-4, msg=str(key))


def test_rollout_records_match_reference():
    """Seq2Seq.record_attention over the fixture's rollout: one record per (name, t) of the reference's forward, edges exactly equal,
    alpha within 1e-4; predictions bit-identical with and without recording."""
    g = golden('attn_rollout.npz')
    model = _fixture_model(g)
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    with torch.no_grad():
        outs0, _ = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
        with model.record_attention() as records:
            outs1, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
    for i, (a, b) in enumerate(zip(outs0, outs1)):
        assert torch.equal(a, b), f'step {i}'
        close(a, g[f'out_{i}'], msg=f'out {i}')
    _check_records(records, g)
    assert {r['mesh'] for r in records if r['phase'] == 'decoder' and r['t'] == 1} == {meshes[1]}


def test_predictor_attention_weights_match_reference():
    """NextFramePredictorS2S.attention_weights: the same records through the trainer class."""
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('attn_rollout.npz')
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=2, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2,
                                                  convolution_type='TransformerConv'))
    load_state(nfp.model, g, 'w/')
    nfp.model.eval()
    records = nfp.attention_weights(torch.from_numpy(g['x']), torch.from_numpy(g['concat']), mask=g['mask'])
    _check_records(records, g)


def _count_launches(monkeypatch):
    from qtmpnn import ops
    n = [0]
    call = ops._lib.call

    def counting(name, *a):
        n[0] += name == 'qt_attn_weights'
        return call(name, *a)
    monkeypatch.setattr(ops._lib, 'call', counting)
    return n


def test_select_and_launch_counts(monkeypatch):
    """select by names and by predicate; unselected convolutions and runs outside the block launch nothing."""
    g = golden('attn_rollout.npz')
    model = _fixture_model(g)
    x, concat = torch.from_numpy(g['x']).to(dev()), torch.from_numpy(g['concat']).to(dev())
    n = _count_launches(monkeypatch)
    with torch.no_grad():
        model(x, None, concat, teacher_forcing_ratio=0, mask=g['mask'])
        assert n[0] == 0
        name = 'encoder.rnns.0.conv_h_c.convolutions.1'
        with model.record_attention([name, 'decoder.fc_out2']) as rec:
            model(x, None, concat, teacher_forcing_ratio=0, mask=g['mask'])
        assert sorted((r['name'], r['t']) for r in rec) == [('decoder.fc_out2', 0), ('decoder.fc_out2', 1), (name, 0), (name, 1)]
        assert n[0] == 4
        with model.record_attention(lambda s: s.startswith('decoder.rnns.0.conv_x')) as rec:
            model(x, None, concat, teacher_forcing_ratio=0, mask=g['mask'])
        assert len(rec) == 8 and all(r['name'].startswith('decoder.rnns.0.conv_x') and r['phase'] == 'decoder' for r in rec)
        assert n[0] == 4 + 8
        with model.record_attention() as rec:
            model(x, None, concat, teacher_forcing_ratio=0, mask=g['mask'])
        # encoder: one launch per layer for all eight stacks (2 layers x 2 steps); decoder: one per step for the cell's layer, and
        # the two head convolutions per step
        assert len(rec) == int(g['n_records']) and n[0] == 4 + 8 + 4 + 2 * 3


def _mh_model():
    from model.seq2seq import Seq2Seq
    torch.manual_seed(4)
    return Seq2Seq(hidden_size=8, dropout=0.1, thresh=0.1, input_timesteps=2, input_features=4, output_timesteps=2, n_layers=1,
                   n_conv_layers=2, convolution_type='MHTransformerConv').to(dev())


@pytest.mark.parametrize('conv', ['TransformerConv', 'MHTransformerConv'])
def test_recorded_training_step_keeps_the_dropout_stream(conv):
    """train() mode, dropout 0.1: a recorded forward returns the same outputs as an unrecorded one from the same state, and the next
    unrecorded step's loss is unchanged -- recording moved neither the attention-dropout seeds nor the device epoch.  The per-
    convolution path of MHTransformerConv cells records too (alpha rows sum to 1 per target and head)."""
    from model.mpnnlstm import masked_mse
    from model.seq2seq import Seq2Seq
    from qtmpnn import ops
    g = golden('attn_rollout.npz')
    if conv == 'TransformerConv':
        model = Seq2Seq(hidden_size=8, dropout=0.1, thresh=0.1, input_timesteps=2, input_features=4, output_timesteps=2, n_layers=1,
                        n_conv_layers=2, convolution_type=conv)
        load_state(model, g, 'w/')
        model.to(dev())
    else:
        model = _mh_model()
    model.train()
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))

    def step():
        outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
        return outs, masked_mse(outs, meshes, y, g['mask'])

    model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])          # (creates the device epoch counter)
    torch.cuda.synchronize()
    state = (ops._ATTN_CALLS[0], {k: v.clone() for k, v in ops._ATTN_EPOCH.items()}, torch.cuda.get_rng_state(), random.getstate())

    def restore():
        ops._ATTN_CALLS[0] = state[0]
        for k, v in state[1].items():
            ops._ATTN_EPOCH[k].copy_(v)
        torch.cuda.set_rng_state(state[2])
        random.setstate(state[3])
    outs_a, _ = step()
    _, loss_a = step()
    restore()
    with model.record_attention() as rec:
        outs_b, _ = step()
    _, loss_b = step()
    for a, b in zip(outs_a, outs_b):
        assert torch.equal(a, b)
    assert float(loss_a.detach()) == float(loss_b.detach())
    # per step: 8 stacks x 2 layers in the encoder, 8 stacks + the two head convolutions in the decoder
    assert len({(r['name'], r['t']) for r in rec}) == len(rec) == 2 * 16 + 2 * 10
    for r in rec:
        H = r['alpha'].shape[1]
        assert H == (3 if conv == 'MHTransformerConv' else 1)
        s = torch.zeros(r['mesh'].N, H, device=dev()).index_add(0, r['edge_index'][1], r['alpha'])
        close(s, np.ones((r['mesh'].N, H)), rtol=1e-5, atol=1e-5, msg=r['name'])


def test_recording_refuses_graph_capture():
    """Recording inside make_graphed_rollout / make_graphed_step raises RuntimeError (static mode: the edge lists need host reads)."""
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('attn_rollout.npz')
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=2, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2,
                                                  convolution_type='TransformerConv'))
    load_state(nfp.model, g, 'w/')
    nfp.model.eval()
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    with nfp.model.record_attention() as rec:
        with pytest.raises(RuntimeError, match='graph capture'):
            nfp.make_graphed_rollout(x, concat, mask=g['mask'])
    assert not rec
    nfp.model.static_shapes = False
    torch.cuda.synchronize()
    nfp.initiate_training(lr=1e-3, lr_decay=0.95)
    nfp.model.train()
    with nfp.model.record_attention() as rec:
        with pytest.raises(RuntimeError, match='graph capture'):
            nfp.make_graphed_step(x.unsqueeze(0), y.unsqueeze(0), concat.unsqueeze(0), mask=g['mask'], warmup=1)
    assert not rec
    nfp.model.static_shapes = False
    torch.cuda.synchronize()
