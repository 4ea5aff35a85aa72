"""predict(use_graph=True): inference rollouts replayed as captured graphs, against eager predict() on the same model -- the
ice fixture, four model configurations with two batch shapes per loader, the host state a graphed call leaves behind, dropout
in train() and eval() mode -- and the forward-only cell launch (qt_lstm_infer) against the training launch it stands in for."""
import random

import numpy as np
import pytest
import torch

from helpers import TinyLoader, climatology_from_base, dev, dist_from_05, golden, load_state

pytestmark = pytest.mark.gpu

LAUNCH = 1_483_228_800_000_000_000          # 1 Jan 2017 in ns, as the loaders' launch dates


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_graphed_predict_golden():
    """test_predict_layout_and_values_golden's assertions on the graphed call: clip 0 is the warm-up, clip 1 a replay."""
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('variant_ice_exp.npz')
    kw = dict(hidden_size=32, dropout=0.1, n_layers=1, transform_func=dist_from_05, dummy=False, n_conv_layers=3,
              rnn_type='LSTM', convolution_type='TransformerConv')
    nfp = NextFramePredictorS2S(thresh=-np.inf, input_features=5, input_timesteps=3, output_timesteps=3, device=dev(),
                                transform_func=dist_from_05, model_kwargs=kw)
    load_state(nfp.model, g, 'w/')
    nfp.model.eval()
    clim = torch.from_numpy(climatology_from_base(g['clim_base'])).to(dev())
    items = [(torch.from_numpy(g['x'][c])[None], torch.from_numpy(g['y'][c])[None], torch.tensor([g['launch'][c]])) for c in range(2)]
    pred = nfp.predict(TinyLoader(items, (24, 32)), clim, mask=g['mask'], use_graph=True)
    ref = g['pred']
    assert pred.shape == ref.shape == (2, 3, 24, 32, 1)
    assert np.array_equal(np.isnan(pred), np.isnan(ref))
    assert np.isnan(pred[:, :, g['mask']]).all() and not np.isnan(pred[:, :, ~g['mask']]).any()
    np.testing.assert_allclose(np.nan_to_num(pred), np.nan_to_num(ref), rtol=1e-4, atol=1e-5)
    assert nfp.model.static_shapes is False


def _mask(shape, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, dtype=bool)
    m[: shape[0] // 4, : shape[1] // 3] = True                     # a land block
    m |= rng.random(shape) < 0.05                                  # and scattered masked pixels
    return m


def _config(name, dropout=0.0):
    """(predictor, loader, climatology or None, predict kwargs) with random weights (seeded).  Without climatology the loader
    yields batches of 2, 2 and 1 clips (two captured shapes, a replay on the second 2-clip batch); a climatology array belongs to
    one launch date, so that loader yields single clips (one shape, every clip after the first a replay)."""
    from model.graph_functions import create_static_heterogeneous_graph
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    torch.manual_seed(0)
    t_in, t_out = 3, 4
    extra, clim = {}, None
    if name == 'cheb_quadtree':
        shape = (64, 64)
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev(),
                                    model_kwargs=dict(hidden_size=16, dropout=dropout, n_layers=2, n_conv_layers=2))
        x, y = synthetic.make_batch(3, 0, 5, t_in, t_out, n_digits=1, pixel_noise=0.02)
    elif name == 'mh_quadtree':
        shape = (64, 64)
        nfp = NextFramePredictorS2S(thresh=0.15, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev(),
                                    model_kwargs=dict(hidden_size=8, dropout=dropout, n_layers=1, n_conv_layers=2,
                                                      transform_func=dist_from_05, convolution_type='MHTransformerConv'))
        x, y = synthetic.make_batch(4, 0, 5, t_in, t_out, n_digits=1, pixel_noise=0.02)
        extra['mask'] = _mask(shape, 1)
    elif name == 'preset_hetero':
        shape = (32, 40)
        mask, hir = _mask(shape, 2), np.zeros(shape, dtype=bool)
        hir[8:20, 10:30] = True
        nfp = NextFramePredictorS2S(thresh=-np.inf, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev(),
                                    model_kwargs=dict(hidden_size=16, dropout=dropout, n_layers=1, n_conv_layers=2))
        rng = np.random.default_rng(5)
        x = rng.random((5, t_in, *shape, 1), dtype=np.float32)
        y = rng.random((5, t_out, *shape, 1), dtype=np.float32)
        extra = dict(mask=mask, high_interest_region=hir,
                     graph_structure=create_static_heterogeneous_graph(shape, 8, mask, high_interest_region=hir,
                                                                       use_edge_attrs=False, device=dev()))
    elif name == 'transformer_pixelwise':
        shape = (24, 32)
        nfp = NextFramePredictorS2S(thresh=-np.inf, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev(),
                                    transform_func=dist_from_05,
                                    model_kwargs=dict(hidden_size=32, dropout=dropout, n_layers=1, n_conv_layers=3,
                                                      transform_func=dist_from_05, convolution_type='TransformerConv'))
        rng = np.random.default_rng(6)
        x = rng.random((4, t_in, *shape, 1), dtype=np.float32)
        y = rng.random((4, t_out, *shape, 1), dtype=np.float32)
        extra['mask'] = _mask(shape, 3)
        base = np.random.default_rng(7).random(shape, dtype=np.float32)
        clim = torch.from_numpy(climatology_from_base(base)).to(dev())
    else:
        raise KeyError(name)
    with torch.no_grad():                       # weights off their initial values (biases, LayerNorms) so every path matters
        for p in nfp.model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    if clim is not None:
        sizes = [1] * len(x)
    else:
        sizes = [2, 2, 1]
    items, c0 = [], 0
    for s in sizes:
        items.append((torch.from_numpy(x[c0:c0 + s]), torch.from_numpy(y[c0:c0 + s]), torch.tensor([LAUNCH + 86_400_000_000_000 * c0])))
        c0 += s
    return nfp, TinyLoader(items, shape), clim, extra


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise', 'preset_hetero', 'mh_quadtree'])
def test_graphed_predict_equals_eager(name):
    """Graphed predict == eager predict in static mode bit for bit, and == the default eager predict within 1e-6 (the two
    eager modes agree bit for bit here already where they do)."""
    nfp, loader, clim, extra = _config(name)
    nfp.model.eval()
    eager = nfp.predict(loader, clim, **extra)
    nfp.model.static_shapes = True
    static = nfp.predict(loader, clim, **extra)
    nfp.model.static_shapes = False
    graphed = nfp.predict(loader, clim, use_graph=True, **extra)
    assert nfp.model.static_shapes is False
    assert graphed.shape == eager.shape == (5 if clim is None else 4, 4, *loader.dataset.image_shape, 1)
    assert _same(graphed, static), float(np.nanmax(np.abs(graphed - static)))
    assert np.array_equal(np.isnan(graphed), np.isnan(eager))
    np.testing.assert_allclose(np.nan_to_num(graphed), np.nan_to_num(eager), rtol=0, atol=1e-6)
    if 'mask' in extra and name == 'transformer_pixelwise':
        assert np.isnan(graphed[:, :, extra['mask']]).all() and not np.isnan(graphed[:, :, ~extra['mask']]).any()
    # a second graphed call captures afresh and gives the same array
    assert _same(nfp.predict(loader, clim, use_graph=True, **extra), graphed)


@pytest.mark.parametrize('call', ['predict', 'score', 'event_dates'])
def test_graphed_predict_leaves_host_state_as_eager(call):
    """After an eval()-mode predict / score / event_dates (one loop serves them all): static_shapes restored, Python's `random`
    advanced as by the eager call, and the next eager training step (attention + decoder dropout in train() mode) gives the
    eager run's loss.  The graphed products themselves are pinned against the static-mode eager ones in their own files; the
    predict case keeps its comparison with the default eager array."""
    from qtmpnn import ops

    def run(use_graph):
        nfp, loader, clim, extra = _config('transformer_pixelwise', dropout=0.1)
        random.seed(11)
        ops._ATTN_CALLS[0] = 0
        ops.dropout_epoch(dev()).zero_()
        nfp.model.eval()
        kw = dict(kind='breakup', persist=2) if call == 'event_dates' else {}
        res = getattr(nfp, call)(loader, clim, use_graph=use_graph, **extra, **kw)
        state, static = random.getstate(), nfp.model.static_shapes
        nfp.model.train()
        nfp.initiate_training(lr=1e-3, lr_decay=0.95)
        x, y, launch = loader[0]
        concat = nfp.get_climatology_array(clim, launch)
        loss = float(nfp.train_step(nfp._clip(x), nfp._clip(y), concat, extra['mask']))
        return res, state, static, loss
    r_e, s_e, st_e, l_e = run(False)
    r_g, s_g, st_g, l_g = run(True)
    assert st_e is False and st_g is False
    assert s_g == s_e
    assert l_g == l_e, (l_g, l_e)
    if call == 'predict':
        np.testing.assert_allclose(np.nan_to_num(r_g), np.nan_to_num(r_e), rtol=0, atol=1e-6)


def test_graphed_predict_dropout_per_replay():
    """train() mode (predict does not switch to eval, like the reference): every replay draws new decoder and attention dropout
    masks; eval() mode: replays are identical."""
    nfp, loader, clim, extra = _config('transformer_pixelwise', dropout=0.3)
    same = TinyLoader([loader[0]] * 3, loader.dataset.image_shape)
    nfp.model.train()
    p = nfp.predict(same, clim, use_graph=True, **extra)
    keep = ~extra['mask']
    assert not np.array_equal(p[1][:, keep], p[2][:, keep])
    assert not np.array_equal(p[0][:, keep], p[1][:, keep])
    nfp.model.eval()
    p = nfp.predict(same, clim, use_graph=True, **extra)
    assert _same(p[0], p[1]) and _same(p[1], p[2])


@pytest.fixture
def launched(monkeypatch):
    from qtmpnn import _lib
    names, call = [], _lib.call

    def rec(name, *a):
        names.append(name)
        return call(name, *a)
    monkeypatch.setattr(_lib, 'call', rec)
    return names


@pytest.mark.parametrize('h', [8, 16, 32, 64, 128])
@pytest.mark.parametrize('pair', [False, True])
def test_forward_only_lstm_cell_bit_identical(h, pair, launched):
    """qt_lstm_infer == qt_lstm_fwd bit for bit, on (N, 4h) gate sums and on the paired (N, 2, 4h) input the attention stacks
    hand over; a node count read from the device (static capacity larger than the valid rows)."""
    from qtmpnn import ops
    from qtmpnn.mesh import Mesh
    torch.manual_seed(100 + h)
    N = 1000
    mesh = Mesh()
    mesh.n_dev = torch.tensor([N - 37], dtype=torch.int32, device=dev())
    G = torch.randn(N, 2, 4 * h, device=dev()) if pair else torch.randn(N, 4 * h, device=dev())
    Cp = torch.randn(N, h, device=dev())
    wc, b, ln = (torch.randn(*s, device=dev()) for s in ((3, h), (4, h), (4, h)))
    with torch.no_grad():
        inf = ops.lstm_cell(G, Cp, wc, b, ln, mesh)
    assert launched == ['qt_lstm_infer']
    train = ops.lstm_cell(G, Cp, wc.clone().requires_grad_(True), b, ln, mesh)
    assert launched[-1] == 'qt_lstm_fwd'
    for a, t in zip(inf, train):
        assert torch.equal(a[:N - 37], t.detach()[:N - 37])
