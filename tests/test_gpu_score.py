"""score(): per-lead-time forecast verification on the GPU (qt_score_rollout, ops.rollout_scores, NextFramePredictorS2S.score)
against the numpy float64 restatement of tests/score_restated.py.  The restatement is fed the project's own eager predict()
frames of the same model and inputs, so both sides score identical fp32 forecasts.

Counts (slots 0, 4-7) must be equal.  Sums (slots 1-3): the restatement forms d = f - y exactly (float64 of two fp32 values); the
kernel rounds d once, |d| not again, d^2 at most twice more, and a tile's sum passes through at most 3 sequential adds, 6
butterfly steps and 2 combines -- at most 14 roundings per term, so to first order |gpu - f64| <= 16 * 2^-24 * sum |term| per
tile and hence for the total (the tile totals are added in float64).  The bound is computed from the restatement's sum |term|."""
import numpy as np
import pytest
import torch

from helpers import TinyLoader, climatology_from_base, dev, dist_from_05, golden, load_state
from score_restated import restated_sums
from test_gpu_predict_graph import LAUNCH, _config, _mask

pytestmark = pytest.mark.gpu

DAY = 86_400_000_000_000
EPS = 16 * 2.0 ** -24


def _perturb(nfp, seed=0):
    torch.manual_seed(seed)
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.05 * torch.randn_like(p))


def _loader(x, y, sizes, shape):
    """Items of `sizes` clips each (1 -> the (1, T, W, H, C) item of a batch_size=1 loader), launch dates one day apart."""
    assert sum(sizes) == len(x) == len(y)
    items, c0 = [], 0
    for s in sizes:
        items.append((torch.from_numpy(x[c0:c0 + s]), torch.from_numpy(y[c0:c0 + s]), torch.tensor([LAUNCH + DAY * c0])))
        c0 += s
    return TinyLoader(items, shape)


def _ice(with_clim):
    """Re-meshing quadtree rollout with a mask on the 96 x 128 ice fixture's inputs (12 tiles per clip): the golden weights and
    single clips with climatology, or one batch of 2 + a single clip without."""
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('rollout_ice96x128_masked_h8.npz')
    kw = dict(hidden_size=int(g['hidden']), dropout=0.0, n_layers=int(g['n_layers']), n_conv_layers=int(g['n_conv']),
              transform_func=dist_from_05)
    nfp = NextFramePredictorS2S(thresh=float(g['thresh']), input_features=3, input_timesteps=2, output_timesteps=3, device=dev(),
                                transform_func=dist_from_05, model_kwargs=kw)
    load_state(nfp.model, g, 'w/')
    # three clips from the one the fixture holds: as stored, flipped left-right under the same mask, rolled by 7 rows
    x = np.stack([g['x'], g['x'][:, :, ::-1], np.roll(g['x'], 7, axis=1)]).astype(np.float32)
    y = np.stack([g['y'], g['y'][:, :, ::-1], np.roll(g['y'], 7, axis=1)]).astype(np.float32)
    clim = torch.from_numpy(climatology_from_base(g['concat'][0, ..., 0])).to(dev()) if with_clim else None
    return nfp, _loader(x, y, [1, 1, 1] if with_clim else [2, 1], (96, 128)), clim, dict(mask=g['mask'])


def _blob100():
    """100 x 100 (P = 10000: nine full tiles and one of 784 pixels), no mask, B = 2."""
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('graph_100_2blob_clean.npz')
    nfp = NextFramePredictorS2S(thresh=float(g['thresh']), input_features=1, input_timesteps=2, output_timesteps=3, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2))
    _perturb(nfp, 1)
    x0 = g['x'].astype(np.float32)                                   # (2, 100, 100, 1): the two input frames
    x = np.stack([x0, np.roll(x0, 11, axis=2)])
    y = np.stack([np.stack([np.roll(x0[-1], 3 * (t + 1), axis=0) for t in range(3)]),
                  np.stack([np.roll(x0[0], -5 * (t + 1), axis=1) for t in range(3)])]).astype(np.float32)
    return nfp, _loader(x, y, [2], (100, 100)), None, {}


def _homogeneous():
    """Uniform preset mesh with a mask (48 x 64, P = 3072): partly masked cells keep their pixels, the labels do not encode the
    mask (Mesh.loss_mask)."""
    from model.graph_functions import create_static_homogeneous_graph
    from model.mpnnlstm import NextFramePredictorS2S
    g = golden('fixed_homog48x64.npz')
    nfp = NextFramePredictorS2S(thresh=-np.inf, input_features=3, input_timesteps=2, output_timesteps=3, device=dev(),
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2))
    _perturb(nfp, 2)
    gs = create_static_homogeneous_graph((48, 64), int(g['max_grid_size']), g['mask'], use_edge_attrs=False, device=dev())
    assert gs['mapping'].loss_mask is not None and g['mask'].any()
    x = np.stack([g['x'], g['x'][:, ::-1], np.roll(g['x'], 9, axis=2)]).astype(np.float32)
    y = np.stack([g['y'], g['y'][:, ::-1], np.roll(g['y'], 9, axis=2)]).astype(np.float32)
    return nfp, _loader(x, y, [2, 1], (48, 64)), None, dict(mask=g['mask'], graph_structure=gs)


def _case(name):
    if name == 'ice_clim':
        return _ice(True)
    if name == 'ice_batched':
        return _ice(False)
    if name == 'blob100':
        return _blob100()
    if name == 'homogeneous_masked':
        return _homogeneous()
    if name == 'quadtree_masked_64':
        nfp, loader, clim, extra = _config('cheb_quadtree')
        return nfp, loader, clim, dict(extra, mask=_mask((64, 64), 4))
    return _config(name)                       # 24 x 32 pixelwise TransformerConv with mask + climatology; 64 x 64 quadtree


def _clips(loader):
    """[(x (T_in, W, H, C), y (T_out, W, H), launch)] per clip of the loader."""
    out = []
    for x, y, launch in loader:
        for b in range(x.shape[0]):
            out.append((x[b].numpy(), y[b].numpy()[..., 0], launch))
    return out


def _fields(nfp, loader, clim, extra):
    """Per clip {source: (T_out, W, H) fp32}: the model's frames from eager predict(), persistence, climatology."""
    frames = nfp.predict(loader, clim, **extra)
    T = frames.shape[1]
    fields = []
    for c, (x, y, launch) in enumerate(_clips(loader)):
        f = {'model': frames[c, ..., 0], 'persistence': np.repeat(x[-1, ..., 0][None], T, axis=0)}
        if clim is not None:
            f['climatology'] = nfp.get_climatology_array(clim, launch).cpu().numpy()[..., 0]
        fields.append(f)
    return fields


def _check(sc, fields, loader, mask, thr):
    clips = _clips(loader)
    assert sc.sums.shape == (len(clips), fields[0]['model'].shape[0], len(sc.sources), 8) and sc.sums.dtype == np.float64
    assert sc.sources == tuple(fields[0])
    worst = 0.0
    for c, (x, y, launch) in enumerate(clips):
        for s, name in enumerate(sc.sources):
            want, absterms = restated_sums(fields[c][name].astype(np.float32), y.astype(np.float32), mask, thr)
            got = sc.sums[c, :, s]
            err = np.abs(got[:, 1:4] - want[:, 1:4])
            print(f'clip {c} {name}: counts {got[:, [0, 4, 5, 6, 7]].tolist()} | max err / bound '
                  f'{float(np.max(err / np.maximum(EPS * absterms, 1e-300))):.3f}')
            np.testing.assert_array_equal(got[:, [0, 4, 5, 6, 7]], want[:, [0, 4, 5, 6, 7]], err_msg=f'clip {c} {name}: counts')
            assert (err <= EPS * absterms).all(), (c, name, got[:, 1:4], want[:, 1:4], EPS * absterms)
            worst = max(worst, float(np.max(err / np.maximum(EPS * absterms, 1e-300))))
    return worst


@pytest.mark.parametrize('name', ['ice_clim', 'ice_batched', 'blob100', 'homogeneous_masked', 'quadtree_masked_64',
                                  'transformer_pixelwise', 'cheb_quadtree'])
def test_score_equals_restatement(name):
    nfp, loader, clim, extra = _case(name)
    nfp.model.eval()
    fields = _fields(nfp, loader, clim, extra)
    sc = nfp.score(loader, clim, **extra)
    assert sc.sources == ('model', 'persistence') + (('climatology',) if clim is not None else ())
    _check(sc, fields, loader, extra.get('mask'), 0.15)
    assert nfp.model.static_shapes is False
    # every unmasked pixel is counted, at every lead time and for every source
    n_valid = int((~extra['mask']).sum()) if 'mask' in extra else int(np.prod(loader.dataset.image_shape))
    assert (sc.sums[..., 0] == n_valid).all()
    # the pooled numbers come from the pooled sums
    lead = sc.by_lead('model')
    np.testing.assert_array_equal(lead['rmse'], np.sqrt(sc.sums[:, :, 0, 3].sum(0) / sc.sums[:, :, 0, 0].sum(0)))


def test_threshold_equal_to_a_predicted_value_is_not_ice():
    """Strict >: with the threshold set to the exact fp32 value one prediction takes, that pixel is no ice on both sides."""
    nfp, loader, clim, extra = _case('transformer_pixelwise')
    nfp.model.eval()
    fields = _fields(nfp, loader, clim, extra)
    keep = ~extra['mask']
    i, j = np.argwhere(keep)[len(np.argwhere(keep)) // 2]
    thr = float(fields[1]['model'][2, i, j])
    assert np.float32(thr) == fields[1]['model'][2, i, j] and not fields[1]['model'][2, i, j] > np.float32(thr)
    sc = nfp.score(loader, clim, threshold=thr, **extra)
    _check(sc, fields, loader, extra['mask'], thr)
    # nudging the threshold one fp32 step down makes exactly that pixel ice (and any other that holds the same value)
    below = float(np.nextafter(np.float32(thr), np.float32(-np.inf)))
    sc2 = nfp.score(loader, clim, threshold=below, **extra)
    _check(sc2, fields, loader, extra['mask'], below)
    ice = lambda s: s.sums[1, 2, 0, 4] + s.sums[1, 2, 0, 5]
    assert ice(sc2) - ice(sc) == int((fields[1]['model'][2][keep] == np.float32(thr)).sum()) >= 1


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise'])
def test_graphed_score_equals_eager_bit_for_bit(name):
    """cheb_quadtree: batches of 2, 2 and 1 clips (two captured shapes, one replay); transformer_pixelwise: single clips with
    climatology (every clip after the first a replay)."""
    nfp, loader, clim, extra = _case(name)
    nfp.model.eval()
    nfp.model.static_shapes = True
    static = nfp.score(loader, clim, **extra)
    static_pred = nfp.predict(loader, clim, **extra)
    nfp.model.static_shapes = False
    graphed = nfp.score(loader, clim, use_graph=True, **extra)
    assert nfp.model.static_shapes is False
    assert graphed.sources == static.sources and graphed.sums.shape == static.sums.shape
    assert np.array_equal(graphed.sums, static.sums), float(np.abs(graphed.sums - static.sums).max())
    again = nfp.score(loader, clim, use_graph=True, **extra)
    assert np.array_equal(again.sums, graphed.sums)
    assert nfp.model.static_shapes is False
    # against the restatement too, and the graphed predict of the same model is what it was
    _check(graphed, _fields(nfp, loader, clim, extra), loader, extra.get('mask'), 0.15)
    pred = nfp.predict(loader, clim, use_graph=True, **extra)
    assert pred.shape == static_pred.shape and np.array_equal(pred, static_pred, equal_nan=True)
    nfp.model.static_shapes = True
    kept = nfp.score(loader, clim, use_graph=True, **extra)
    assert nfp.model.static_shapes is True and np.array_equal(kept.sums, graphed.sums)


def test_persistence_rows_differ_only_through_y():
    """One frame serves every lead time: with the same truth at every step the persistence rows are identical (the model's are
    not), and they equal the restatement fed x[-1, ..., 0] repeated."""
    nfp, loader, clim, extra = _case('quadtree_masked_64')
    nfp.model.eval()
    same_y = TinyLoader([(x, y[:, :1].expand_as(y).contiguous(), d) for x, y, d in loader], loader.dataset.image_shape)
    sc = nfp.score(same_y, clim, **extra)
    p = sc.sums[:, :, sc.sources.index('persistence')]
    assert (p == p[:, :1]).all() and p[..., 3].min() > 0
    m = sc.sums[:, :, 0]
    assert not (m[..., 3] == m[:, :1, 3]).all()
    _check(sc, _fields(nfp, same_y, clim, extra), same_y, extra['mask'], 0.15)


def test_rollout_scores_tile_left_empty_by_the_mask():
    """ops.rollout_scores per tile: the mask covers the whole first 1024-pixel tile (rows 0-15 of a 64-wide frame) and part of
    the second; that tile's 8 slots are zero for every source and the totals are the restatement's.  Baselines given as
    B*T*P (per-step) and B*P (one frame) fields; a second call gives the same bits."""
    from qtmpnn import ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    mask = np.zeros((64, 64), dtype=bool)
    mask[:16] = True
    mask[16:20, 5:40] = True
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0, mask=mask)
        field = torch.rand(y.shape, device=dev())
        tiles = ops.rollout_scores(y_hat, meshes, y, 0.15, persistence=x[:, -1, :, :, 0], climatology=field, per_tile=True)
        total = ops.rollout_scores(y_hat, meshes, y, 0.15, persistence=x[:, -1, :, :, 0], climatology=field)
        total2 = ops.rollout_scores(y_hat, meshes, y, 0.15, persistence=x[:, -1, :, :, 0], climatology=field)
    T, B = y.shape[1], y.shape[0]
    assert tiles.shape == (T, B, 4, 3, 8) and tiles.dtype == torch.float32
    assert total.shape == (T, B, 3, 8) and total.dtype == torch.float64 and total.is_cuda
    assert torch.equal(total, total2) and torch.equal(total, tiles.double().sum(2))
    tiles = tiles.cpu().numpy()
    assert (tiles[:, :, 0] == 0).all()
    assert (tiles[:, :, 1, :, 0] == 1024 - 4 * 35).all() and (tiles[:, :, 2:, :, 0] == 1024).all()
    loader1 = TinyLoader([loader[0]], (64, 64))
    frames = nfp.predict(loader1, None, mask=mask)
    got = total.cpu().numpy()
    for b in range(B):
        srcs = [frames[b, ..., 0], np.repeat(x[b, -1, :, :, 0].cpu().numpy()[None], T, axis=0), field[b, ..., 0].cpu().numpy()]
        for s, f in enumerate(srcs):
            want, absterms = restated_sums(f, y[b, ..., 0].cpu().numpy(), mask, 0.15)
            np.testing.assert_array_equal(got[:, b, s][:, [0, 4, 5, 6, 7]], want[:, [0, 4, 5, 6, 7]])
            assert (np.abs(got[:, b, s, 1:4] - want[:, 1:4]) <= EPS * absterms).all()


def test_rollout_scores_refuses_by_name():
    from qtmpnn import ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    with pytest.raises(ValueError, match='rollout_scores: y has'):
        ops.rollout_scores(y_hat, meshes, y[:, :2])
    with pytest.raises(ValueError, match='rollout_scores: persistence has'):
        ops.rollout_scores(y_hat, meshes, y, persistence=x[0, -1, :, :, 0])
    with pytest.raises(ValueError, match='rollout_scores: climatology has'):
        ops.rollout_scores(y_hat, meshes, y, climatology=y[:, :2])
    with pytest.raises(ValueError, match='rollout_scores: outputs must be fp32'):
        ops.rollout_scores([o.double() for o in y_hat], meshes, y)
    with pytest.raises(ValueError, match='rollout_scores: outputs must be fp32'):
        ops.rollout_scores([o.cpu() for o in y_hat], meshes, y)
    # outputs under autograd are detached, not refused
    outs, meshes = nfp.model(x, teacher_forcing_ratio=0)
    assert outs[0].requires_grad
    s = ops.rollout_scores(outs, meshes, y)
    assert not s.requires_grad and s.shape == (len(outs), x.shape[0], 1, 8)
