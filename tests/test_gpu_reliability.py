"""reliability(): probability verification on the GPU (qt_reliability_rollout, ops.rollout_reliability,
NextFramePredictorS2S.reliability) against the numpy restatement of tests/reliability_restated.py.  Through reliability() the
restatement is fed the project's own eager predict() frames of the same model and inputs, so both sides bin identical fp32
forecasts; at the op level it is fed the hand-made node values themselves.

Counts (slots 0, 1) must be equal.  Float sums (slots 2, 3), per bin: the restatement forms its terms in float64.  The kernel
adds f itself (no rounding) and rounds f - o once and its square once more (the error of d enters d^2 twice: 3 roundings of the
term); a tile's sum then passes through at most 3 rounded sequential adds per thread (four pixels in pixel order, the first
add to +0 is exact, pixels of other bins add +0 exactly), 6 butterfly steps and 2 combines: 11 roundings.  That is at most 14
roundings on the longest chain, plus 2 for the second-order terms: R = 16, so |gpu - f64| <= 16 * 2^-24 * sum |term| per tile
and bin and hence for the total (the tile totals are added in float64).  This is k_score_multi's order and test_gpu_score's
EPS.  The bound is computed from the restatement's sum |term|."""
import functools

import numpy as np
import pytest
import torch

from helpers import dev
from reliability_restated import restated_reliability
from test_gpu_predict_graph import _config
from test_gpu_score import _case, _clips, _fields, _loader, _perturb

pytestmark = pytest.mark.gpu

EPS = 16 * 2.0 ** -24
SHAPE, T17, B2 = (24, 32), 17, 2           # the edge table's frame (P = 768: one ragged tile), steps (16 + 1) and clips
THR = 0.5


def _close(got, want, absterms, what):
    """Counts equal, float slots within EPS * sum |term|; -> worst err / bound."""
    np.testing.assert_array_equal(got[..., :2], want[..., :2], err_msg=f'{what}: counts')
    err = np.abs(got[..., 2:] - want[..., 2:])
    worst = float(np.max(err / np.maximum(EPS * absterms, 1e-300)))
    print(f'{what}: n per bin {got[..., 0].sum(axis=tuple(range(got.ndim - 2))).tolist()} | max err / bound {worst:.3f}')
    assert (err <= EPS * absterms).all(), (what, worst)
    return worst


def edge_table(K):
    """(B2, T17, 24, 32) fp32 fields for the three sources and the truth: every bin edge k / K as an fp32 value with its fp32
    neighbours on both sides, negatives, -0, values of 1 and above, tiny ones, and uniform values in (-0.1, 1.1) for the rest;
    their places differ per step, clip and source.  The truth holds 0 / 1, values around THR and THR itself."""
    rng = np.random.default_rng(100 + K)
    edges = (np.arange(K + 1, dtype=np.float32) / np.float32(K)).astype(np.float32)
    special = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                              np.array([-0.0, -0.25, -1e-30, -3.0, 1.5, 2.0, 7.0, 1e-30, 1e-10], np.float32)]).astype(np.float32)
    P = SHAPE[0] * SHAPE[1]
    fields = []
    for s in range(3):
        f = rng.uniform(-0.1, 1.1, (B2, T17, P)).astype(np.float32)
        for b in range(B2):
            for z in range(T17):
                at = rng.permutation(P)[:len(special)]
                f[b, z, at] = special
        fields.append(f.reshape(B2, T17, *SHAPE))
    y = rng.choice(np.array([0.0, 1.0, THR, np.nextafter(np.float32(THR), np.float32(1)), 0.2, 0.8], np.float32),
                   (B2, T17, *SHAPE)).astype(np.float32)
    return fields, y


def _restated_table(K, S):
    fields, y = edge_table(K)
    fields[1] = np.repeat(fields[1][:, :1], T17, axis=1)               # persistence: one frame for every lead time
    want = np.zeros((T17, B2, S, K, 4))
    absterms = np.zeros((T17, B2, S, K, 2))
    for b in range(B2):
        for s in range(S):
            want[:, b, s], absterms[:, b, s] = restated_reliability(fields[s][b], y[b], None, THR, K)
    return fields, y, want, absterms


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('K', [2, 10, 32])
def test_op_edge_table_over_two_launches(K, S):
    """Hand-made (N, 4) outputs on a 24 x 32 pixelwise mesh, 17 steps: a launch of 16 and a launch of 1 into the same partial
    buffer.  Column 0 carries the values (the other columns a decoy); with S = 3 persistence is a B*P frame and climatology a
    B*T*P field.  Every bin is populated, and the edges and their neighbours fall where the restatement puts them."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    fields, y, want, absterms = _restated_table(K, S)
    assert (want[..., 0].sum(axis=(0, 1)) > 0).any(axis=0).all(), 'a bin is empty for every source'
    mesh = build_pixel_mesh(B2, *SHAPE, None, dev())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    outs = []
    for z in range(T17):
        o = torch.full((B2 * SHAPE[0] * SHAPE[1], 4), 0.37, device=dev())
        o[:, 0] = t(fields[0][:, z]).reshape(-1)
        outs.append(o)
    kw = dict(persistence=t(fields[1][:, 0]), climatology=t(fields[2])) if S == 3 else {}
    got = ops.rollout_reliability(outs, [mesh] * T17, t(y), THR, K, **kw)
    tiles = ops.rollout_reliability(outs, [mesh] * T17, t(y), THR, K, per_tile=True, **kw)
    assert got.shape == (T17, B2, S, K, 4) and got.dtype == torch.float64 and got.is_cuda and not got.requires_grad
    assert tiles.shape == (T17, B2, 1, S, K, 4) and tiles.dtype == torch.float32
    assert torch.equal(got, tiles.double().sum(2))
    assert torch.equal(got, ops.rollout_reliability(outs, [mesh] * T17, t(y), THR, K, **kw))
    got = got.cpu().numpy()
    assert (got[..., 0].sum(axis=3) == SHAPE[0] * SHAPE[1]).all()
    _close(got, want, absterms, f'K={K} S={S}')


def test_nan_forecast_is_counted_in_bin_0():
    """A NaN node value: bin 0 of its step and clip counts it and has NaN float sums; every other bin, step and clip is the
    restatement's."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    fields, y, want, absterms = _restated_table(10, 1)
    f = fields[0][:, :3].copy()
    f[1, 2, 5, 7] = np.nan
    want, absterms = want[:3].copy(), absterms[:3].copy()
    want[:, 1, 0], absterms[:, 1, 0] = restated_reliability(f[1], y[1, :3], None, THR, 10)
    assert np.isnan(want[2, 1, 0, 0, 2:]).all() and np.isnan(want).sum() == 2
    mesh = build_pixel_mesh(B2, *SHAPE, None, dev())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    outs = [t(f[:, z]).reshape(-1, 1) for z in range(3)]
    got = ops.rollout_reliability(outs, [mesh] * 3, t(y[:, :3]), THR, 10).cpu().numpy()
    assert np.isnan(got[2, 1, 0, 0, 2:]).all() and np.isnan(got).sum() == 2
    np.testing.assert_array_equal(got[..., :2], want[..., :2])
    fin = np.isfinite(want[..., 2:])
    assert (np.abs(got[..., 2:] - want[..., 2:])[fin] <= (EPS * absterms)[fin]).all()


def _binary64():
    """A binary=True predictor (test_gpu_bce's) on 64 x 64 quadtrees with a 0 / 1 truth: batches of 2 and 1 clips."""
    from qtmpnn import synthetic
    from test_gpu_bce import _binary_predictor
    nfp = _binary_predictor(3)
    _perturb(nfp, 9)
    x, y = synthetic.make_batch(3, 0, 3, 3, 3, n_digits=1, pixel_noise=0.02)
    y = (y > 0.5).astype(np.float32)
    return nfp, _loader(x.astype(np.float32), y, [2, 1], (64, 64)), None, {}


CASES = {'ice_clim': (0.15, 10), 'blob100': (0.15, 32), 'homogeneous_masked': (0.15, 10), 'transformer_pixelwise': (0.15, 7),
         'binary64': (0.5, 10)}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(predictor, loader, climatology, kwargs, per-clip fields from eager predict()): made once per case, not modified."""
    nfp, loader, clim, extra = _binary64() if name == 'binary64' else _case(name)
    nfp.model.eval()
    return nfp, loader, clim, extra, _fields(nfp, loader, clim, extra)


def _check(rel, fields, loader, mask, thr, K, what):
    clips = _clips(loader)
    T = fields[0]['model'].shape[0]
    assert rel.sums.shape == (len(clips), T, len(rel.sources), K, 4) and rel.sums.dtype == np.float64
    assert rel.sources == tuple(fields[0]) and rel.bins == K and rel.threshold == thr
    worst = 0.0
    for c, (x, y, launch) in enumerate(clips):
        for s, name in enumerate(rel.sources):
            want, absterms = restated_reliability(fields[c][name].astype(np.float32), y.astype(np.float32), mask, thr, K)
            worst = max(worst, _close(rel.sums[c, :, s], want, absterms, f'{what} clip {c} {name}'))
    return worst


@pytest.mark.parametrize('name', list(CASES))
def test_reliability_equals_restatement(name):
    thr, K = CASES[name]
    nfp, loader, clim, extra, fields = _reference(name)
    rel = nfp.reliability(loader, clim, threshold=thr, bins=K, **extra)
    assert rel.sources == ('model', 'persistence') + (('climatology',) if clim is not None else ())
    _check(rel, fields, loader, extra.get('mask'), thr, K, name)
    assert nfp.model.static_shapes is False
    n_valid = int((~extra['mask']).sum()) if 'mask' in extra else int(np.prod(loader.dataset.image_shape))
    assert (rel.sums[..., 0].sum(axis=-1) == n_valid).all()
    # the derived numbers come from the pooled sums
    lead = rel.by_lead('model')
    np.testing.assert_array_equal(lead['brier'], rel.sums[:, :, 0, :, 3].sum(axis=(0, 2)) / rel.sums[:, :, 0, :, 0].sum(axis=(0, 2)))
    if name == 'binary64':
        # a probability head: every value is in [0, 1], and the events are the 0 / 1 truth itself
        ev = sum(float((y[..., 0] > 0.5).sum()) for _, y, _ in loader)
        assert rel.sums[:, :, 0, :, 1].sum() == ev > 0
        assert np.isfinite(lead['brier']).all() and (lead['brier'] <= 1).all()


def test_bin_totals_are_scores_counts():
    """The same loader through score(): summed over the bins, n is Scores' slot 0 and the events are its hits + misses."""
    thr, K = CASES['ice_clim']
    nfp, loader, clim, extra, _ = _reference('ice_clim')
    rel = nfp.reliability(loader, clim, threshold=thr, bins=K, **extra)
    sc = nfp.score(loader, clim, threshold=thr, **extra)
    assert rel.sources == sc.sources and len(rel.sources) == 3
    np.testing.assert_array_equal(rel.sums[..., 0].sum(axis=-1), sc.sums[..., 0])
    np.testing.assert_array_equal(rel.sums[..., 1].sum(axis=-1), sc.sums[..., 4] + sc.sums[..., 6])
    assert rel.sums[..., 1].sum() > 0
    assert rel.skill('model', 'climatology').shape == (sc.sums.shape[1],)


def test_tile_left_empty_by_the_mask():
    """ops.rollout_reliability per tile: the mask covers the whole first 1024-pixel tile (rows 0-15 of a 64-wide frame) and part
    of the second; that tile's slots are zero for every source and bin, and the bins of the others add up to their pixels."""
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
        args = dict(persistence=x[:, -1, :, :, 0], climatology=field)
        tiles = ops.rollout_reliability(y_hat, meshes, y, 0.15, 10, per_tile=True, **args)
        total = ops.rollout_reliability(y_hat, meshes, y, 0.15, 10, **args)
    T, B = y.shape[1], y.shape[0]
    assert tiles.shape == (T, B, 4, 3, 10, 4) and tiles.dtype == torch.float32
    assert total.shape == (T, B, 3, 10, 4) and torch.equal(total, tiles.double().sum(2))
    tiles = tiles.cpu().numpy()
    assert (tiles[:, :, 0] == 0).all()
    assert (tiles[:, :, 1, :, :, 0].sum(-1) == 1024 - 4 * 35).all() and (tiles[:, :, 2:, :, :, 0].sum(-1) == 1024).all()
    got = total.cpu().numpy()
    yb = y[..., 0].cpu().numpy()
    for b in range(B):
        want, absterms = restated_reliability(field[b, ..., 0].cpu().numpy(), yb[b], mask, 0.15, 10)
        _close(got[:, b, 2], want, absterms, f'clip {b} dense field')


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise'])
def test_graphed_reliability_equals_eager_bit_for_bit(name):
    """cheb_quadtree: batches of 2, 2 and 1 clips (two captured shapes, one replay); transformer_pixelwise: single clips with
    climatology (every clip after the first a replay)."""
    nfp, loader, clim, extra = _config(name)
    nfp.model.eval()
    nfp.model.static_shapes = True
    static = nfp.reliability(loader, clim, bins=10, **extra)
    nfp.model.static_shapes = False
    graphed = nfp.reliability(loader, clim, use_graph=True, bins=10, **extra)
    assert nfp.model.static_shapes is False
    assert graphed.sources == static.sources and graphed.sums.shape == static.sums.shape
    assert np.array_equal(graphed.sums, static.sums), float(np.abs(graphed.sums - static.sums).max())
    assert graphed.sums[..., 0].sum() > 0
    again = nfp.reliability(loader, clim, use_graph=True, bins=10, **extra)
    assert np.array_equal(again.sums, graphed.sums)
    nfp.model.static_shapes = True
    kept = nfp.reliability(loader, clim, use_graph=True, bins=10, **extra)
    assert nfp.model.static_shapes is True and np.array_equal(kept.sums, graphed.sums)


def test_reliability_refuses_by_name(monkeypatch):
    from qtmpnn import _lib, ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    ok = ops.rollout_reliability(y_hat, meshes, y)
    assert ok.shape == (len(y_hat), x.shape[0], 1, 10, 4)
    # from here on nothing may be launched
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    for bad in (1, 33, 10.0):
        with pytest.raises(ValueError, match='rollout_reliability: bins must be an integer in 2..32'):
            ops.rollout_reliability(y_hat, meshes, y, bins=bad)
        with pytest.raises(ValueError, match='reliability: bins must be an integer in 2..32'):
            nfp.reliability(loader, clim, bins=bad)
        with pytest.raises(ValueError, match='make_graphed_reliability: bins must be'):
            nfp.make_graphed_reliability(x, y, bins=bad)
    with pytest.raises(ValueError, match='rollout_reliability: y has'):
        ops.rollout_reliability(y_hat, meshes, y[:, :2])
    with pytest.raises(ValueError, match='rollout_reliability: persistence has'):
        ops.rollout_reliability(y_hat, meshes, y, persistence=x[0, -1, :, :, 0])
    with pytest.raises(ValueError, match='rollout_reliability: outputs must be fp32'):
        ops.rollout_reliability([o.cpu() for o in y_hat], meshes, y)
    with pytest.raises(ValueError, match='rollout_reliability: 3 output steps for'):
        ops.rollout_reliability(y_hat[:3], meshes, y)
    assert launched == [] and nfp.model.static_shapes is False
