"""Per-pixel verification maps on the GPU (qt_score_maps, ops.rollout_score_maps, NextFramePredictorS2S.score_maps) against the
numpy restatement of tests/score_maps_restated.py, fed the project's own eager predict() frames of the same model and inputs.

Equality is exact, all 8 slots: both sides form d = f - y in fp32 and widen it (so |d| and d^2 are exact in float64) and add the
clips' terms to a pixel's running float64 sums one by one in loader order -- the same terms in the same order.  A difference means
one of these three is violated.

score() keeps the signature that tests/test_score_host.py pins, so the maps are asked for through score_maps(), the same call
with `.maps` filled in; everything the issue states for score(maps=True) is checked on score_maps()."""
import numpy as np
import pytest
import torch

from helpers import TinyLoader, dev
from score_maps_restated import restated_maps
from test_gpu_score import EPS, _case, _clips, _fields, _perturb  # noqa: F401  (_perturb: the cases' weights are perturbed)

pytestmark = pytest.mark.gpu


def _restated(nfp, loader, clim, extra, thr=0.15):
    fields = _fields(nfp, loader, clim, extra)
    truths = [y.astype(np.float32) for _, y, _ in _clips(loader)]
    return restated_maps(fields, truths, extra.get('mask'), thr)


@pytest.mark.parametrize('name', ['blob100', 'homogeneous_masked', 'ice_batched', 'transformer_pixelwise'])
def test_maps_equal_restatement_bit_for_bit(name):
    """blob100: P = 10000 = 39 * 256 + 16 (a part-empty last block), B = 2; homogeneous_masked: loss_mask, not the labels,
    excludes pixels; ice_batched: mask + re-meshing, a batch of 2 then a single clip (accumulation within a launch and across
    batches); transformer_pixelwise: climatology, S = 3, single clips."""
    nfp, loader, clim, extra = _case(name)
    nfp.model.eval()
    want = _restated(nfp, loader, clim, extra)
    sc = nfp.score_maps(loader, clim, **extra)
    W, H = loader.dataset.image_shape
    S = 3 if clim is not None else 2
    assert sc.maps.sources == sc.sources == ('model', 'persistence', 'climatology')[:S]
    assert sc.maps.sums.shape == want.shape == (nfp.output_timesteps, S, 8, W, H) and sc.maps.sums.dtype == np.float64
    n_clips = len(_clips(loader))
    keep = ~extra['mask'] if 'mask' in extra else np.ones((W, H), bool)
    assert (want[:, :, 0][..., keep] == n_clips).all() and want[:, :, 3].max() > 0
    for k in range(8):
        np.testing.assert_array_equal(sc.maps.sums[:, :, k], want[:, :, k], err_msg=f'{name}: slot {k}')
    assert nfp.model.static_shapes is False


def test_rollout_score_maps_over_more_than_16_steps():
    """17 steps over one repeated mesh: the second launch's z0 offsets of y, both baselines and maps.  Outputs are random (N, 4)
    rows (row stride 4, column 0 is read), persistence is one frame per clip (B*P), climatology a field per step (B*T*P)."""
    from qtmpnn import ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, _, _ = loader[0]
    x = x.to(dev())
    with torch.no_grad():
        _, meshes = nfp.model(x, teacher_forcing_ratio=0)
    mesh, T = meshes[0], 17
    B, P, (W, H) = mesh.B, mesh.P, loader.dataset.image_shape
    assert B == 2 and P == W * H
    g = torch.Generator(device='cpu').manual_seed(3)
    outs = [torch.rand(mesh.N, 4, generator=g).to(dev()) for _ in range(T)]
    y = torch.rand(B, T, W, H, 1, generator=g).to(dev())
    pers = torch.rand(B, W, H, generator=g).to(dev())
    field = torch.rand(B, T, W, H, generator=g).to(dev())
    maps = torch.zeros(T, 3, 8, P, dtype=torch.float64, device=dev())
    assert ops.rollout_score_maps(outs, [mesh] * T, y, maps, 0.5, persistence=pers, climatology=field) is maps
    lab = mesh.labels.cpu().numpy().reshape(B, P)
    assert lab.min() >= 0 and lab.max() < mesh.N
    fields, truths = [], []
    for b in range(B):
        model = np.stack([o.cpu().numpy()[lab[b], 0].reshape(W, H) for o in outs])
        fields.append({'model': model, 'persistence': np.repeat(pers[b].cpu().numpy()[None], T, axis=0),
                       'climatology': field[b].cpu().numpy()})
        truths.append(y[b, ..., 0].cpu().numpy())
    want = restated_maps(fields, truths, None, 0.5)
    got = maps.cpu().numpy().reshape(T, 3, 8, W, H)
    for k in range(8):
        np.testing.assert_array_equal(got[:, :, k], want[:, :, k], err_msg=f'slot {k}')
    assert (got[16, :, 0] == B).all() and got[16, :, 3].min() > 0
    # a second call adds the same clips again, onto the running values
    ops.rollout_score_maps(outs, [mesh] * T, y, maps, 0.5, persistence=pers, climatology=field)
    want2 = restated_maps(fields + fields, truths + truths, None, 0.5)
    np.testing.assert_array_equal(maps.cpu().numpy().reshape(T, 3, 8, W, H), want2)


def test_graphed_maps_equal_eager_bit_for_bit():
    """cheb_quadtree, batches of 2, 2 and 1 clips: two captures (each batch added once, by the warm-up) and one replay.  The eager
    side runs in static mode, as in test_graphed_score_equals_eager_bit_for_bit: that is the rollout a capture holds."""
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    nfp.model.static_shapes = True
    eager = nfp.score_maps(loader, clim, **extra)
    want = _restated(nfp, loader, clim, extra)                      # from the static-mode frames, the ones both sides score
    nfp.model.static_shapes = False
    graphed = nfp.score_maps(loader, clim, use_graph=True, **extra)
    assert nfp.model.static_shapes is False
    assert graphed.sources == eager.sources and graphed.maps.sources == eager.maps.sources
    assert graphed.sums.shape == eager.sums.shape and np.array_equal(graphed.sums, eager.sums)
    assert graphed.maps.sums.shape == eager.maps.sums.shape
    np.testing.assert_array_equal(graphed.maps.sums, eager.maps.sums)
    assert (graphed.maps.sums[:, :, 0] == 5).all()                  # every clip exactly once
    np.testing.assert_array_equal(graphed.maps.sums, want)


def test_maps_agree_with_the_sums():
    """One score_maps() call on ice_batched: summed over the pixels the maps give the per-clip sums summed over the clips.  Counts
    and n exactly; sum d, sum |d|, sum d^2 within k_score_multi's stated bound, 16 * 2^-24 * sum |term| per (clip, step) sum and
    hence for their total over the clips.  sum |term| comes from the maps, which are exact to float64 (their own rounding, at
    most (clips + pixels) * 2^-53 relative, is nine orders below the bound)."""
    nfp, loader, clim, extra = _case('ice_batched')
    nfp.model.eval()
    sc = nfp.score_maps(loader, clim, **extra)
    pooled = sc.maps.sums.sum(axis=(-2, -1))                        # (T, S, 8)
    clips = sc.sums.sum(axis=0)                                     # (T, S, 8)
    assert pooled.shape == clips.shape == (3, 2, 8)
    np.testing.assert_array_equal(pooled[..., [0, 4, 5, 6, 7]], clips[..., [0, 4, 5, 6, 7]])
    assert (pooled[..., 0] == 3 * int((~extra['mask']).sum())).all()
    absterm = np.stack([pooled[..., 2], pooled[..., 2], pooled[..., 3]], axis=-1)
    err = np.abs(pooled[..., 1:4] - clips[..., 1:4])
    print('max err / bound', float(np.max(err / (EPS * absterm))))
    assert (absterm > 0).all() and (err <= EPS * absterm).all(), (err, EPS * absterm)
    # ScoreMaps.pooled() is that sum: what derives from counts alone equals Scores.by_lead()'s
    for s, name in enumerate(sc.sources):
        lead, pl = sc.by_lead(name), sc.maps.pooled(name)
        np.testing.assert_array_equal(pl['n'], lead['n'])
        np.testing.assert_array_equal(pl['iiee'], lead['iiee'])
        np.testing.assert_array_equal(pl['accuracy'], lead['accuracy'])


def test_masked_pixels_stay_zero():
    nfp, loader, clim, extra = _case('quadtree_masked_64')
    nfp.model.eval()
    sc = nfp.score_maps(loader, clim, **extra)
    mask = extra['mask']
    assert mask.any() and sc.maps.sums.shape == (4, 2, 8, 64, 64)
    assert (sc.maps.sums[..., mask] == 0).all()
    assert (sc.maps.sums[:, :, 0][..., ~mask] == len(_clips(loader))).all()
    m = sc.maps.metrics('model')
    assert np.isnan(m['rmse'][:, mask]).all() and not np.isnan(m['rmse'][:, ~mask]).any()
    # a region of unmasked pixels pools to the restatement's numbers for those pixels
    region = np.zeros((64, 64), bool)
    region[30:50, 10:40] = True
    want = _restated(nfp, loader, clim, extra)[:, 0][..., region & ~mask].sum(-1)       # (T, 8)
    np.testing.assert_array_equal(sc.maps.pooled('model', weights=region)['over'], want[:, 5])
    np.testing.assert_array_equal(sc.maps.pooled('model', weights=region)['n'], want[:, 0])


def test_score_without_maps_is_unchanged():
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    plain = nfp.score(loader, clim, **extra)
    again = nfp.score(loader, clim, use_graph=False, **extra)
    with_maps = nfp.score_maps(loader, clim, **extra)
    assert plain.maps is None and again.maps is None and with_maps.maps is not None
    assert np.array_equal(plain.sums, again.sums) and np.array_equal(plain.sums, with_maps.sums)
    assert plain.sources == with_maps.sources
    graphed = nfp.score(loader, clim, use_graph=True, **extra)
    assert graphed.maps is None


def test_maps_refusals_by_name():
    from qtmpnn import ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    T, P = len(y_hat), meshes[0].P
    good = torch.zeros(T, 1, 8, P, dtype=torch.float64, device=dev())
    ops.rollout_score_maps(y_hat, meshes, y, good)
    assert (good[:, 0, 0] == x.shape[0]).all()
    for bad in (good.float(), good.cpu(), torch.zeros(T + 1, 1, 8, P, dtype=torch.float64, device=dev()),
                torch.zeros(T, 2, 8, P, dtype=torch.float64, device=dev()),
                torch.zeros(T, 1, 8, P + 1, dtype=torch.float64, device=dev()), good.transpose(0, 1), None):
        with pytest.raises(ValueError, match='rollout_score_maps: maps must be'):
            ops.rollout_score_maps(y_hat, meshes, y, bad)
    # with a baseline S = 2: the one-source buffer no longer fits
    with pytest.raises(ValueError, match='rollout_score_maps: maps must be'):
        ops.rollout_score_maps(y_hat, meshes, y, good, persistence=x[:, -1, :, :, 0])
    # everything rollout_scores refuses, under this op's name
    with pytest.raises(ValueError, match='rollout_score_maps: y has'):
        ops.rollout_score_maps(y_hat, meshes, y[:, :2], good)
    with pytest.raises(ValueError, match='rollout_score_maps: persistence has'):
        ops.rollout_score_maps(y_hat, meshes, y, good, persistence=x[0, -1, :, :, 0])
    with pytest.raises(ValueError, match='rollout_score_maps: climatology has'):
        ops.rollout_score_maps(y_hat, meshes, y, good, climatology=y[:, :2])
    with pytest.raises(ValueError, match='rollout_score_maps: outputs must be fp32'):
        ops.rollout_score_maps([o.double() for o in y_hat], meshes, y, good)
    with pytest.raises(ValueError, match='rollout_score_maps: 3 output steps for 4 meshes'):
        ops.rollout_score_maps(y_hat[:3], meshes, y, good)
    # a loader whose second batch has another frame shape
    x1, y1, d1 = loader[1]
    mixed = TinyLoader([loader[0], (x1[:, :, :32, :48].contiguous(), y1[:, :, :32, :48].contiguous(), d1)], (64, 64))
    for use_graph in (False, True):
        with pytest.raises(ValueError, match=r'score_maps: a batch of \(32, 48\) frames after \(64, 64\)'):
            nfp.score_maps(mixed, clim, use_graph=use_graph, **extra)
        assert nfp.model.static_shapes is False
