"""fss(): neighbourhood verification on the GPU (qt_fss_rollout, ops.rollout_fss, NextFramePredictorS2S.fss) against the numpy
int64 restatement of tests/fss_restated.py.  Everything is an integer, so every comparison is exact equality.  At the op level
the restatement is fed the hand-made node values themselves; through fss() it is fed the project's own eager predict() frames of
the same model and inputs, so both sides threshold identical fp32 forecasts."""
import copy
import functools

import numpy as np
import pytest
import torch

from fss_restated import indicator, restated_fss, window_counts
from helpers import dev
from test_gpu_predict_graph import _config
from test_gpu_score import _case, _clips, _fields

pytestmark = pytest.mark.gpu

THR = 0.5
DEFAULT = (1, 3, 5, 9, 17, 33)
SMALL, RAGGED = (24, 32), (40, 72)      # smaller than one patch and than the largest window; 2 x 3 tiles, ragged on both axes


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _blobs(rng, B, T, shape, block=6):
    """(B, T, *shape) fp32 in (0, 1): blocks of 6 x 6 pixels (they straddle the 32-pixel tile borders) with pixel noise, so the
    fields have ice regions with ragged edges on both sides of THR."""
    n, m = shape
    coarse = rng.random((B, T, -(n // -block), -(m // -block)))
    f = np.kron(coarse, np.ones((block, block)))[..., :n, :m]
    return (0.75 * f + 0.25 * rng.random((B, T, n, m))).astype(np.float32)


def _fields_for(shape, B, T, seed):
    """[model, persistence, climatology] and the truth, (B, T, *shape) fp32 each: blobs, with THR itself, its fp32 neighbours on
    both sides, NaN and +-inf at places that differ per step, clip and source.  Persistence is one frame for every lead time."""
    rng = np.random.default_rng(seed)
    t32 = np.float32(THR)
    special = np.array([t32, np.nextafter(t32, np.float32(-np.inf)), np.nextafter(t32, np.float32(np.inf)), np.nan, np.inf, -np.inf,
                        t32, np.nan], np.float32)
    out = []
    for s in range(4):
        f = _blobs(rng, B, T, shape)
        flat = f.reshape(B, T, -1)
        for b in range(B):
            for z in range(T):
                flat[b, z, rng.permutation(flat.shape[2])[:len(special)]] = special
        out.append(f)
    out[1] = np.repeat(out[1][:, :1], T, axis=1)
    return out[:3], out[3]


def _want(fields, y, mask, scales, S, counted=None):
    """(T, B, S, K, 5) int64 from the restatement."""
    B, T = y.shape[:2]
    want = np.zeros((T, B, S, len(scales), 5), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            want[:, b, s] = restated_fss(fields[s][b], y[b], mask, THR, scales, None if counted is None else counted[b])
    return want


def _outs(model, rows=None, fill=0.37):
    """Per step an (N, 4) matrix: the (B, T, P') node values in column 0, a decoy (ice) elsewhere and in rows beyond them."""
    outs = []
    for z in range(model.shape[1]):
        v = model[:, z].reshape(-1)
        o = torch.full((len(v) if rows is None else rows, 4), fill, device=dev())
        o[:len(v), 0] = _t(v)
        outs.append(o)
    return outs


@functools.lru_cache(maxsize=None)
def _small_table():
    fields, y = _fields_for(SMALL, 2, 17, 21)
    return fields, y, {sc: _want(fields, y, None, sc, 3) for sc in ((1, 3, 33), DEFAULT)}


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('scales', [(1, 3, 33), DEFAULT])
def test_op_edge_values_over_two_launches(scales, S):
    """Hand-made (N, 4) outputs on a 24 x 32 pixelwise mesh, B = 2, 17 steps: a launch of 16 and a launch of 1 into one buffer.
    Column 0 carries the values (a decoy above THR elsewhere); with S = 3 persistence is a B*P frame and climatology a B*T*P
    field.  The frame is smaller than the largest window and than one patch."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    fields, y, wants = _small_table()
    want = wants[scales][:, :, :S]
    B, T, K = 2, 17, len(scales)
    for f in fields + [y]:                                   # every special value is there, on both sides of the comparison
        assert np.isnan(f).any() and np.isinf(f).any() and (f == np.float32(THR)).any()
    assert (want[..., 2] > 0).all() and (want[:, :, :, -1, 3] > want[:, :, :, 0, 3]).all()
    mesh = build_pixel_mesh(B, *SMALL, None, dev())
    outs = _outs(fields[0], fill=0.87)
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2])) if S == 3 else {}
    got = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, scales, **kw)
    tiles = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, scales, per_tile=True, **kw)
    assert got.shape == (T, B, S, K, 5) and got.dtype == torch.int64 and got.is_cuda and not got.requires_grad
    assert tiles.shape == (T, B, 1, S, K, 5) and tiles.dtype == torch.int32
    assert torch.equal(got, tiles.sum(2, dtype=torch.int64))
    assert torch.equal(got, ops.rollout_fss(outs, [mesh] * T, _t(y), THR, scales, **kw))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (got[..., 0] == SMALL[0] * SMALL[1]).all()


@functools.lru_cache(maxsize=None)
def _ragged_table():
    """40 x 72, B = 2, T = 2: blobs, plus ice in the truth around the corner shared by tiles (0,0), (0,1), (1,0), (1,1) and in
    the frame's last rows and columns, and model ice on the other side of that corner."""
    fields, y = _fields_for(RAGGED, 2, 2, 22)
    y[..., 30:34, 30:34] = 0.9
    y[..., 36:40, 66:72] = 0.9
    fields[0][..., 32:36, 32:36] = 0.9
    fields[0][..., 0:3, 0:3] = 0.9
    return fields, y


TILE_PIXELS = [32 * 32, 32 * 32, 32 * 8, 8 * 32, 8 * 32, 8 * 8]


def test_ragged_tiles_and_halos():
    """A 40 x 72 pixelwise mesh: 2 x 3 tiles, ragged on both axes; every window above scale 1 crosses into a halo somewhere,
    and the ice at (31, 31) / (32, 32) is seen from centres of the diagonally opposite tiles."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    keep = np.ones(RAGGED, bool)
    io = indicator(y[0, 0], keep, THR)
    assert io[31, 31] and io[32, 32] and io[39, 71]          # a 3 x 3 window around either corner pixel crosses the tile corner
    want = _want(fields, y, None, DEFAULT, 3)
    mesh = build_pixel_mesh(B, *RAGGED, None, dev())
    outs = _outs(fields[0], fill=0.87)
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2]))
    got = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, DEFAULT, **kw)
    tiles = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, DEFAULT, per_tile=True, **kw)
    assert tiles.shape == (T, B, 6, 3, 6, 5) and torch.equal(got, tiles.sum(2, dtype=torch.int64))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    tiles = tiles.cpu().numpy()
    assert (tiles[..., 0] == np.array(TILE_PIXELS).reshape(1, 1, 6, 1, 1)).all()
    # a tile's own sums: tile (1, 2), rows 32-39 and columns 64-71, the frame's corner, from the restatement's window counts
    co = window_counts(io, 9)[32:, 64:]
    cs = window_counts(indicator(fields[0][0, 0], keep, THR), 9)[32:, 64:]
    k9 = DEFAULT.index(9)
    assert tiles[0, 0, 5, 0, k9].tolist() == [64, int(io[32:, 64:].sum()), int(((cs - co) ** 2).sum()), int((cs * cs).sum()),
                                              int((co * co).sum())]


def _land_mask():
    """(40, 72) bool: the whole tile (0, 1) (rows 0-31, columns 32-63), a block across the corner of the lower tiles and
    scattered pixels."""
    mask = np.random.default_rng(23).random(RAGGED) < 0.06
    mask[:32, 32:64] = True
    mask[30:35, 60:67] = True
    return mask


def _assert_uncounted_inside_windows(keep):
    """Some counted centre has an uncounted pixel inside its 3 x 3 window (and inside the frame)."""
    holes = window_counts((~keep).astype(np.int64), 3)
    assert (~keep).any() and (holes[keep] > 0).any()


@pytest.mark.parametrize('how', ['loss_mask', 'labels'])
def test_uncounted_pixels_under_a_mask(how):
    """The ragged frame with a mask, carried by Mesh.loss_mask (the labels know nothing of it) or by the labels (-1 under the
    mask, fewer nodes than pixels).  Uncounted pixels add nothing to a window and are no centres; the fully masked tile's slots
    are all zero."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    mask = _land_mask()
    keep = ~mask
    _assert_uncounted_inside_windows(keep)
    want = _want(fields, y, mask, DEFAULT, 3)
    assert (want[..., 0] == keep.sum()).all()
    if how == 'loss_mask':
        mesh = copy.copy(build_pixel_mesh(B, *RAGGED, None, dev()))
        mesh.loss_mask = _t(mask.astype(np.uint8))
        outs = _outs(fields[0], fill=0.87)
    else:
        mesh = build_pixel_mesh(B, *RAGGED, mask, dev())
        assert mesh.loss_mask is None and mesh.N == B * keep.sum() and (mesh.labels.cpu().numpy()[:, mask] == -1).all()
        outs = _outs(fields[0][:, :, keep], fill=0.87)       # node order is raster order over the unmasked pixels
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2]))
    got = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, DEFAULT, **kw)
    tiles = ops.rollout_fss(outs, [mesh] * T, _t(y), THR, DEFAULT, per_tile=True, **kw)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, tiles.sum(2, dtype=torch.int64))
    assert (tiles[:, :, 1] == 0).all() and (tiles[:, :, 0, ..., 0] > 0).all()


def test_quadtree_labels_on_a_static_capacity_mesh():
    """A quadtree mesh built with a mask in static mode: labels -1 under the mask, several pixels per node, N is the capacity
    B * n * m and the node count is on the device.  The output buffers hold ice in every row beyond the nodes; at step 1 the
    node count the kernel is given is 40 short, so the pixels of the last 40 nodes are uncounted there too."""
    from qtmpnn import ops
    from qtmpnn.mesh import build_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    mask = _land_mask()
    crit = _blobs(np.random.default_rng(24), B, 1, RAGGED)[:, 0]
    crit = np.where(crit > 0.5, crit, np.float32(0))         # cells of several pixels where the criterion is flat
    mesh = build_mesh(src=_t(crit), thresh=0.1, mask=mask, static=True)
    labels = mesh.labels.cpu().numpy().reshape(B, *RAGGED)
    N = mesh.n_valid
    assert mesh.N == B * RAGGED[0] * RAGGED[1] and 40 < N < mesh.N and (labels[:, mask] == -1).all()
    assert labels.max() == N - 1 and N < (labels >= 0).sum()                                       # some nodes span pixels
    stale = copy.copy(mesh)
    stale.n_dev = torch.tensor([N - 40], dtype=torch.int32, device=dev())
    rng = np.random.default_rng(25)
    node = (0.2 + 0.6 * rng.random((T, N))).astype(np.float32)
    node[:, rng.permutation(N)[:4]] = np.array([THR, np.nan, np.inf, np.nextafter(np.float32(THR), np.float32(1))], np.float32)
    outs = []
    for z in range(T):
        o = torch.full((mesh.N, 4), 0.87, device=dev())      # capacity rows and the other columns: ice, if they were read
        o[:N, 0] = _t(node[z])
        outs.append(o)
    counted = np.stack([labels >= 0, (labels >= 0) & (labels < N - 40)], axis=1)            # (B, T, n, m)
    assert counted[:, 0].sum() > counted[:, 1].sum() > 0
    _assert_uncounted_inside_windows(counted[0, 1])
    model = np.where(counted, node[np.arange(T)[None, :, None, None], np.maximum(labels, 0)[:, None]], np.float32(0.87))
    fields = [model.astype(np.float32), fields[1], fields[2]]
    want = _want(fields, y, None, DEFAULT, 3, counted)
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2]))
    got = ops.rollout_fss(outs, [mesh, stale], _t(y), THR, DEFAULT, **kw)
    tiles = ops.rollout_fss(outs, [mesh, stale], _t(y), THR, DEFAULT, per_tile=True, **kw)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, tiles.sum(2, dtype=torch.int64)) and (tiles[:, :, 1] == 0).all()
    assert (want[0, :, 0, 0, 0] == counted[:, 0].sum(axis=(1, 2))).all()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(predictor, loader, climatology, kwargs, per-clip fields from eager predict()): made once per case, not modified."""
    nfp, loader, clim, extra = _case(name)
    nfp.model.eval()
    return nfp, loader, clim, extra, _fields(nfp, loader, clim, extra)


@pytest.mark.parametrize('name', ['cheb_quadtree', 'quadtree_masked_64', 'transformer_pixelwise'])
def test_fss_equals_restatement_and_scores_table(name):
    """Re-meshing quadtree rollouts on 64 x 64 clips in batches of 2, 2 and 1 (the second with a mask), and a 24 x 32 pixelwise
    one with a mask and climatology: the sums are the restatement's on eager predict()'s frames, and the scale-1 slots are
    score()'s table on the same loader."""
    from qtmpnn.fss import FSS
    thr = 0.15
    nfp, loader, clim, extra, fields = _reference(name)
    r = nfp.fss(loader, clim, threshold=thr, **extra)
    assert isinstance(r, FSS) and r.scales == DEFAULT and r.threshold == thr
    assert r.sources == ('model', 'persistence') + (('climatology',) if clim is not None else ()) == tuple(fields[0])
    assert (len(r.sources) == 3) == (name == 'transformer_pixelwise')
    clips = _clips(loader)
    T = fields[0]['model'].shape[0]
    assert r.sums.shape == (len(clips), T, len(r.sources), 6, 5) and r.sums.dtype == np.int64
    mask = extra.get('mask')
    for c, (x, y, launch) in enumerate(clips):
        for s, src in enumerate(r.sources):
            want = restated_fss(fields[c][src].astype(np.float32), y.astype(np.float32), mask, thr, DEFAULT)
            np.testing.assert_array_equal(r.sums[c, :, s], want, err_msg=f'{name} clip {c} {src}')
    assert r.sums[..., 4].sum() > 0 and r.sums[:, :, 1, :, 2].sum() > 0 and nfp.model.static_shapes is False
    sc = nfp.score(loader, clim, threshold=thr, **extra)
    assert sc.sources == r.sources
    hits, over, under = sc.sums[..., 4], sc.sums[..., 5], sc.sums[..., 6]
    one = r.sums[:, :, :, 0]
    np.testing.assert_array_equal(one[..., 0], sc.sums[..., 0])
    np.testing.assert_array_equal(one[..., 2], over + under)
    np.testing.assert_array_equal(one[..., 3], hits + over)
    np.testing.assert_array_equal(one[..., 4], hits + under)
    np.testing.assert_array_equal(one[..., 1], one[..., 4])
    lead = r.by_lead('model')
    assert lead['fss'].shape == (T, 6) and r.skill().shape == (T, 6) and lead['useful_scale'].shape == (T,)


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise'])
def test_graphed_fss_equals_eager_bit_for_bit(name):
    """cheb_quadtree: batches of 2, 2 and 1 clips (two captured shapes, one replay); transformer_pixelwise: single clips with
    climatology (every clip after the first a replay)."""
    nfp, loader, clim, extra = _config(name)
    nfp.model.eval()
    nfp.model.static_shapes = True
    static = nfp.fss(loader, clim, scales=(1, 5, 33), **extra)
    nfp.model.static_shapes = False
    graphed = nfp.fss(loader, clim, use_graph=True, scales=(1, 5, 33), **extra)
    assert nfp.model.static_shapes is False
    assert graphed.sources == static.sources and len(graphed.sources) == (3 if clim is not None else 2)
    np.testing.assert_array_equal(graphed.sums, static.sums)
    assert graphed.sums[..., 0].sum() > 0 and graphed.sums[..., 2].sum() > 0
    again = nfp.fss(loader, clim, use_graph=True, scales=(1, 5, 33), **extra)
    np.testing.assert_array_equal(again.sums, graphed.sums)


def test_fss_refuses_by_name(monkeypatch):
    from qtmpnn import _lib, ops
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    ok = ops.rollout_fss(y_hat, meshes, y)
    assert ok.shape == (len(y_hat), x.shape[0], 1, 6, 5) and ok.dtype == torch.int64
    # from here on nothing may be launched
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    for bad, why in (((1, 2), 'must be odd'), ((3, 1), 'strictly increasing'), ((), 'empty'), ((1, 35), 'in 1..33'),
                     ((1.0, 3), 'integers'), (tuple(range(1, 19, 2)), 'at most 8')):
        with pytest.raises(ValueError, match=f'rollout_fss: .*{why}'):
            ops.rollout_fss(y_hat, meshes, y, scales=bad)
        with pytest.raises(ValueError, match=f'fss: .*{why}'):
            nfp.fss(loader, clim, scales=bad)
        with pytest.raises(ValueError, match=f'make_graphed_fss: .*{why}'):
            nfp.make_graphed_fss(x, y, scales=bad)
    with pytest.raises(ValueError, match='rollout_fss: y has'):
        ops.rollout_fss(y_hat, meshes, y[:, :2])
    with pytest.raises(ValueError, match='rollout_fss: persistence has'):
        ops.rollout_fss(y_hat, meshes, y, persistence=x[0, -1, :, :, 0])
    with pytest.raises(ValueError, match='rollout_fss: outputs must be fp32'):
        ops.rollout_fss([o.cpu() for o in y_hat], meshes, y)
    with pytest.raises(ValueError, match='rollout_fss: 3 output steps for'):
        ops.rollout_fss(y_hat[:3], meshes, y)
    assert launched == [] and nfp.model.static_shapes is False
