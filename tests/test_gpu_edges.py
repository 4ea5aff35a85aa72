"""edge_distance(): ice-edge verification on the GPU (qt_edge_rollout, ops.rollout_edges, NextFramePredictorS2S.edge_distance)
against the brute-force restatement of tests/edges_restated.py.  Everything is an integer, so every comparison is exact equality.
At the op level the restatement is fed the hand-made node values themselves; through edge_distance() it is fed the project's own
eager predict() frames of the same model and inputs, so both sides threshold identical fp32 forecasts."""
import copy
import functools

import numpy as np
import pytest
import torch

from edges_restated import edge_set, ice, restated_edges
from helpers import dev
from test_gpu_fss import RAGGED, SMALL, THR, _blobs, _fields_for, _land_mask, _outs, _reference, _t
from test_gpu_predict_graph import _config
from test_gpu_score import _case, _clips

pytestmark = pytest.mark.gpu


def _want(fields, y, mask, S, counted=None):
    """(T, B, S, 8) int64 from the restatement."""
    B, T = y.shape[:2]
    want = np.zeros((T, B, S, 8), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            want[:, b, s] = restated_edges(fields[s][b], y[b], mask, THR, None if counted is None else counted[b])
    return want


def _total(tiles):
    """The bands' int32 partials (T, B, bands, S, 8) -> the int64 totals: slots 0-5 added, slots 6-7 maximised."""
    return torch.cat([tiles[..., :6].sum(2, dtype=torch.int64), tiles[..., 6:].amax(2).to(torch.int64)], dim=-1)


def _run(outs, meshes, y, S, fields):
    """rollout_edges with S sources -> (totals, per-band partials), after the checks every case shares."""
    from qtmpnn import ops
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2])) if S == 3 else {}
    got = ops.rollout_edges(outs, meshes, _t(y), THR, **kw)
    tiles = ops.rollout_edges(outs, meshes, _t(y), THR, per_tile=True, **kw)
    T, B, n = len(outs), meshes[0].B, meshes[0].n
    assert got.shape == (T, B, S, 8) and got.dtype == torch.int64 and got.is_cuda and not got.requires_grad
    assert tiles.shape == (T, B, -(n // -16), S, 8) and tiles.dtype == torch.int32
    assert torch.equal(got, _total(tiles))
    assert torch.equal(got, ops.rollout_edges(outs, meshes, _t(y), THR, **kw))
    return got.cpu().numpy(), tiles.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _small_table():
    fields, y = _fields_for(SMALL, 2, 17, 31)
    return fields, y, _want(fields, y, None, 3)


@pytest.mark.parametrize('S', [1, 3])
def test_op_edge_values_over_two_launches(S):
    """Hand-made (N, 4) outputs on a 24 x 32 pixelwise mesh, B = 2, 17 steps: a launch of 16 and a launch of 1 into one buffer.
    Column 0 carries the values (a decoy above THR elsewhere); with S = 3 persistence is a B*P frame and climatology a B*T*P
    field."""
    from qtmpnn.mesh import build_pixel_mesh
    fields, y, want = _small_table()
    want = want[:, :, :S]
    B, T = 2, 17
    for f in fields + [y]:                                   # every special value is there, on both sides of the comparison
        assert np.isnan(f).any() and np.isinf(f).any() and (f == np.float32(THR)).any()
    assert (want[..., :2] > 0).all() and (want[..., 2:] > 0).all()
    mesh = build_pixel_mesh(B, *SMALL, None, dev())
    got, tiles = _run(_outs(fields[0], fill=0.87), [mesh] * T, y, S, fields)
    np.testing.assert_array_equal(got, want)
    assert tiles.shape[2] == 2 and (tiles[:, :, :, :, :2].sum(axis=2) == want[..., :2]).all()


@functools.lru_cache(maxsize=None)
def _ragged_table():
    """40 x 72 (two 64-bit words per row, the second 8 columns wide; bands of 16, 16 and 8 rows), B = 2, T = 2: blobs, then ice
    planted at the word boundary -- columns 63 and 64 in the truth, columns 60-62 and 65-67 on either side of it in the model --
    and in the last row and the last column."""
    fields, y = _fields_for(RAGGED, 2, 2, 32)
    for f in fields + [y]:
        f[..., 8:14, 56:72] = 0.1                            # open water around the planted ice
    y[..., 10:12, 63:65] = 0.9
    fields[0][..., 10:12, 60:63] = 0.9
    fields[0][..., 10:12, 65:68] = 0.9
    y[..., 36:40, 18:32] = y[..., 18:32, 68:72] = 0.1
    y[..., 39, 20:30] = 0.9                                  # the last row
    y[..., 20:30, 71] = 0.9                                  # the last column
    fields[0][..., 35:40, 38:52] = fields[0][..., 0:8, 66:72] = 0.1
    fields[0][..., 38:40, 40:50] = 0.9
    fields[0][..., 0:6, 70:72] = 0.9
    return fields, y


def test_word_boundary_ragged_bands_and_last_row_and_column():
    from qtmpnn.mesh import build_pixel_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    keep = np.ones(RAGGED, bool)
    ey, ef = edge_set(ice(y[0, 0], keep, THR), keep), edge_set(ice(fields[0][0, 0], keep, THR), keep)
    assert ey[10, 63] and ey[10, 64] and ef[10, 62] and ef[10, 65] and not ef[10, 63] and not ef[10, 64]
    assert ey[39, 25] and ey[25, 71] and ef[39, 40] and ef[38, 45] and not ef[39, 45] and ef[3, 70] and ef[5, 71] and not ef[3, 71]
    want = _want(fields, y, None, 3)
    mesh = build_pixel_mesh(B, *RAGGED, None, dev())
    got, tiles = _run(_outs(fields[0], fill=0.87), [mesh] * T, y, 3, fields)
    np.testing.assert_array_equal(got, want)
    # a band's own counts: rows 32-39, the ragged last band
    assert tiles.shape[2] == 3
    assert tiles[0, 0, 2, 0, 0] == ef[32:].sum() > 0 and tiles[0, 0, 2, 0, 1] == ey[32:].sum() > 0


@pytest.mark.parametrize('shape', [(8, 256), (256, 8)])
def test_one_edge_pixel_near_each_end(shape):
    """The widest and the tallest frame taken, B = 1, T = 1: the truth's only ice is a pixel one step inside one corner, the
    model's one step inside the opposite corner, so each search crosses every word of a row or every row of the frame, and the
    max slots hold the largest distance the frame has room for.  Persistence has ice at both ends; climatology has none."""
    from qtmpnn.mesh import build_pixel_mesh
    n, m = shape
    y = np.full((1, 1, n, m), 0.1, np.float32)
    fields = [y.copy(), y.copy(), y.copy()]
    y[..., 1, 1] = 0.9
    fields[0][..., n - 2, m - 2] = 0.9
    fields[1][..., 1, 1] = fields[1][..., n - 2, m - 2] = 0.9
    want = _want(fields, y, None, 3)
    d2 = (n - 3) ** 2 + (m - 3) ** 2
    assert want[0, 0, 0].tolist()[:2] == [1, 1] and want[0, 0, 0].tolist()[4:] == [d2, d2, d2, d2]
    assert want[0, 0, 1].tolist()[:2] == [2, 1] and want[0, 0, 1].tolist()[4:] == [d2, 0, d2, 0]
    assert want[0, 0, 2].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    mesh = build_pixel_mesh(1, n, m, None, dev())
    got, _ = _run(_outs(fields[0], fill=0.87), [mesh], y, 3, fields)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('how', ['loss_mask', 'labels'])
def test_uncounted_pixels_under_a_mask(how):
    """The ragged frame with a mask, carried by Mesh.loss_mask (the labels know nothing of it) or by the labels (-1 under the
    mask, fewer nodes than pixels: node order is raster order over the kept pixels).  Uncounted pixels neither form nor block
    edges."""
    from qtmpnn.mesh import build_pixel_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    mask = _land_mask()
    keep = ~mask
    # the mask matters: without it some ice pixel next to a masked pixel would (or would not) be an edge
    assert (edge_set(ice(y[0, 0], keep, THR), keep) != edge_set(ice(y[0, 0], keep | True, THR), keep | True))[keep].any()
    want = _want(fields, y, mask, 3)
    if how == 'loss_mask':
        mesh = copy.copy(build_pixel_mesh(B, *RAGGED, None, dev()))
        mesh.loss_mask = _t(mask.astype(np.uint8))
        outs = _outs(fields[0], fill=0.87)
    else:
        mesh = build_pixel_mesh(B, *RAGGED, mask, dev())
        assert mesh.loss_mask is None and mesh.N == B * keep.sum() and (mesh.labels.cpu().numpy()[:, mask] == -1).all()
        outs = _outs(fields[0][:, :, keep], fill=0.87)
    got, tiles = _run(outs, [mesh] * T, y, 3, fields)
    np.testing.assert_array_equal(got, want)
    assert (want[..., :2] > 0).all()


def test_quadtree_labels_on_a_static_capacity_mesh_with_stale_labels():
    """A quadtree mesh built with a mask in static mode: labels -1 under the mask, several pixels per node, N is the capacity
    and the node count is on the device.  The output buffers hold ice in every row beyond the nodes; at step 1 the node count
    the kernel is given is 40 short, so the pixels of the last 40 nodes are uncounted there too."""
    from qtmpnn.mesh import build_mesh
    fields, y = _ragged_table()
    B, T = 2, 2
    mask = _land_mask()
    crit = _blobs(np.random.default_rng(24), B, 1, RAGGED)[:, 0]
    crit = np.where(crit > 0.5, crit, np.float32(0))
    mesh = build_mesh(src=_t(crit), thresh=0.1, mask=mask, static=True)
    labels = mesh.labels.cpu().numpy().reshape(B, *RAGGED)
    N = mesh.n_valid
    assert mesh.N == B * RAGGED[0] * RAGGED[1] and 40 < N < mesh.N and (labels[:, mask] == -1).all()
    stale = copy.copy(mesh)
    stale.n_dev = torch.tensor([N - 40], dtype=torch.int32, device=dev())
    rng = np.random.default_rng(35)
    node = (0.2 + 0.6 * rng.random((T, N))).astype(np.float32)
    node[:, rng.permutation(N)[:4]] = np.array([THR, np.nan, np.inf, np.nextafter(np.float32(THR), np.float32(1))], np.float32)
    outs = []
    for z in range(T):
        o = torch.full((mesh.N, 4), 0.87, device=dev())      # capacity rows and the other columns: ice, if they were read
        o[:N, 0] = _t(node[z])
        outs.append(o)
    counted = np.stack([labels >= 0, (labels >= 0) & (labels < N - 40)], axis=1)            # (B, T, n, m)
    assert counted[:, 0].sum() > counted[:, 1].sum() > 0
    model = np.where(counted, node[np.arange(T)[None, :, None, None], np.maximum(labels, 0)[:, None]], np.float32(0.87))
    fields = [model.astype(np.float32), fields[1], fields[2]]
    want = _want(fields, y, None, 3, counted)
    got, _ = _run(outs, [mesh, stale], y, 3, fields)
    np.testing.assert_array_equal(got, want)
    assert (want[:, :, :, :2] > 0).all() and (want[0] != want[1]).any()


def test_a_source_without_ice_and_an_all_ice_truth():
    """Step 0: the model has no ice at all; step 1: the truth is all ice (no edge); step 2: both have edges.  The slots of a
    direction without a target are 0, the counts are not."""
    from qtmpnn.mesh import build_pixel_mesh
    fields, y = _fields_for(SMALL, 1, 3, 36)
    fields, y = [f.copy() for f in fields], y.copy()
    fields[0][:, 0] = 0.1
    y[:, 1] = 0.9
    want = _want(fields, y, None, 3)
    assert want[0, 0, 0].tolist()[0] == 0 and want[0, 0, 0, 1] > 0 and want[0, 0, 0, 2:].tolist() == [0] * 6
    assert (want[1, 0, :, 1] == 0).all() and (want[1, 0, :, 0] > 0).all() and (want[1, 0, :, 2:] == 0).all()
    assert (want[2] > 0).all() and (want[0, 0, 1:, 2:] > 0).all()
    mesh = build_pixel_mesh(1, *SMALL, None, dev())
    got, _ = _run(_outs(fields[0], fill=0.87), [mesh] * 3, y, 3, fields)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('name', ['cheb_quadtree', 'quadtree_masked_64', 'transformer_pixelwise'])
def test_edge_distance_equals_restatement(name):
    """Re-meshing quadtree rollouts on 64 x 64 clips in batches of 2, 2 and 1 (the second with a mask), and a 24 x 32 pixelwise
    one with a mask and climatology: the sums are the restatement's on eager predict()'s frames."""
    from qtmpnn.edges import EdgeDistance
    thr = 0.15
    nfp, loader, clim, extra, fields = _reference(name)
    r = nfp.edge_distance(loader, clim, threshold=thr, **extra)
    assert isinstance(r, EdgeDistance) and r.threshold == thr
    assert r.sources == ('model', 'persistence') + (('climatology',) if clim is not None else ()) == tuple(fields[0])
    clips = _clips(loader)
    T = fields[0]['model'].shape[0]
    assert r.sums.shape == (len(clips), T, len(r.sources), 8) and r.sums.dtype == np.int64
    mask = extra.get('mask')
    for c, (x, y, launch) in enumerate(clips):
        for s, src in enumerate(r.sources):
            want = restated_edges(fields[c][src].astype(np.float32), y.astype(np.float32), mask, thr)
            print(name, 'clip', c, src, 'n_f', want[:, 0].tolist(), 'n_o', want[:, 1].tolist())
            np.testing.assert_array_equal(r.sums[c, :, s], want, err_msg=f'{name} clip {c} {src}')
    assert nfp.model.static_shapes is False
    assert (r.sums[:, :, 1, :2] > 0).all() and (r.sums[:, :, 0, 0] > 0).any() and r.sums[:, :, 0, 2:].sum() > 0
    lead = r.by_lead('model', pixel_km=25.0)
    assert lead['displacement'].shape == (T,) and r.skill().shape == (T,) and r.displacement('persistence').shape == (len(clips), T)


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise'])
def test_graphed_edge_distance_equals_eager_bit_for_bit(name):
    """cheb_quadtree: batches of 2, 2 and 1 clips (two captured shapes, one replay); transformer_pixelwise: single clips with
    climatology (every clip after the first a replay)."""
    nfp, loader, clim, extra = _config(name)
    nfp.model.eval()
    nfp.model.static_shapes = True
    static = nfp.edge_distance(loader, clim, **extra)
    nfp.model.static_shapes = False
    graphed = nfp.edge_distance(loader, clim, use_graph=True, **extra)
    assert nfp.model.static_shapes is False
    assert graphed.sources == static.sources and len(graphed.sources) == (3 if clim is not None else 2)
    np.testing.assert_array_equal(graphed.sums, static.sums)
    again = nfp.edge_distance(loader, clim, use_graph=True, **extra)
    np.testing.assert_array_equal(again.sums, graphed.sums)


def test_edges_refuse_by_name(monkeypatch):
    from qtmpnn import _lib, ops
    from qtmpnn.mesh import build_pixel_mesh
    nfp, loader, clim, extra = _case('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    ok = ops.rollout_edges(y_hat, meshes, y)
    assert ok.shape == (len(y_hat), x.shape[0], 1, 8) and ok.dtype == torch.int64
    big = build_pixel_mesh(1, 8, 264, None, dev())
    # through the method and the captured twin the rollout runs first; the op then refuses the batch under its own name
    with pytest.raises(ValueError, match='rollout_edges: y has'):
        nfp.edge_distance([(loader[0][0], loader[0][1][:, :2], loader[0][2])], clim, **extra)
    assert nfp.model.static_shapes is False
    with pytest.raises(ValueError, match='rollout_edges: y has'):
        nfp.make_graphed_edges(x, y[:, :2], **extra)
    nfp.model.static_shapes = False
    # from here on nothing may be launched
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    with pytest.raises(ValueError, match='rollout_edges: y has'):
        ops.rollout_edges(y_hat, meshes, y[:, :2])
    with pytest.raises(ValueError, match='rollout_edges: persistence has'):
        ops.rollout_edges(y_hat, meshes, y, persistence=x[0, -1, :, :, 0])
    with pytest.raises(ValueError, match='rollout_edges: outputs must be fp32'):
        ops.rollout_edges([o.cpu() for o in y_hat], meshes, y)
    with pytest.raises(ValueError, match='rollout_edges: 3 output steps for'):
        ops.rollout_edges(y_hat[:3], meshes, y)
    with pytest.raises(ValueError, match='rollout_edges: a frame of 8 x 264 pixels is larger than 256 x 256'):
        ops.rollout_edges([torch.zeros(8 * 264, 1, device=dev())], [big], torch.zeros(8 * 264, device=dev()))
    assert launched == []
