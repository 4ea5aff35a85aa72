"""The six verification products count the same pixels (csrc/verify.hip: PixelReader::counted): a pixel of a step and clip counts
iff its label is a node of that step (0 <= label < the step's node count) and Mesh.loss_mask does not cover it.  One frame on
which every kernel's ragged edge is present at once, hand-made labels, and the counts of rollout_scores, rollout_reliability,
rollout_fss, rollout_score_maps, rollout_edges and rollout_event_dates against the dense mask computed in numpy.  Every number
compared is an integer: exact equality."""
import copy
import functools

import numpy as np
import pytest
import torch

from edges_restated import edge_set, ice
from helpers import dev

pytestmark = pytest.mark.gpu

# 33 x 72, P = 2376: k_score_multi has two full 1024-pixel tiles and a ragged third; k_fss_multi 2 x 3 tiles of 32 x 32 whose
# halos leave the frame on every side; k_edge_planes three bands of 16 rows, the last of one row, and a second 64-bit word of 8
# columns per row.  17 steps: a launch of 16 and a launch of one.
N_, M_, B, T, THR, STALE = 33, 72, 2, 17, 0.5, 3
P = N_ * M_


@functools.lru_cache(maxsize=None)
def _frame():
    """-> (labels (B, P) int32, n_stale, loss_mask (N_, M_) bool, counted (B, T, N_, M_) bool).  Marked pixels sit on both
    sides of every tile, band and word boundary (rows 0, 15 | 16, 31 | 32; columns 0, 31 | 32, 63 | 64, 71; flat pixels
    1023 | 1024 and 2047 | 2048) and at random places; marked pixel i of clip b has label -1 if (i + b) % 5 is 0 or 3, a label
    beyond the node count of step STALE if it is 1 or 4, and loss_mask covers those with odd i: pixels that are only masked,
    holes and stale pixels under the mask, and holes and stale pixels outside it, in both clips."""
    rng = np.random.default_rng(57)
    marked = [r * M_ + c for r in (0, 15, 16, 31, 32) for c in (0, 31, 32, 63, 64, 71)] + [1023, 1024, 2047, 2048]
    marked += [int(p) for p in rng.permutation(P) if p not in marked][:41]
    marked = np.array(marked)
    i = np.arange(len(marked))
    hole, beyond = np.zeros((B, P), bool), np.zeros((B, P), bool)
    for b in range(B):
        hole[b, marked[np.isin((i + b) % 5, (0, 3))]] = True
        beyond[b, marked[np.isin((i + b) % 5, (1, 4))]] = True
    mask = np.zeros(P, bool)
    mask[marked[i % 2 == 1]] = True
    # nodes: the ordinary pixels of both clips in raster order, then the `beyond` ones; holes have none
    labels = np.full((B, P), -1, np.int32)
    plain = ~hole & ~beyond
    labels[plain] = np.arange(plain.sum())
    labels[beyond] = plain.sum() + np.arange(beyond.sum())
    n_stale = int(plain.sum())
    counted = np.repeat((labels >= 0)[:, None], T, axis=1)
    counted[:, STALE] &= labels < n_stale
    counted &= ~mask
    for kind in (hole & mask, hole & ~mask, beyond & mask, beyond & ~mask, plain & mask):
        assert kind[0].any() and kind[1].any()
    assert labels.max() + 1 < B * P and not np.array_equal(counted[0], counted[1])
    return labels, n_stale, mask.reshape(N_, M_), counted.reshape(B, T, N_, M_)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.mark.parametrize('S', [1, 3])
def test_six_products_count_the_same_pixels(S):
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    labels, n_stale, mask, counted = _frame()
    rng = np.random.default_rng(58)
    fields = [rng.random((B, T, N_, M_), dtype=np.float32) for _ in range(3)]
    fields[1] = np.repeat(fields[1][:, :1], T, axis=1)               # persistence: one frame for every lead time
    y = rng.random((B, T, N_, M_), dtype=np.float32)
    launch = rng.random((B, N_, M_), dtype=np.float32)
    mesh = copy.copy(build_pixel_mesh(B, N_, M_, None, dev()))
    mesh.labels = _t(labels.reshape(B, N_, M_))
    mesh.loss_mask = _t(mask.astype(np.uint8))
    stale = copy.copy(mesh)
    stale.n_dev = torch.tensor([n_stale], dtype=torch.int32, device=dev())
    meshes = [mesh] * T
    meshes[STALE] = stale
    outs, node = [], labels >= 0
    for z in range(T):
        o = torch.full((B * P, 4), 0.87, device=dev())        # B * P rows: N is larger than every label and than n_stale
        o[_t(labels[node].astype(np.int64)), 0] = _t(fields[0][:, z].reshape(B, P)[node])
        outs.append(o)
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2])) if S == 3 else {}
    n = counted.sum(axis=(2, 3)).T                                   # (T, B)
    assert len(set(n.reshape(-1).tolist())) >= 3 and (n[STALE] < n[0]).all()
    want = np.repeat(n[:, :, None], S, axis=2)                       # (T, B, S)

    scores = ops.rollout_scores(outs, meshes, _t(y), THR, **kw).cpu().numpy()
    np.testing.assert_array_equal(scores[..., 0], want, err_msg='rollout_scores: n')
    rel = ops.rollout_reliability(outs, meshes, _t(y), THR, 10, **kw).cpu().numpy()
    np.testing.assert_array_equal(rel[..., 0].sum(axis=-1), want, err_msg='rollout_reliability: bin totals')
    fss = ops.rollout_fss(outs, meshes, _t(y), THR, (1, 5, 33), **kw).cpu().numpy()
    np.testing.assert_array_equal(fss[..., 0], np.repeat(want[..., None], 3, axis=3), err_msg='rollout_fss: n')
    maps = torch.zeros(T, S, 8, P, dtype=torch.float64, device=dev())
    maps = ops.rollout_score_maps(outs, meshes, _t(y), maps, THR, **kw).cpu().numpy()
    per_pixel = counted.sum(axis=0).reshape(T, 1, P)                 # the maps are summed over the clips
    np.testing.assert_array_equal(maps[:, :, 0], np.repeat(per_pixel, S, axis=1), err_msg='rollout_score_maps: n per pixel')
    np.testing.assert_array_equal(maps[:, :, 0].sum(axis=-1), want.sum(axis=1), err_msg='rollout_score_maps: n')

    # an uncounted pixel is no ice and no open water: the sizes of the edge sets are those of the dense mask's
    edges = ops.rollout_edges(outs, meshes, _t(y), THR, **kw).cpu().numpy()
    for z in range(T):
        for b in range(B):
            c = counted[b, z]
            n_o = edge_set(ice(y[b, z], c, THR), c).sum()
            sizes = [[edge_set(ice(fields[s][b, z], c, THR), c).sum(), n_o] for s in range(S)]
            assert edges[z, b, :, :2].tolist() == sizes, ('rollout_edges: |E(f)|, |E(y)|', z, b)

    ekw = dict(climatology=kw['climatology']) if S == 3 else {}
    dates, sums = ops.rollout_event_dates(outs, meshes, _t(y), _t(launch), THR, 'breakup', 2, **ekw)
    dates = dates.cpu().numpy().reshape(B, -1, N_, M_)
    dead = ~counted.all(axis=1)                                      # uncounted at any step
    assert dates.shape[1] == (3 if S == 3 else 2) and dead.sum() > mask.sum() * B
    for s in range(dates.shape[1]):
        np.testing.assert_array_equal(dates[:, s] == -2, dead, err_msg=f'rollout_event_dates: -2 of source {s}')
    np.testing.assert_array_equal(sums.cpu().numpy()[..., 0], np.repeat((~dead).sum(axis=(1, 2))[:, None], dates.shape[1] - 1, 1))
