"""Host checks of tests/mesh_model.py, the model that tests/test_gpu_mesh_oracle.py holds the on-device quadtree build to.

  * the model reproduces the labels and pixel counts of every graph_*.npz golden and the KAT labels;
  * its positional features are O.flatten of O.positional_encoding;
  * every case of the table has the property it is there for, the unflagged local walk equals the oracle on it, and every hazard
    flag of mesh_model.HAZARDS changes the labels of the cases designated for it -- a flag that no case detects is a hole in the
    table;
  * frames with more base rows than base columns are refused with IndexError.
"""
import glob
import os

import numpy as np
import pytest
import torch

import mesh_model as M
from oracle import qt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
UNIQUE = list({c.key: c for c in M.cases()}.values())          # the two stage-1 variants of a max_size 64 case share a model


def _criterion(c):
    pad = lambda a: np.pad(a, ((0, M.cdiv(c.n, c.max_size) * c.max_size - c.n), (0, M.cdiv(c.m, c.max_size) * c.max_size - c.m)), mode='edge')
    return [M.dist_from_05(pad(a)) if c.transform else a for a in c.imgs]


def _has_node(md, b, x, y, s):
    cl = md.cell[md.node_off[b]:md.node_off[b + 1]]
    return bool(((cl[:, 0] == x) & (cl[:, 1] == y) & (cl[:, 2] == s)).any())


def _outside_quadrant(c, md):
    ms, h = c.max_size, c.max_size // 2
    return any(not _has_node(md, b, X, Y, ms) and (X + h >= c.n or Y + h >= c.m)
               for b in range(c.B) for X in range(0, c.n, ms) for Y in range(0, c.m, ms))


def _hot_outside(c, md):
    ms = c.max_size
    for b in (2, 3):
        r, col = (int(v[0]) for v in np.nonzero(c.imgs[b]))
        if (r < ms and col < ms) or _has_node(md, b, 0, 0, ms):
            return False
    return True


def _masked_head(c, md):
    s = 2
    while s <= c.max_size:
        for r, col in zip(*np.nonzero(c.mask)):
            if r % s == 0 and col % s == 0 and not c.mask[r:r + s, col:col + s].all():
                return True
        s *= 2
    return False


PROPS = {
    'clipped': lambda c, md: bool(((md.cell[:, 2] > 1) & ((md.cell[:, 0] + md.cell[:, 2] > c.n) | (md.cell[:, 1] + md.cell[:, 2] > c.m))).any()),
    'unsplit_base': lambda c, md: bool((md.cell[:, 2] == c.max_size).any()),
    'level6': lambda c, md: bool((md.level == 6).any()),
    'per_pixel_clip1': lambda c, md: md.node_off[2] - md.node_off[1] == c.n * c.m,
    'per_pixel': lambda c, md: md.N == c.B * c.n * c.m and bool((md.cell[:, 2] == 1).all()),
    'all_base': lambda c, md: md.N == c.B * md.nbase and bool((md.cell[:, 2] == c.max_size).all()),
    'tie': lambda c, md: any(bool((a == np.float32(c.thresh)).any()) for a in _criterion(c)),
    'narrow': lambda c, md: c.n < c.max_size or c.m < c.max_size,
    'sliver': lambda c, md: c.n % c.max_size == 1 or c.m % c.max_size == 1,
    'outside_quadrant': _outside_quadrant,
    'hot_outside_cell00': _hot_outside,
    'mask_extra_only': lambda c, md: (c.mask.sum() == 1 and not c.mask[:c.max_size, :c.max_size].any()
                                      and c.mask[:c.max_size + 1, :c.max_size + 1].any() and not c.imgs[0].any()
                                      and not _has_node(md, 0, 0, 0, c.max_size)),
    'zero_counts': lambda c, md: bool((np.diff(md.cell_off) == 0).any()),
    'masked': lambda c, md: bool(c.mask.any() and (md.labels[:, c.mask] == -1).all() and (md.labels[:, ~c.mask] >= 0).all()),
    'masked_head': _masked_head,
    'hir_only': lambda c, md: bool(c.mask is None and c.hir.any() and (md.level[:, c.hir] == 0).all() and (md.labels >= 0).all()),
    'negative': lambda c, md: bool((c.imgs < 0).any()),
}


# --------------------------------------------------------------------------------------------------- the model and the goldens
@pytest.mark.parametrize('path', sorted(glob.glob(os.path.join(GOLDEN, 'graph_*.npz'))), ids=lambda p: os.path.basename(p)[6:-4])
def test_model_reproduces_the_graph_goldens(path):
    g = np.load(path, allow_pickle=False)
    img0 = g['x'][..., 0].max(axis=0)
    md = M.model_of(img0[None], 64, float(g['thresh']), str(g['condition']), g['mask'] if 'mask' in g.files else None,
                    g['hir'] if 'hir' in g.files else None, M.dist_from_05 if bool(g['has_transform']) else None)
    assert np.array_equal(md.labels[0], g['labels'])
    assert np.array_equal(md.npix, g['npix'])
    assert md.N == len(g['npix']) and md.node_off.tolist() == [0, md.N]


def test_model_reproduces_the_kat_labels():
    k = np.load(os.path.join(GOLDEN, 'kat.npz'), allow_pickle=False)
    for i in (1, 2, 3):
        assert np.array_equal(M.model_of(k[f'kat{i}_img'][None], 4, .5).labels[0], k[f'kat{i}_labels'])
    for cond in O.CONDITIONS:
        md = M.model_of(k['kat6_img'][None], 8, .9 if 'max' in cond else .1, cond)
        assert np.array_equal(md.labels[0], k['kat6_' + cond]), cond
        assert np.array_equal(M.local_walk(k['kat6_img'], .9 if 'max' in cond else .1, 8, condition=cond), k['kat6_' + cond])


def test_return_cells_leaves_the_default_alone():
    c = M.case('grid-50x70-ms16')
    for img in c.imgs:
        plain = O.quadtree_decompose(img, thresh=np.float32(0.5), max_size=16)
        lab, cells = O.quadtree_decompose(img, thresh=np.float32(0.5), max_size=16, return_cells=True)
        assert isinstance(plain, np.ndarray) and np.array_equal(plain, lab)
        assert cells.shape == (lab.max() + 1, 3) and cells.dtype == np.int64
        # label i is the leaf (x, y, s): it owns exactly the square's pixels inside the frame
        for i, (x, y, s) in enumerate(cells):
            assert (lab[x:x + s, y:y + s] == i).all() and (lab == i).sum() == lab[x:x + s, y:y + s].size


@pytest.mark.parametrize('name', ['grid-65x129-ms64', 'grid-50x70-ms8', 'both-80x150-ms16', 'grid-24x32-ms64'])
def test_posfeat_is_flatten_of_the_positional_encoding(name):
    c = M.case(name + '-q1' if name.endswith('ms64') else name)
    md = M.model_for(c)
    pe = torch.from_numpy(O.positional_encoding(c.n, c.m))[None]
    for b in range(c.B):
        lo, hi = md.node_off[b], md.node_off[b + 1]
        lab = np.where(md.labels[b] >= 0, md.labels[b] - lo, -1)
        want = O.flatten(pe, lab, md.npix[lo:hi].astype(np.float64))[0].numpy()
        np.testing.assert_allclose(md.posfeat[lo:hi, :2], want, rtol=1e-13, atol=1e-15)
    assert np.array_equal(md.posfeat[:, 2], md.npix / (c.max_size / 2) ** 2)
    # ... and a clipped cell's mean is that of the pixels it keeps, not of the whole square
    cl = md.cell
    clipped = np.nonzero((cl[:, 1] + cl[:, 2] > c.m))[0]
    if len(clipped):
        i = clipped[0]
        assert md.posfeat[i, 0] * c.m == (cl[i, 1] + c.m - 1) / 2.0 < cl[i, 1] + (cl[i, 2] - 1) / 2.0


# ------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize('c', UNIQUE, ids=lambda c: c.key)
def test_case(c):
    kw = dict(mask=c.mask, hir=c.hir, condition=c.condition, transform=M.dist_from_05 if c.transform else None)
    if c.tall:
        assert M.cdiv(c.n, c.max_size) > M.cdiv(c.m, c.max_size)
        for f in (M.walk, M.local_walk):
            with pytest.raises(IndexError):
                f(c.imgs[0], c.thresh, c.max_size, **kw)
        return
    md = M.model_for(c)
    assert c.B >= 3 and md.B == c.B and md.labels.shape == c.imgs.shape
    for p in c.props:
        assert PROPS[p](c, md), f'{c.name}: property {p} does not hold'
    # consistency of the assembled arrays with one another
    assert md.node_off[0] == 0 and md.node_off[-1] == md.N == len(md.cell) and md.npix.sum() == (md.labels >= 0).sum()
    assert (md.cell[:, 3] == np.repeat(np.arange(c.B), np.diff(md.node_off))).all()
    nbj = M.cdiv(c.m, c.max_size)
    for b in range(c.B):
        for base in range(md.nbase):
            X, Y = base // nbj * c.max_size, base % nbj * c.max_size
            blk = md.labels[b, X:X + c.max_size, Y:Y + c.max_size]
            slot = b * md.nbase + md.nbase - 1 - base
            if (blk >= 0).any():
                assert md.cell_off[slot] == blk[blk >= 0].min() and md.cell_off[slot + 1] == blk.max() + 1
            else:
                assert md.cell_off[slot] == md.cell_off[slot + 1]
    # the unflagged local walk equals the oracle; every designated hazard changes the labels
    local = [M.local_walk(im, c.thresh, c.max_size, **kw) for im in c.imgs]
    for b in range(c.B):
        lab = np.where(md.labels[b] >= 0, md.labels[b] - md.node_off[b], -1)
        assert np.array_equal(local[b], lab), f'{c.name}: the local walk differs from the oracle on clip {b}'
    for hz in c.detects:
        assert any(not np.array_equal(M.local_walk(im, c.thresh, c.max_size, hazard=hz, **kw), local[b])
                   for b, im in enumerate(c.imgs)), f'{c.name} is designated for "{M.HAZARDS[hz]}" and does not detect it'


def test_every_hazard_has_a_designated_case():
    for hz in M.HAZARDS:
        assert any(hz in c.detects and not c.tall for c in M.cases()), f'no case detects: {M.HAZARDS[hz]}'
    # the table names every frame and max_size, and the refusals are the tall base grids
    assert {(c.n, c.m, c.max_size) for c in M.cases()} >= {(n, m, ms) for n, m in M.FRAMES for ms in M.MAX_SIZES}
    assert sorted(c.name for c in M.cases() if c.tall) == [f'grid-64x40-ms{ms}' for ms in (16, 2, 4, 8)]
    for ms in (64,):
        assert {c.quads for c in M.cases() if c.max_size == ms} == {True, False}


def test_remesh_indices_against_a_pixel_loop():
    old = M.model_for(M.case('both-80x150-ms16'))
    c = M.case('both-80x150-ms16')
    rng = np.random.default_rng(3)
    val = rng.choice(np.array([0.0, 0.125, 0.25], np.float32), size=old.N, p=[0.9, 0.07, 0.03])
    crit = M.remesh_criterion(val, old.labels)
    assert crit.dtype == np.float32 and (crit[:, c.mask] == 0).all()
    ok = old.labels >= 0
    assert np.array_equal(crit[ok], val[old.labels[ok]])
    new = M.model_of(crit, 16, 0.125, mask=c.mask, hir=c.hir)
    fwd, bwd = M.remesh_indices(old, new)
    want_f, want_b = np.full(new.N, -1), np.full(old.N, -1)
    for b in range(c.B):
        for r in range(c.n):
            for col in range(c.m):
                lo, ln = old.labels[b, r, col], new.labels[b, r, col]
                if ln >= 0 and new.level[b, r, col] == 0:
                    want_f[ln] = lo
                if lo >= 0 and old.level[b, r, col] == 0:
                    want_b[lo] = ln
    assert np.array_equal(fwd, want_f) and np.array_equal(bwd, want_b)
    assert (fwd >= 0).any() and (fwd == -1).any() and (bwd >= 0).any() and (bwd == -1).any()
