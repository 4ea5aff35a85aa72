"""Host checks of the float64 Laplacian / Chebyshev model (tests/cheb_f64.py) on its own: its adjacency is the oracle's, its
distances are the reference's recorded edge attributes, its operator equals both oracle ChebConv restatements, its adjoint is the
transpose of its forward -- and the bound the GPU tests use is sharp enough to see one wrong edge, one wrong centroid or one
entry of L^ off by 2^-10.  No GPU, nothing of qtmpnn."""
import glob
import os

import numpy as np
import pytest
import torch

import cheb_f64 as M
from helpers import GOLDEN

GRAPHS = sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(GOLDEN, 'graph_*.npz')))


def hand_map():
    """16 x 24: an 8 x 8 cell, four 4 x 4 cells, sixteen 2 x 2 cells, an 8 x 8 block of single pixels with masked ones among them --
    pixel (10, 10) has all four neighbours masked: a node without an edge --, and a 16 x 16 cell at column 16 that the image border
    clips to 8 columns.  Returns (labels (16, 24), row of the isolated node, row of the clipped cell)."""
    lab = -np.ones((16, 24), np.int64)
    nxt = [0]

    def cell(r, c, z):
        lab[r:r + z, c:c + z] = nxt[0]
        nxt[0] += 1
        return nxt[0] - 1
    cell(0, 0, 8)
    for r in (0, 4):
        for c in (8, 12):
            cell(r, c, 4)
    for r in range(8, 16, 2):
        for c in range(0, 8, 2):
            cell(r, c, 2)
    masked = {(9, 10), (11, 10), (10, 9), (10, 11), (14, 13), (14, 14)}
    lone = None
    for r in range(8, 16):
        for c in range(8, 16):
            if (r, c) not in masked:
                k = cell(r, c, 1)
                if (r, c) == (10, 10):
                    lone = k
    clipped = cell(0, 16, 16)
    return lab, lone, clipped


def _maps():
    """name -> labels (B, n, m): the nine recorded graphs, the hand map (alone and as two clips), and oracle decompositions."""
    from oracle import qt_oracle as O
    out = {}
    for name in GRAPHS:
        out[name] = np.load(os.path.join(GOLDEN, f'graph_{name}.npz'), allow_pickle=False)['labels'][None].astype(np.int64)
    lab, _, _ = hand_map()
    out['hand'] = lab[None]
    second = np.where(lab[::-1, ::-1] >= 0, lab[::-1, ::-1] + lab.max() + 1, -1)
    out['hand_x2'] = np.stack([lab, second])
    rng = np.random.default_rng(3)
    img = np.zeros((50, 70))
    img[11:19, 40:52] = rng.random((8, 12))
    img[44:50, 3:9] = 1.0
    out['quadtree50x70'] = O.quadtree_decompose(img, thresh=0.1, max_size=64)[None]
    mask = np.zeros((40, 56), bool)
    mask[0:17, 0:20] = True
    mask[30:34, 40:56] = True
    out['static40x56'] = np.asarray(O.static_graph((40, 56), 16, mask, use_edge_attrs=False)['labels'])[None]
    out['homog40x56'] = np.asarray(O.static_graph((40, 56), 16, mask, use_edge_attrs=False, homogeneous=True)['labels'])[None]
    pm = np.zeros((12, 20), bool)
    pm[3:6, 4:15] = True
    pm[0, 0] = pm[11, 1] = pm[10, 0] = True                      # (pixel (11, 0) loses both neighbours)
    out['pixel12x20'] = np.asarray(O.pixel_graph(torch.zeros(1, 12, 20, 3), pm, use_edge_attrs=False)['labels'])[None]
    return out


MAPS = _maps()


def draw(rng, *shape):
    """sign * (0.5 + U[0, 1)): no term is small against its neighbours."""
    return rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))


def unclipped_centroids(labels, L, resolution=0.25):
    """(xy with the centroid of every border-clipped cell moved to that of the whole square, rows of those cells).  A clipped
    cell: its pixels fill a rectangle h x w, h != w, that ends at the bottom or right image border; the square has side max(h, w)
    rounded up to a power of two."""
    lab = np.asarray(labels)
    B, n, m = lab.shape
    xy = L.xy.copy()
    ok = lab >= 0
    _, rr, cc = np.meshgrid(np.arange(B), np.arange(n), np.arange(m), indexing='ij')
    big = np.iinfo(np.int64).max
    r0, c0 = np.full(L.N, big), np.full(L.N, big)
    r1, c1 = np.full(L.N, -1), np.full(L.N, -1)
    np.minimum.at(r0, lab[ok], rr[ok])
    np.minimum.at(c0, lab[ok], cc[ok])
    np.maximum.at(r1, lab[ok], rr[ok])
    np.maximum.at(c1, lab[ok], cc[ok])
    cnt = np.bincount(lab[ok], minlength=L.N)
    h, w = r1 - r0 + 1, c1 - c0 + 1
    clipped = (cnt > 0) & (cnt == h * w) & (h != w) & (((r1 == n - 1) & (h < w)) | ((c1 == m - 1) & (w < h)))
    rows = np.nonzero(clipped)[0]
    z = 2.0 ** np.ceil(np.log2(np.maximum(h[rows], w[rows])))
    xy[rows, 0] = (c0[rows] + 0.5 * (z - 1)) * resolution
    xy[rows, 1] = (r0[rows] + 0.5 * (z - 1)) * resolution
    return xy, rows


def test_hand_map_has_a_clipped_cell_and_a_node_without_an_edge():
    lab, lone, clipped = hand_map()
    L = M.laplacian(lab[None])
    assert L.rowlen[lone] == 0 and L.dis[lone] == 0 and L.deg[lone] == 0
    assert (lab == clipped).sum() == 16 * 8 and (lab[:, 16:] == clipped).all()
    assert np.allclose(L.xy[clipped], [19.5 * 0.25, 7.5 * 0.25])
    xy, rows = unclipped_centroids(lab[None], L)
    assert rows.tolist() == [clipped] and np.allclose(xy[clipped], [23.5 * 0.25, 7.5 * 0.25])
    # no edge joins the two clips of the doubled map
    L2 = M.laplacian(MAPS['hand_x2'])
    assert L2.N == 2 * L.N and L2.E == 2 * L.E and ((L2.row < L.N) == (L2.col < L.N)).all()


def test_clipped_cells_exist_in_recorded_graphs_too():
    have = [name for name in GRAPHS if len(unclipped_centroids(MAPS[name], M.laplacian(MAPS[name]))[1])]
    assert have, 'no recorded graph holds a cell clipped by the image border'


@pytest.mark.parametrize('name', sorted(MAPS))
def test_adjacency_equals_the_oracle(name):
    from oracle import qt_oracle as O
    lab = MAPS[name]
    L = M.laplacian(lab)
    want = set()
    for b in range(lab.shape[0]):
        e = O.adjacency_sorted(lab[b])
        want |= {(int(i), int(j)) for i, j in zip(e[0], e[1]) if i != j}
    assert L.neighbours() == want and len(want) == L.E
    rev = set((j, i) for i, j in want)
    assert rev == want                                            # every pair both ways


@pytest.mark.parametrize('name', GRAPHS)
def test_distances_equal_the_recorded_edge_attributes(name):
    """The recorded `attrs` are the reference's float32 distances (column 1 where it also recorded angles).  Its coordinates are
    float32 means of npix positional-encoding terms scaled twice: (npix + 3) roundings of a value <= X = max(n, m) * 0.25 each,
    two nodes per edge and two axes (sqrt 2), then two squares, an add and a square root on the distance (4): the golden lies
    within sqrt 2 ((npix_i + 3) + (npix_j + 3)) U X + 4 U w of the model."""
    g = np.load(os.path.join(GOLDEN, f'graph_{name}.npz'), allow_pickle=False)
    lab = MAPS[name]
    L = M.laplacian(lab)
    e = g['edges'].astype(np.int64)
    keep = e[0] != e[1]
    assert np.array_equal(e[0][keep], L.row) and np.array_equal(e[1][keep], L.col)       # both in (row, col) order
    attrs = g['attrs'].astype(np.float64)
    d = (attrs[:, 1] if attrs.ndim == 2 else attrs)[keep]
    assert ((attrs[:, 1] if attrs.ndim == 2 else attrs)[~keep] == 0).all()
    npix = g['npix'].astype(np.float64)
    X = max(lab.shape[1:]) * 0.25
    tol = np.sqrt(2.0) * (npix[L.row] + npix[L.col] + 6.0) * M.U * X + 4.0 * M.U * L.w
    assert (np.abs(d - L.w) <= tol).all(), float((np.abs(d - L.w) / tol).max())


def _oracle_graph(lab2d):
    """The oracle's own graph of one clip in float64: its edge set, its flatten of the positional encoding, its distances."""
    from oracle import qt_oracle as O
    n, m = lab2d.shape
    N = int(lab2d.max()) + 1
    cnt = np.maximum(np.bincount(lab2d[lab2d >= 0], minlength=N), 1).astype(np.float64)
    pe = torch.from_numpy(O.positional_encoding(n, m))[None]
    pos = O.flatten(pe, lab2d, cnt)[0]
    xx, yy = pos[:, 0] * m * 0.25, pos[:, 1] * n * 0.25
    ei = torch.as_tensor(O.adjacency_sorted(lab2d))
    return ei, O.edge_dist(ei[0], ei[1], xx, yy), N


@pytest.mark.parametrize('name', sorted(n for n in MAPS if MAPS[n].shape[0] == 1))
def test_operator_equals_both_oracle_chebconvs(name):
    """K = 3, weights that copy T_k into the k-th block of output columns, no bias: the oracle's output IS [T_0 | T_1 | T_2]."""
    from oracle import qt_oracle as O
    lab = MAPS[name][0]
    L = M.laplacian(lab[None])
    ei, d, N = _oracle_graph(lab)
    assert N == L.N
    C, K = 3, 3
    x = draw(np.random.default_rng(5), N, C)
    T, A = M.planes(L, x, K)
    want = np.concatenate(list(T), axis=1)
    scale = np.concatenate(list(A), axis=1).max()
    Ws = []
    for k in range(K):
        W = torch.zeros(K * C, C, dtype=torch.float64)
        W[k * C:(k + 1) * C] = torch.eye(C, dtype=torch.float64)
        Ws.append(W)
    got = O.cheb_conv(torch.from_numpy(x), ei, d, Ws, None).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(scale, 1.0)
    if N <= 2500:                                                  # (the dense form holds an N x N matrix)
        got = O.cheb_conv_dense(torch.from_numpy(x), ei, d, Ws, None).numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(scale, 1.0)
    v, a = M.axpby(L, x, 2.0, T[1], -1.0, T[0], 0.5)
    assert np.abs(v - (2.0 * M.apply(L, x)[0] - T[1] + 0.5 * T[0])).max() <= 1e-12 * a.max()
    o, _ = M.ones(L, 3)
    T1, _ = M.planes(L, np.ones((N, 1)), 3)
    assert np.array_equal(o, T1[:, :, 0].T)


def test_dense_oracle_ran_on_some_map():
    assert any(MAPS[n].shape[0] == 1 and M.laplacian(MAPS[n]).N <= 2500 for n in MAPS)


@pytest.mark.parametrize('name', ['hand_x2', '64_1blob_clean', 'homog40x56'])
def test_clenshaw_is_the_transpose_of_planes(name):
    """<G, planes(Z)> = <clenshaw(G), Z>, also for an operator whose entries are NOT symmetric (the transpose is then another
    matrix, and the model must use it)."""
    L = M.laplacian(MAPS[name])
    rng = np.random.default_rng(7)
    for Lx in (L, L.with_val(L.val * (1.0 + 0.3 * rng.random(L.E)))):
        for K in (2, 3, 5):
            Z, G = draw(rng, L.N, 4), draw(rng, K, L.N, 4)
            lhs = float((G * M.planes(Lx, Z, K)[0]).sum())
            rhs = float((M.clenshaw(Lx, G, K)[0] * Z).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (K, lhs, rhs)
    # the adjoint's majorant is the forward majorant of the transposed pattern
    G = draw(rng, 3, L.N, 2)
    assert (M.clenshaw(L, G, 3)[1] >= np.abs(M.clenshaw(L, G, 3)[0]) - 1e-12).all()


@pytest.mark.parametrize('name', sorted(MAPS))
def test_one_wrong_edge_centroid_or_entry_is_ten_bounds_away(name):
    """What keeps the GPU tests' tolerance honest: against the operator of the true map, each wrong operator moves at least one
    entry of T_1 = L^ x by more than ten times the bound of that entry, plane_bound(L, 1, A_1) = (d_max + 24) 2^-24 A_1."""
    lab = MAPS[name]
    L = M.laplacian(lab)
    assert L.E > 0
    rng = np.random.default_rng(11)
    x = draw(rng, L.N, 2)
    T, A = M.planes(L, x, 2)
    tol = 10.0 * M.plane_bound(L, 1, A[1])

    def moved(Lw):
        d = np.abs(M.planes(Lw, x, 2)[0][1] - T[1])
        return bool((d > tol).any())
    e = L.E // 2
    keep = np.arange(L.E) != e
    assert moved(M.Lap(L.N, L.row[keep], L.col[keep], L.w[keep], L.xy)), 'dropping one edge'
    # the same edge pointed at another valid node: one that is no neighbour of the row where the map has one (else the entry
    # lands on another of the row's edges)
    i = int(L.row[e])
    taken = set(L.col[L.row == i].tolist()) | {i}
    cand = [j for j in np.nonzero(L.rowlen > 0)[0].tolist() if j not in taken] or [j for j in sorted(taken) if j not in (i, int(L.col[e]))]
    other = cand[0]
    col = L.col.copy()
    col[e] = other
    assert moved(M.Lap(L.N, L.row, col, L.w, L.xy)), 'redirecting one edge'
    xy, rows = unclipped_centroids(lab, L)
    if len(rows):
        assert moved(M.laplacian(lab, xy=xy)), 'the unclipped centroid of a border cell'
    # one entry times 1 + 2^-10: the entry with the largest share of its row's majorant
    share = np.abs(L.val)[:, None] * np.abs(x[L.col]) / A[1][L.row]
    e = int(share.max(axis=1).argmax())
    val = L.val.copy()
    val[e] *= 1.0 + 2.0 ** -10
    assert moved(L.with_val(val)), 'one entry of L^ scaled by 1 + 2^-10'


def test_the_hand_maps_were_checked_with_a_wrong_centroid():
    for name in ('hand', 'hand_x2'):
        assert len(unclipped_centroids(MAPS[name], M.laplacian(MAPS[name]))[1])
