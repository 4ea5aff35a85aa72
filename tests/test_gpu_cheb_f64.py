"""The chain every ChebConv runs through -- qt_edges_count / qt_edges_fill / qt_edges_norm(_tiles) (csrc/edges.hip), k_spmm / k_spmm1
(csrc/cheb.hip), the clip-resident and tile-resident k_cheb_clip (csrc/chebclip.hip), forwards and as the Clenshaw backward --
against the float64 model tests/cheb_f64.py, which knows a mesh only by its label map.

Every comparison is kernel against model, never kernel against kernel.  The bounds live beside the model with their derivations
(cheb_f64.w_bound, dis_bound, nrm_bound, plane_bound): twice a count of float32 roundings times 2^-24 times the majorant the model
returns; an entry whose majorant is 0 must be exact.  Inputs are sign * (0.5 + U[0, 1)), so that one wrong edge, centroid or weight
is ten bounds away (tests/test_cheb_f64_host.py).  Every case prints its worst error / bound before it asserts (pytest -s; a
recorded run: profiles/cheb_f64.txt)."""
import copy

import numpy as np
import pytest
import torch

import cheb_f64 as M
from helpers import _tile_mesh, dev, golden

pytestmark = pytest.mark.gpu

SENT = -7.25            # sentinel of pre-filled outputs
WORST = {}              # family -> worst error / bound seen in this session


# ------------------------------------------------------------------------------------------------------------------ helpers
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


def draw(rng, *shape):
    """sign * (0.5 + U[0, 1)) as float32."""
    return (rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))).astype(np.float32)


def compare(got, ref, bound):
    """Worst |got - ref| / bound over all entries; inf where a compared entry is not finite or an entry with bound 0 differs."""
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64)
    ref, bound = np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float('inf')
    err = np.abs(got - ref)
    pos = bound > 0
    if (err[~pos] != 0).any():
        return float('inf')
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check(family, name, got, ref, bound):
    ratio = compare(got, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f'  [{family}] {name}: {ratio:.3g}')
    assert ratio <= 1.0, f'{family} {name}: worst error / bound = {ratio:.4g}'
    return ratio


def pad(mesh, a, fill=np.nan):
    """Node tensor for `mesh` from the (n_valid, ...) array a: in static mode padded to the capacity with `fill` rows."""
    a = np.asarray(a, np.float32)
    if mesh.N > a.shape[0]:
        a = np.concatenate([a, np.full((mesh.N - a.shape[0], *a.shape[1:]), fill, np.float32)])
    return _t(a)


def untouched(name, t, nv, axis=0):
    """The capacity rows of an output that was pre-filled with SENT still hold it."""
    cap = _np(t).take(range(nv, t.shape[axis]), axis=axis)
    assert (cap == SENT).all(), f'{name}: a capacity row was written'


# ------------------------------------------------------------------------------------------------------------------- meshes
TAGS = ['S', 'C', 'D', 'Z', 'P', 'H', 'T', 'wide64x128', 'masked_tile', 'ice96x128']
SMALL = ['S', 'C', 'D', 'Z', 'P', 'H', 'T']            # frames of at most 64 x 64: the clip-resident launches
TILE_B = {'wide64x128': 3, 'masked_tile': 2, 'ice96x128': 2}
_CACHE = {}


def _sparse64(B, static=False):
    """The sparse 64 x 64 mesh of seed 11 (tests/test_gpu_ops.py): cells of 1 .. 32 pixels side by side."""
    from qtmpnn import synthetic
    from qtmpnn.mesh import build_mesh
    img = np.stack([synthetic.make_clip(11 + i, n_frames=1, pixel_noise=0.0)[0, ..., 0] for i in range(B)])
    return build_mesh(src=torch.from_numpy(img).to(dev()), thresh=0.1, static=static)


def _build(tag):
    from qtmpnn.mesh import build_mesh, build_pixel_mesh
    if tag == 'S':                                     # 24 x 32, B = 1
        c = np.zeros((1, 24, 32), np.float32)
        c[0, 0:5, 0:7] = 1.0
        return build_mesh(src=_t(c), thresh=0.5)
    if tag == 'C':                                     # 64 x 40, B = 2: cells that the right border clips
        c = np.zeros((2, 64, 40), np.float32)
        c[0, 30:36, 33:40] = 1.0
        c[1] = np.random.default_rng(ord('C')).random((64, 40)) < 0.03
        return build_mesh(src=_t(c), thresh=0.5)
    if tag in ('D', 'T'):
        return _sparse64(3, static=(tag == 'T'))
    if tag == 'Z':                                     # a constant frame: one node per clip, no edge
        return build_mesh(src=torch.zeros(2, 64, 64, device=dev()), thresh=0.1)
    if tag == 'P':
        mk = np.zeros((24, 32), bool)
        mk[5:9, 10:30] = True
        mk[20, 0:3] = True
        return build_pixel_mesh(2, 24, 32, mask=mk, device=dev())
    if tag == 'H':
        from model.graph_functions import create_static_homogeneous_graph
        g = golden('fixed_homog48x64.npz')
        ms = create_static_homogeneous_graph((48, 64), int(g['max_grid_size']), g['mask'], use_edge_attrs=False, device=dev())['mapping']
        return ms.for_batch(2)
    return _tile_mesh(tag, TILE_B[tag])[0]


def get(tag):
    """(mesh, model L^ of its labels), built once."""
    if tag not in _CACHE:
        mesh = _build(tag)
        _CACHE[tag] = (mesh, M.laplacian(_np(mesh.labels), resolution=mesh.resolution, N=mesh.n_valid))
    return _CACHE[tag]


def host_graph(mesh):
    """The device's graph arrays of the valid rows, on the host."""
    nv = mesh.n_valid
    rp = _np(mesh.rowptr).astype(np.int64)[:nv + 1]
    E = int(rp[-1])
    return dict(nv=nv, rp=rp, E=E, col=_np(mesh.col)[:E].astype(np.int64), w=_np(mesh.w)[:E], nrm=_np(mesh.nrm)[:E],
                dis=_np(mesh.dis)[:nv], ell=_np(mesh.ell)[:nv])


def graph_check(tag, g, L):
    """The graph assertions of one mesh from host arrays (g: host_graph) against the model L."""
    nv, rp, E, col = g['nv'], g['rp'], g['E'], g['col']
    assert nv == L.N and rp[0] == 0 and (np.diff(rp) >= 0).all() and E == L.E, (nv, L.N, E, L.E)
    d = np.diff(rp)
    row = np.repeat(np.arange(nv), d)
    order = np.lexsort((col, row))
    # per row the same neighbour set (the model's edges are in (row, col) order and hold no pair twice)
    assert np.array_equal(row[order], L.row) and np.array_equal(col[order], L.col), 'neighbour sets differ'
    assert np.array_equal(d, L.rowlen)
    check('w', tag, g['w'][order], L.w, M.w_bound(L))                  # 2 roundings (cheb_f64.w_bound): 4 U <= 8 U
    check('dis', tag, g['dis'], L.dis, M.dis_bound(L))                 # (d + 1) / 2 + 2 roundings: (d + 5) U <= (d + 8) U
    check('nrm', tag, g['nrm'][order], L.val, M.nrm_bound(L))          # (d_i + d_j) / 2 + 9: (d_i + d_j + 18) U <= (.. + 24) U
    # every stored edge has its transpose: nrm_ij = -(dis_i w) dis_j and nrm_ji = -(dis_j w) dis_i share w bit for bit and round
    # twice each, so they lie within 2 * 2 U of each other
    key = L.row * max(nv, 1) + L.col
    pos = np.searchsorted(key, L.col * max(nv, 1) + L.row)
    assert E == 0 or (pos < E).all() and np.array_equal(key[np.minimum(pos, E - 1)], L.col * max(nv, 1) + L.row), 'an edge without its transpose'
    ns = g['nrm'][order].astype(np.float64)
    ws = g['w'][order]
    if E:
        assert np.array_equal(ws, ws[pos]), 'w_ij != w_ji'
        check('nrm transpose', tag, ns[pos], ns, 4.0 * M.U * np.abs(ns))
        print(f'  [nrm] {tag}: {int((ns != ns[pos]).sum())} of {E} entries differ from their transpose in the last bit')
    # ell: the row's first four col / nrm entries bit for bit, unused slots = the row itself with weight 0, the fourth column
    # complemented exactly where the row has more than four edges
    ell = g['ell']
    nb = g['nrm'].view(np.int32)
    for k in range(4):
        used = d > k
        e = np.minimum(rp[:-1] + k, max(E - 1, 0))
        want_c = np.where(used, col[e] if E else 0, np.arange(nv))
        if k == 3:
            want_c = np.where(d > 4, ~want_c, want_c)
        want_w = np.where(used, nb[e] if E else 0, 0)
        assert np.array_equal(ell[:, k].astype(np.int64), want_c), f'ell column {k}'
        assert np.array_equal(ell[:, 4 + k], want_w.astype(np.int32)), f'ell weight {k}'
    assert ((ell[:, 3] < 0) == (d > 4)).all()


@pytest.mark.parametrize('tag', TAGS)
def test_graph(tag):
    mesh, L = get(tag)
    lab = _np(mesh.labels)
    cell = _np(mesh.cell)[:mesh.n_valid]
    n, m = mesh.n, mesh.m
    # the property this mesh is here for
    if tag == 'S':
        assert (n, m, mesh.B) == (24, 32, 1)
    elif tag == 'C':
        clipped = (cell[:, 2] > 1) & ((cell[:, 0] + cell[:, 2] > n) | (cell[:, 1] + cell[:, 2] > m))
        assert (n, m, mesh.B) == (64, 40, 2) and clipped.any()
        # ... and the clipped extent is where the pixels are: the model's centroid of such a cell is not the whole square's
        i = int(np.nonzero(clipped)[0][0])
        assert (lab == i).sum() < cell[i, 2] ** 2
    elif tag == 'D':
        assert mesh.B == 3 and L.rowlen.max() > 4 and mesh.tail_rec is not None
    elif tag == 'Z':
        assert mesh.N == 2 and L.E == 0 and (_np(mesh.dis) == 0).all()
    elif tag == 'P':
        assert mesh.pixelwise and (lab < 0).any() and (L.w == mesh.resolution).all()
    elif tag == 'H':
        assert mesh.loss_mask is not None and (n, m, mesh.B) == (48, 64, 2)
    elif tag == 'T':
        assert mesh.n_dev is not None and mesh.N == 3 * 64 * 64 and mesh.n_valid == get('D')[0].N
    else:
        assert mesh.tiles is not None and mesh.B == TILE_B[tag]
        off = _np(mesh.cell_off).astype(np.int64)
        tile_of = np.searchsorted(off, np.arange(L.N), side='right') - 1
        assert (tile_of[L.row] != tile_of[L.col]).any(), 'no row with an edge into another tile'
    noff = _np(mesh.node_off).astype(np.int64)
    clip_of = np.searchsorted(noff, np.arange(L.N), side='right') - 1
    assert (clip_of[L.row] == clip_of[L.col]).all(), 'an edge joins two clips'
    graph_check(tag, host_graph(mesh), L)


# --------------------------------------------------------------------------------------------------------------- aggregates
@pytest.mark.parametrize('addends', [True, False])
@pytest.mark.parametrize('C', [1, 3, 4, 20, 24])
@pytest.mark.parametrize('tag', ['S', 'D', 'Z', 'T', 'ice96x128'])
def test_spmm(tag, C, addends):
    """qt_spmm (no ELL array): the scalar path (C = 1, 3), EPT = 8 (C = 4, 20) and EPT = 4 (C = 24), with and without p and q.
    One hop: plane_bound with k = 1 -- the row's fused multiply-adds, the roundings of its L^ entries and the three of the epilogue."""
    from qtmpnn.mesh import spmm
    mesh, L = get(tag)
    nv = L.N
    # which side of the XCD-wise workgroup remapping (taken from 64 workgroups of 64 threads on, N C / 4 >= 4096) this case is on
    if tag in ('S', 'Z'):
        assert nv * C / 4 < 4096 - 64
    if tag == 'ice96x128' and C % 4 == 0:
        assert nv * C // 4 >= 4096
    if tag == 'D':                                     # one mesh on both sides
        assert nv * 4 / 4 < 4096 - 64 and nv * 20 // 4 >= 4096
    rng = np.random.default_rng(1000 + C)
    x, p, q = (draw(rng, nv, C) for _ in range(3))
    out = torch.full((mesh.N, C), SENT, device=dev())
    if addends:
        spmm(mesh, pad(mesh, x), 2.0, pad(mesh, p), -1.0, pad(mesh, q), 0.5, out, C)
        ref, mag = M.axpby(L, x, 2.0, p, -1.0, q, 0.5)
    else:
        spmm(mesh, pad(mesh, x), 1.0, None, 0.0, None, 0.0, out, C)
        ref, mag = M.axpby(L, x, 1.0)
    check('spmm', f'{tag} C={C} addends={int(addends)}', out[:nv], ref, M.plane_bound(L, 1, mag))
    untouched('spmm', out, nv)


@pytest.mark.parametrize('widths', [(4, 16), (8, 32)])
@pytest.mark.parametrize('tag', ['S', 'D', 'T', 'wide64x128'])
def test_spmm2_two_strided_parts_in_place(tag, widths):
    """qt_spmm2 with the ELL array: two row-strided parts, out aliasing p (the in-place Clenshaw step).  (8, 32) is EPT = 4.
    One hop, k = 1."""
    from qtmpnn.mesh import spmm2
    mesh, L = get(tag)
    nv = L.N
    rng = np.random.default_rng(sum(widths))
    wa, wb = widths
    wide_x, wide_q = draw(rng, nv, wa + wb + 12), draw(rng, nv, wa + wb + 4)
    X, Q = pad(mesh, wide_x), pad(mesh, wide_q)
    xs = [X[:, 4:4 + wa], X[:, 8 + wa:8 + wa + wb]]
    qs = [Q[:, 0:wa], Q[:, 4 + wa:4 + wa + wb]]
    p = [draw(rng, nv, wa), draw(rng, nv, wb)]
    ps = [pad(mesh, a, SENT) for a in p]
    spmm2(mesh, xs, 2.0, ps, 1.0, qs, -1.0, ps)
    for i, (c0, q0, w) in enumerate(((4, 0, wa), (8 + wa, 4 + wa, wb))):
        ref, mag = M.axpby(L, wide_x[:, c0:c0 + w], 2.0, p[i], 1.0, wide_q[:, q0:q0 + w], -1.0)
        check('spmm2', f'{tag} {widths} part {i}', ps[i][:nv], ref, M.plane_bound(L, 1, mag))
        untouched('spmm2', ps[i], nv)
    grid = -(-nv * (wb // 4) // 64)
    print(f'  [spmm2] {tag} {widths}: part b of {grid} workgroups, XCD remapping {"on" if grid >= 64 else "off"}')


@pytest.mark.parametrize('ks', [2, 3, 5])
@pytest.mark.parametrize('tag', ['S', 'D', 'Z', 'P'])
def test_cheb_ones(tag, ks):
    """Mesh.cheb_ones: [1, L^ 1, T_2(L^) 1, .. | 0-pad]; column k is k hops of the scalar path: plane_bound with that k."""
    mesh, L = get(tag)
    got = _np(mesh.cheb_ones(ks))
    ref, mag = M.ones(L, ks)
    assert got.shape == (L.N, -(-ks // 4) * 4) and (got[:, ks:] == 0).all() and (got[:, 0] == 1).all()
    for k in range(1, ks):
        check('cheb_ones', f'{tag} ks={ks} column {k}', got[:, k], ref[:, k], M.plane_bound(L, k, mag[:, k]))


def test_scalar_cheb3_forward_and_gradients():
    """ops.scalar_cheb3 (k_spmm1 twice, then qt_act_bwd and k_spmm1 twice) on the sparse 64 x 64 mesh, with a dropout mask and a
    residual that is a column view: y = tanh(drop (u_0 + L^ u_1 + T_2(L^) u_2)) + res, and dL/dU, dL/dres against float64 autograd
    of that formula on the model's L^."""
    from qtmpnn import ops
    mesh, L = get('D')
    N = L.N
    rng = np.random.default_rng(33)
    u = draw(rng, N, 4) * 0.5
    u[:, 3] = 0
    xw = draw(rng, N, 4)
    drop = ((rng.random(N) > 0.2) / 0.8).astype(np.float32)
    gy = draw(rng, N, 4)
    gy[:, 1:] = 0
    assert (drop == 0).any() and (drop > 1).any()
    Ud, Xd = _t(u).requires_grad_(True), _t(xw).requires_grad_(True)
    Y = ops.scalar_cheb3(Ud, Xd[:, :1], _t(drop), mesh)
    gU, gX = torch.autograd.grad(Y, [Ud, Xd], _t(gy))
    # float64: the formula, and autograd of it
    Ls = torch.sparse_coo_tensor(torch.from_numpy(np.stack([L.row, L.col])), torch.from_numpy(L.val), (N, N)).coalesce()
    U64 = torch.from_numpy(u.astype(np.float64)).requires_grad_(True)
    R64 = torch.from_numpy(xw[:, :1].astype(np.float64)).requires_grad_(True)
    d64 = torch.from_numpy(drop.astype(np.float64))[:, None]
    mm = lambda v: torch.sparse.mm(Ls, v)
    v64 = U64[:, 0:1] + mm(U64[:, 1:2]) + 2.0 * mm(mm(U64[:, 2:3])) - U64[:, 2:3]
    y64 = torch.tanh(d64 * v64) + R64
    gU64, gR64 = torch.autograd.grad(y64, [U64, R64], torch.from_numpy(gy[:, :1].astype(np.float64)))
    # forward.  v: two hops (b_1 = u_1 + 2 L^ u_2, then u_0 + L^ b_1 - u_2) on the majorant |u_0| + |L^| |u_1| + A_2(|u_2|);
    # then one product with drop (1 rounding, passed on by tanh' <= 1), tanhf (<= 2 ulp = 4 roundings of |tanh|) and the add
    # of res (1 rounding of |y|), doubled like every count
    ud = u.astype(np.float64)
    A2 = M.planes(L, ud[:, 2], 3)[1][2]
    vmag = np.abs(ud[:, 0]) + M.apply(L, ud[:, 1])[1] + A2
    v = v64.detach().numpy()[:, 0]
    y = y64.detach().numpy()[:, 0]
    dd = drop.astype(np.float64)
    ybound = dd * M.plane_bound(L, 2, vmag) + 2.0 * M.U * (dd * np.abs(v) + 4.0 * np.abs(np.tanh(dd * v)) + np.abs(y))
    got = _np(Y)
    assert (got[:, 1:] == 0).all()
    check('scalar_cheb3', 'forward', got[:, 0], y, ybound)
    # backward.  qt_act_bwd recomputes t = y - res from the stored y (its error ybound, plus 1 rounding of |t|), then
    # g = gy (1 - t t) drop: the square and the difference round once each, the two products once each; doubled.  Columns 1
    # and 2 are one and two hops on g: plane_bound on A_k(|g|), plus the error of g carried through the same majorant recurrence.
    gref = gU64.numpy()
    t = np.tanh(dd * v)
    g0 = gref[:, 0]
    gyd = np.abs(gy[:, 0].astype(np.float64))
    gbound = gyd * dd * (2.0 * np.abs(t) * (ybound + 2.0 * M.U * np.abs(t)) + 2.0 * M.U * (t * t + np.abs(1.0 - t * t))) + 4.0 * M.U * np.abs(g0)
    _, Ag = M.planes(L, g0, 3)
    _, Ae = M.planes(L, gbound, 3)
    gotU = _np(gU)
    assert (gotU[:, 3] == 0).all()
    check('scalar_cheb3', 'dU column 0', gotU[:, 0], g0, gbound)
    for k in (1, 2):
        check('scalar_cheb3', f'dU column {k}', gotU[:, k], gref[:, k], Ae[k] + M.plane_bound(L, k, Ag[k]))
    gotX = _np(gX)
    assert np.array_equal(gotX[:, 0], gy[:, 0]) and (gotX[:, 1:] == 0).all() and np.array_equal(gR64.numpy()[:, 0], gy[:, 0].astype(np.float64))


# -------------------------------------------------------------------------------------------------------------- recurrences
KW = [(2, (8,)), (3, (16, 4)), (5, (4, 16)), (7, (8,))]


def _operands(mesh, L, K, widths, seed):
    """Z parts as column views of one wide matrix, gradient planes G per part; host copies of both."""
    rng = np.random.default_rng(seed)
    nv = L.N
    wide = draw(rng, nv, sum(widths) + 8)
    W = pad(mesh, wide)
    Zs, zs, o = [], [], 4
    for w in widths:
        Zs.append(W[:, o:o + w])
        zs.append(wide[:, o:o + w])
        o += w
    gs = [draw(rng, K, nv, w) for w in widths]
    return Zs, zs, gs


def _dev_planes(mesh, g):
    """(K, N, w) device gradient planes from the (K, n_valid, w) host array: capacity rows NaN."""
    if mesh.N > g.shape[1]:
        g = np.concatenate([g, np.full((g.shape[0], mesh.N - g.shape[1], g.shape[2]), np.nan, np.float32)], axis=1)
    return _t(g)


def _slice_major(G, K, N, w):
    t = G.clone()
    t[1:] = G[1:].view(K - 1, N, w // 4, 4).permute(0, 2, 1, 3).reshape(K - 1, N, w)
    return t


_REFS = {}


def refs(tag, L, zs, gs, K, seed):
    """The model's planes (T, A) per part and its adjoint (value, majorant) per part, computed once per case."""
    key = (tag, K, seed)
    if key not in _REFS:
        _REFS.clear()
        _REFS[key] = ([M.planes(L, z, K) for z in zs], [M.clenshaw(L, g, K) for g in gs])
    return _REFS[key]


def check_forward(family, name, L, fwd, planes_rm, K):
    """planes_rm[i] (K - 1, N, w) row-major against T_1 .. T_{K-1}: plane k is k hops, plane_bound(L, k, A_k)."""
    for i, (T, A) in enumerate(fwd):
        for k in range(1, K):
            check(family, f'{name} part {i} T_{k}', planes_rm[i][k - 1, :L.N], T[k], M.plane_bound(L, k, A[k]))


def check_adjoint(family, name, L, adj, got0, K):
    """got0[i] (N, w): plane 0 after the Clenshaw backward, against sum_k T_k(L^)^T G_k: K - 1 hops on the adjoint's majorant."""
    for i, (ref, mag) in enumerate(adj):
        check(family, f'{name} part {i}', got0[i][:L.N], ref, M.plane_bound(L, K - 1, mag))


@pytest.mark.parametrize('K,widths', KW)
@pytest.mark.parametrize('tag', SMALL + ['wide64x128'])
def test_per_hop_recurrence(tag, K, widths):
    """One qt_spmm2 launch per hop (ops._CLIP_CHEB off): forward planes through ops._cheb_planes, and the Clenshaw backward as
    ops._cheb_backward issues it."""
    from qtmpnn import ops
    from qtmpnn.mesh import spmm2
    mesh, L = get(tag)
    Zs, zs, gs = _operands(mesh, L, K, widths, 10 * K + len(widths))
    fwd, adj = refs(tag, L, zs, gs, K, 10)
    prev, ops._CLIP_CHEB = ops._CLIP_CHEB, False
    try:
        TZs, sm = ops._cheb_planes(Zs, mesh, K)
        assert sm == 0
    finally:
        ops._CLIP_CHEB = prev
    check_forward('per-hop forward', f'{tag} K={K} {widths}', L, fwd, TZs, K)
    Gr = [_dev_planes(mesh, g) for g in gs]
    for k in range(K - 2, 0, -1):
        spmm2(mesh, [g[k + 1] for g in Gr], 2.0, [g[k] for g in Gr], 1.0, [g[k + 2] for g in Gr] if k + 2 < K else None, -1.0,
              [g[k] for g in Gr])
    spmm2(mesh, [g[1] for g in Gr], 1.0, [g[0] for g in Gr], 1.0, [g[2] for g in Gr] if K > 2 else None, -1.0, [g[0] for g in Gr])
    check_adjoint('per-hop Clenshaw', f'{tag} K={K} {widths}', L, adj, [g[0] for g in Gr], K)
    if mesh.N > L.N:
        assert all(bool(torch.isnan(g[0, L.N:]).all()) for g in Gr)            # capacity rows: as given


@pytest.mark.parametrize('K,widths', KW)
@pytest.mark.parametrize('tag', SMALL)
def test_clip_resident_recurrence(tag, K, widths):
    """csrc/chebclip.hip, a clip's rows in LDS: forward planes and the Clenshaw backward (row-major and slice-major gradient
    planes) at both slice widths and the automatic choice, each run against the model."""
    from qtmpnn import ops
    mesh, L = get(tag)
    assert mesh.tail_rec is not None and mesh.n * mesh.m <= 4096
    nv, N = L.N, mesh.N
    Zs, zs, gs = _operands(mesh, L, K, widths, 20 * K + len(widths))
    fwd, adj = refs(tag, L, zs, gs, K, 20)
    for width in (4, 2, 0):
        fused = [torch.full((K - 1, N, w), SENT, device=dev()) for w in widths]
        ops.clip_planes(mesh, Zs, fused, K, width=width)
        rm = [ops.planes_rowmajor(a, 1) for a in fused]
        check_forward('clip forward', f'{tag} K={K} {widths} width={width}', L, fwd, rm, K)
        for a in rm:
            untouched('clip forward', a, nv, axis=1)
        for sm in (0, 1):
            G = [_dev_planes(mesh, g) for g in gs]
            Gin = [_slice_major(g, K, N, w) if sm else g.clone() for g, w in zip(G, widths)]
            Gw = [g.clone() for g in Gin]
            ops.clip_clenshaw(mesh, Gw, K, sm=sm, width=width)
            check_adjoint('clip Clenshaw', f'{tag} K={K} {widths} width={width} sm={sm}', L, adj, [g[0] for g in Gw], K)
            for a, b in zip(Gw, Gin):
                assert torch.equal(torch.nan_to_num(a[1:], nan=SENT), torch.nan_to_num(b[1:], nan=SENT))      # planes 1 .. K-1 stay as given
                if N > nv:
                    assert bool(torch.isnan(a[0, nv:]).all())


@pytest.mark.parametrize('K,widths', [(3, (4, 16)), (5, (16, 16)), (4, (16,))])
@pytest.mark.parametrize('tag', ['wide64x128', 'masked_tile', 'ice96x128'])
def test_tile_resident_recurrence(tag, K, widths):
    """csrc/chebclip.hip with TILE = true, on the (mesh, B, K, widths) combinations and with the calls of tests/test_gpu_ops.py::
    test_tile_resident_recurrence_equals_per_hop_launches (a fresh mesh, column views as Z): forward planes and both Clenshaw
    layouts against the model; the error word stays 0 after every launch."""
    from qtmpnn import ops
    mesh, _ = _tile_mesh(tag, TILE_B[tag])
    _, L = get(tag)
    assert mesh.tiles is not None and mesh.N == L.N and torch.equal(mesh.labels, get(tag)[0].labels)
    N = mesh.N
    Zs, zs, gs = _operands(mesh, L, K, widths, 30 * K + len(widths))
    fwd, adj = refs(tag, L, zs, gs, K, 30)
    fused = [torch.empty(K - 1, N, w, device=dev()) for w in widths]
    ops.clip_planes(mesh, Zs, fused, K)
    assert int(mesh.tiles['err']) == 0, 'error word set by the forward launch'
    check_forward('tile forward', f'{tag} K={K} {widths}', L, fwd, [ops.planes_rowmajor(a, 1) for a in fused], K)
    G = [_t(g) for g in gs]
    Gf = [g.clone() for g in G]
    ops.clip_clenshaw(mesh, Gf, K)
    assert int(mesh.tiles['err']) == 0, 'error word set by the backward launch'
    Gs = [_slice_major(g, K, N, w) for g, w in zip(G, widths)]
    ops.clip_clenshaw(mesh, Gs, K, sm=1)
    assert int(mesh.tiles['err']) == 0, 'error word set by the slice-major backward launch'
    check_adjoint('tile Clenshaw', f'{tag} K={K} {widths} sm=0', L, adj, [g[0] for g in Gf], K)
    check_adjoint('tile Clenshaw', f'{tag} K={K} {widths} sm=1', L, adj, [g[0] for g in Gs], K)
    for a, g0 in zip(Gf, G):
        assert torch.equal(a[1:], g0[1:])


# ------------------------------------------------------------------------------------------------------------------- tamper
def test_one_weight_off_by_a_thousandth_fails_the_comparison():
    """The bound can fail on the device: one entry of L^ times 1.001 -- in `nrm` and, being among its row's first four, in the ELL
    array that k_spmm and the clip-resident kernel read it from -- on a shallow copy of the 64 x 64 mesh.  Values only: no index,
    count or capacity changes.  The row has at most four edges, so both kernels take this weight from `ell` alone."""
    from qtmpnn import ops
    from qtmpnn.mesh import spmm2
    mesh, L = get('D')
    g = host_graph(mesh)
    d = np.diff(g['rp'])
    short = np.nonzero((d >= 1) & (d <= 4))[0]
    i = int(short[len(short) // 3])
    e = int(g['rp'][i])
    bad = copy.copy(mesh)
    bad.nrm = mesh.nrm.clone()
    bad.ell = mesh.ell.clone()
    bad.nrm[e] *= 1.001
    bad.ell[i, 4:5] = bad.nrm[e:e + 1].view(torch.int32)
    assert int(bad.ell[i, 0]) == int(mesh.col[e]) and not torch.equal(bad.ell, mesh.ell)
    rng = np.random.default_rng(77)
    x = draw(rng, L.N, 8)
    ref, mag = M.axpby(L, x, 1.0)
    for ms, fails in ((mesh, False), (bad, True)):
        out = torch.empty(L.N, 8, device=dev())
        spmm2(ms, [_t(x)], 1.0, None, 0.0, None, 0.0, [out])
        r = compare(out, ref, M.plane_bound(L, 1, mag))
        print(f'  [tamper] spmm2 tampered={int(fails)}: {r:.3g}')
        assert (r > 1.0) == fails
        K = 3
        fused = [torch.empty(K - 1, L.N, 8, device=dev())]
        ops.clip_planes(ms, [_t(x)], fused, K)
        T, A = M.planes(L, x, K)
        r = max(compare(ops.planes_rowmajor(fused[0], 1)[k - 1], T[k], M.plane_bound(L, k, A[k])) for k in range(1, K))
        print(f'  [tamper] clip forward tampered={int(fails)}: {r:.3g}')
        assert (r > 1.0) == fails


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per family of this session (the figures of profiles/cheb_f64.txt); every one is <= 1."""
    for fam in sorted(WORST):
        print(f'  worst [{fam}]: {WORST[fam]:.3g}')
    assert all(v <= 1.0 for v in WORST.values())
