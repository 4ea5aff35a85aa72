"""The on-device quadtree build (csrc/quadtree.hip through qtmpnn.mesh.build_mesh) against tests/mesh_model.py: per-clip walks of
the oracle's sequential depth-first decomposition, assembled into the batched mesh.  Kernel against model, never kernel against
kernel: labels, levels, cells, node and base-cell offsets, pixel counts and the re-mesh row indices must be EQUAL; posfeat, whose
three channels are one float32 division each of exactly representable operands, must lie within 2 * 2^-24 relative
(mesh_model.posfeat_bound).  The cases and the property each is there for: mesh_model.cases(), proved to bite by
tests/test_mesh_model_host.py.  Every case prints its node count and worst posfeat error / bound before it asserts (pytest -s; a
recorded run: profiles/mesh_oracle.txt)."""
import numpy as np
import pytest
import torch

import cheb_f64
import mesh_model as M
from helpers import dev
from test_gpu_cheb_f64 import graph_check, host_graph

pytestmark = pytest.mark.gpu

WORST = {'posfeat': 0.0}
ALL = M.cases()


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def build(c, monkeypatch, static=False):
    """build_mesh of a case of the table (the transform path hands over the padded criterion with n, m given)."""
    from model.graph_functions import _criterion
    from qtmpnn import mesh as mesh_mod
    if c.quads is not None:
        monkeypatch.setattr(mesh_mod, '_STAGE1_QUADS', c.quads)
    src = _dev(c.imgs)
    if c.transform:
        src = _criterion(src, c.n, c.m, c.max_size, M.dist_from_05)
        assert tuple(src.shape[1:]) == (M.cdiv(c.n, c.max_size) * c.max_size, M.cdiv(c.m, c.max_size) * c.max_size)
    return mesh_mod.build_mesh(src=src, n=c.n, m=c.m, thresh=c.thresh, condition=c.condition, mask=c.mask,
                               high_interest_region=c.hir, max_size=c.max_size, static=static)


def compare(name, mesh, md):
    """Every output of the build against the model: exact, but for posfeat."""
    nv = mesh.n_valid
    assert nv == md.N, f'{name}: {nv} nodes, the walk gives {md.N}'
    assert mesh.N == (md.B * md.n * md.m if mesh.n_dev is not None else md.N)
    assert (mesh.B, mesh.n, mesh.m) == (md.B, md.n, md.m)
    lab = _np(mesh.labels).astype(np.int64)
    assert np.array_equal(lab, md.labels), f'{name}: labels differ at {int((lab != md.labels).sum())} pixels'
    assert np.array_equal(_np(mesh.level), md.level), f'{name}: level'
    assert np.array_equal(_np(mesh.node_off).astype(np.int64), md.node_off), f'{name}: node_off'
    if mesh.max_size == 64:
        assert np.array_equal(_np(mesh.cell_off).astype(np.int64), md.cell_off), f'{name}: cell_off'
    assert np.array_equal(_np(mesh.cell)[:nv].astype(np.int64), md.cell[:nv]), f'{name}: cell'
    assert np.array_equal(_np(mesh.npix)[:nv].astype(np.float64), md.npix.astype(np.float64)), f'{name}: npix'
    got = _np(mesh.posfeat)[:nv].astype(np.float64)
    assert got.dtype == np.float64 and _np(mesh.posfeat).dtype == np.float32
    err, bound = np.abs(got - md.posfeat), M.posfeat_bound(md)
    assert (err[bound == 0] == 0).all(), f'{name}: posfeat differs where the model is exactly 0'
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    WORST['posfeat'] = max(WORST['posfeat'], ratio)
    per_clip = np.diff(md.node_off).tolist()
    print(f'  [mesh_oracle] {name}: N = {md.N} {per_clip if len(per_clip) <= 6 else ""} posfeat worst error / bound = {ratio:.3g} '
          f'(session worst {WORST["posfeat"]:.3g})')
    assert ratio <= 1.0, f'{name}: posfeat worst error / bound = {ratio:.4g}'


# ------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize('c', [c for c in ALL if not c.tall], ids=lambda c: c.name)
def test_build(c, monkeypatch):
    compare(c.name, build(c, monkeypatch), M.model_for(c))


@pytest.mark.parametrize('c', [c for c in ALL if c.transform], ids=lambda c: c.name)
def test_transform_api(c, monkeypatch):
    """model.graph_functions.quadtree_decompose(..., transform_func=dist_from_05): the caller's path to the same labels."""
    from model.graph_functions import quadtree_decompose
    from qtmpnn import mesh as mesh_mod
    if c.quads is not None:
        monkeypatch.setattr(mesh_mod, '_STAGE1_QUADS', c.quads)
    md = M.model_for(c)
    for b in range(c.B):
        lab = quadtree_decompose(_dev(c.imgs[b]), thresh=c.thresh, max_size=c.max_size, transform_func=M.dist_from_05)
        assert np.array_equal(lab, np.where(md.labels[b] >= 0, md.labels[b] - md.node_off[b], -1))


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('c', [c for c in ALL if c.tall], ids=lambda c: c.name)
def test_tall_base_grid_is_refused(c, monkeypatch):
    """More base rows than base columns: the oracle's split window is empty (IndexError), and so says build_mesh -- from an
    image and from node values alike, before anything is launched."""
    with pytest.raises(IndexError):
        M.walk(c.imgs[0], c.thresh, c.max_size)
    with pytest.raises(IndexError):
        build(c, monkeypatch)
    old = build(M.case(f'grid-{c.n}x{c.m}-ms32'), monkeypatch)
    with pytest.raises(IndexError):
        from qtmpnn.mesh import build_mesh
        build_mesh(prev=(torch.zeros(old.N, device=dev()), old), thresh=0.5, max_size=c.max_size)
    torch.cuda.synchronize()


@pytest.mark.parametrize('max_size', [1, 128])
def test_max_size_out_of_range_is_refused(max_size):
    """The kernels hold base cells of 2 .. 64 pixels a side in LDS: any other power of two raises and launches nothing."""
    from qtmpnn.mesh import build_mesh
    with pytest.raises((RuntimeError, ValueError, AssertionError)):
        build_mesh(src=torch.zeros(2, 128, 128, device=dev()), thresh=0.5, max_size=max_size)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- re-mesh
REMESH = ['grid-64x64-ms64-q1', 'grid-64x64-ms64-q0', 'grid-64x40-ms64-q1', 'both-80x150-ms64-q1', 'both-80x150-ms64-q0',
          'grid-128x128-ms64-q1', 'grid-64x64-ms8', 'both-100x100-ms16']


@pytest.mark.parametrize('static', [False, True], ids=['dynamic', 'static'])
@pytest.mark.parametrize('name', REMESH)
def test_remesh(name, static, monkeypatch):
    """build_mesh(prev=(val[:, 0], old)) with strided node values: the criterion is the un-flattened node values (masked pixels
    read 0), quantised so that ties with thresh = 0.125 occur; labels, level, cell, fwd_src and bwd_src against the model."""
    from qtmpnn.mesh import build_mesh
    c = M.case(name)
    old, omd = build(c, monkeypatch, static=static), M.model_for(c)
    rng = np.random.default_rng(len(name))
    val = np.full((old.N, 4), 0.75, np.float32)                  # (columns 1 .. 3 and the capacity rows: never read)
    val[:omd.N, 0] = rng.choice(np.array([0.0, 0.125, 0.25], np.float32), size=omd.N, p=[0.9, 0.07, 0.03])
    dval = _dev(val)
    assert dval[:, 0].stride(0) == 4
    new = build_mesh(prev=(dval[:, 0], old), thresh=0.125, mask=c.mask, high_interest_region=c.hir, max_size=c.max_size, static=static)
    crit = M.remesh_criterion(val[:omd.N, 0], omd.labels)
    assert (crit == 0.125).any() and (crit > 0.125).any()
    nmd = M.model_of(crit, c.max_size, 0.125, mask=c.mask, hir=c.hir)
    compare(f'remesh {name} static={int(static)}', new, nmd)
    fwd, bwd = M.remesh_indices(omd, nmd)
    assert np.array_equal(_np(new.fwd_src)[:nmd.N].astype(np.int64), fwd), 'fwd_src'
    assert np.array_equal(_np(new.bwd_src)[:omd.N].astype(np.int64), bwd), 'bwd_src'
    assert (fwd >= 0).any() and (bwd >= 0).any() and (bwd == -1).any()


# --------------------------------------------------------------------------------------------------- static mode and the scans
def _scan_case(n, m, ms, B):
    """B clips of the grid kinds (zero | all above | blob | scattered | quantised, in turn) for the scan-length cases."""
    rng = M._rng('scan', n, m, ms, B)
    kinds = [lambda: np.zeros((n, m), np.float32), lambda: np.ones((n, m), np.float32), lambda: M.img_blob(rng, n, m),
             lambda: M.img_scattered(rng, n, m), lambda: M.img_quantised(rng, n, m, 'max_larger_than')]
    return M._case(f'scan-{n}x{m}-ms{ms}-B{B}', np.stack([kinds[(b + 2) % 5]() for b in range(B)]), ms)


# counts = B * base cells (* 4 with the quadrant kernel): stage 3 scans up to 1024 itself in static mode (more than 256: with a
# carry), k_scan_small loops over chunks of 2048, and above 32768 three kernels scan
SCAN = {'320': (64, 64, 8, 5), '1024': (32, 64, 2, 2), '3072': (64, 64, 2, 3), '33792': (64, 64, 2, 33)}
_SCAN_CASES = {}


def _scan(tag):
    if tag not in _SCAN_CASES:
        _SCAN_CASES[tag] = _scan_case(*SCAN[tag])
    return _SCAN_CASES[tag]


@pytest.mark.parametrize('static', [False, True], ids=['dynamic', 'static'])
@pytest.mark.parametrize('tag', list(SCAN))
def test_scan_lengths_through_the_build(tag, static, monkeypatch):
    c = _scan(tag)
    nbase = M.cdiv(c.n, c.max_size) * M.cdiv(c.m, c.max_size)
    assert c.B * nbase == int(tag)
    mesh = build(c, monkeypatch, static=static)
    compare(f'{c.name} static={int(static)}', mesh, M.model_for(c))


STATIC = ['grid-64x64-ms64-q1', 'grid-65x129-ms64-q1', 'grid-65x129-ms64-q0', 'both-80x150-ms64-q1', 'maskwhole-128x128-ms64-q1',
          'grid-50x70-ms4', 'cond-33x65-ms32-min_smaller_than', 'transform-50x70-ms8']


@pytest.mark.parametrize('name', STATIC)
def test_static_mode(name, monkeypatch):
    """Static mode (capacity rows, node count on the device): n_valid and every valid row equal the model, and the dynamic build."""
    c = M.case(name)
    st, dy = build(c, monkeypatch, static=True), build(c, monkeypatch)
    assert st.n_dev is not None and st.N == c.B * c.n * c.m
    compare(f'static {name}', st, M.model_for(c))
    nv = dy.N
    assert st.n_valid == nv
    for f in ('labels', 'level', 'node_off'):
        assert torch.equal(getattr(st, f), getattr(dy, f)), f
    for f in ('cell', 'npix', 'posfeat'):
        assert torch.equal(getattr(st, f)[:nv], getattr(dy, f)[:nv]), f


@pytest.mark.parametrize('length', [1, 8, 2047, 2048, 2049, 32768, 32769, 70001])
def test_scan_i32_is_cumsum(length):
    """qt_scan_i32: out[0] = 0, out[i + 1] = in[0] + .. + in[i], the trailing total included; one workgroup up to 32768 items
    (chunks of 2048), three kernels beyond."""
    from qtmpnn import _lib
    rng = np.random.default_rng(length)
    cnt = rng.integers(0, 4097, length).astype(np.int32)
    d_in = _dev(cnt)
    d_out = torch.full((length + 1,), -7, dtype=torch.int32, device=dev())
    tmp = torch.empty(length // 1024 + 8, dtype=torch.int32, device=dev())
    _lib.call('qt_scan_i32', _lib.ptr(d_in), _lib.ptr(d_out), length, _lib.ptr(tmp))
    want = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    assert want[-1] < 2 ** 31
    assert np.array_equal(_np(d_out).astype(np.int64), want)


# -------------------------------------------------------------------------------------------------------------- graph on top
@pytest.mark.parametrize('name', ['grid-65x129-ms64-q1', 'grid-64x40-ms64-q1', 'both-80x150-ms64-q1', 'both-100x100-ms16', 'grid-50x70-ms8'])
def test_graph_on_the_oracle_labels(name, monkeypatch):
    """CSR, w, dis, nrm and ell of clipped and masked cells against cheb_f64.laplacian of the ORACLE's labels (the assertions of
    tests/test_gpu_cheb_f64.py, which take the device's own labels)."""
    c = M.case(name)
    mesh, md = build(c, monkeypatch), M.model_for(c)
    L = cheb_f64.laplacian(md.labels, resolution=mesh.resolution, N=md.N)
    graph_check(f'oracle {name}', host_graph(mesh), L)
