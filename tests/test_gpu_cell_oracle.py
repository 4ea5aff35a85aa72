"""One GConvLSTM update on a real device mesh against the oracle's cell run in float64 on the CPU, across the dispatch table of
the gate GEMM + cell: the persistent k_gate_cell_p (each instantiated reduction length, the generic one and GATE_P_MAXK), the
tiled k_gemm_fwd of hidden 8 / 16 / 32, qt_dense2 + qt_lstm_fwd at hidden 64 and 128, the reduction at MAXQ (512 rows), both
backward launches (qt_lstm_bwd_dgrad, qt_lstm_bwd), and the meshes where kernels go wrong: one node without edges per clip,
more rows than one persistent sweep covers, and a frame of several 64 x 64 base cells."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import close, dev, grad_close

pytestmark = pytest.mark.gpu


def _mesh_64(seed, noise=0.0, B=1, thresh=0.1):
    from qtmpnn import synthetic
    from qtmpnn.mesh import build_mesh
    img = np.stack([synthetic.make_clip(seed + i, n_frames=1, pixel_noise=noise)[0, ..., 0] for i in range(B)])
    return build_mesh(src=torch.from_numpy(img).to(dev()), thresh=thresh), img


def _oracle_graph(mesh):
    ei = mesh.edge_index(True).cpu()
    return ei, mesh.edge_attrs(False).cpu()


@pytest.fixture
def launched(monkeypatch):
    from qtmpnn import _lib
    names, call = [], _lib.call

    def rec(name, *a):
        names.append(name)
        return call(name, *a)
    monkeypatch.setattr(_lib, 'call', rec)
    return names


@contextlib.contextmanager
def _float64():
    """The oracle allocates its zero states and PyG-style constants with the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _mesh(kind):
    from qtmpnn import synthetic
    from qtmpnn.mesh import build_mesh, build_pixel_mesh
    if kind == 'quad64':                  # two clips of a 64 x 64 quadtree mesh: clip-resident planes
        return _mesh_64(3, noise=0.02, B=2)[0]
    if kind == 'single':                  # a constant frame: each clip is ONE 64 x 64 node without edges (deg 0: inf -> 0)
        return build_mesh(src=torch.zeros(2, 64, 64, device=dev()), thresh=0.1)
    if kind == 'pixel':                   # thresh = -inf: 3 x 4096 rows, more than one sweep of the persistent grid
        return build_pixel_mesh(3, 64, 64, device=dev())
    assert kind == 'tile128'              # one 128 x 128 frame: several base cells, tile-resident or per-hop planes
    img = synthetic.make_clip(30, canvas=(128, 128), n_digits=2, n_frames=1, pixel_noise=0.02)[..., 0]
    return build_mesh(src=torch.from_numpy(np.ascontiguousarray(img)).to(dev()), thresh=0.1)


# (conv, hidden, n_conv, cin, packed gate rows K or None, mesh kind, first step with H = C = None); the branch in the id
CASES = [
    ('ChebConv', 16, 1, 4, 64, 'quad64', True, 'persistent-nj8'),
    ('ChebConv', 8, 2, 8, 84, 'quad64', False, 'persistent-nj11'),
    ('ChebConv', 16, 1, 16, 100, 'quad64', False, 'persistent-nj13'),
    ('ChebConv', 16, 1, 68, 256, 'quad64', False, 'persistent-maxk'),
    ('ChebConv', 16, 1, 72, 268, 'quad64', False, 'tiled-h16'),
    ('ChebConv', 8, 4, 24, 296, 'quad64', False, 'tiled-h8'),
    ('ChebConv', 32, 1, 4, None, 'quad64', False, 'tiled-h32'),
    ('ChebConv', 64, 1, 4, None, 'quad64', False, 'dense2-lpn16'),
    ('ChebConv', 64, 3, 8, 512, 'quad64', False, 'dense2-maxq'),
    ('ChebConv', 128, 1, 4, None, 'quad64', False, 'dense2-lpn32'),
    ('GCNConv', 16, 2, 4, None, 'quad64', True, 'gcn-gate-cell'),
    ('GCNConv', 64, 5, 20, 512, 'quad64', False, 'gcn-maxq'),
    ('GCNConv', 128, 2, 4, None, 'quad64', False, 'gcn-lpn32'),
    ('ChebConv', 16, 1, 4, 64, 'single', True, 'single-h16'),
    ('ChebConv', 64, 1, 4, None, 'single', False, 'single-h64'),
    ('ChebConv', 8, 1, 4, None, 'pixel', True, 'pixel-h8'),
    ('ChebConv', 16, 1, 4, 64, 'pixel', False, 'pixel-h16'),
    ('ChebConv', 128, 1, 4, None, 'pixel', False, 'pixel-h128'),
    ('ChebConv', 16, 2, 4, None, 'tile128', True, 'tile128-h16'),
    ('ChebConv', 64, 2, 4, None, 'tile128', False, 'tile128-h64'),
]


def _init(ref, conv):
    """Xavier-like weights (about 1 / sqrt(fan-in) per composed product), so that the gates stay live (see _assert_live)."""
    torch.manual_seed(1234)
    nk = 3 if conv == 'ChebConv' else 1
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name.endswith('weight'):
                p.normal_(0, (nk * p.shape[1]) ** -0.5)
            elif name.startswith('w_c_'):
                p.normal_(0, 0.5)
            else:
                p.normal_(0, 0.2)


def _gate_preacts(ref, X, ei, ew, H, C):
    """The oracle's four gate pre-activations (i, f, c, o), the arguments of its sigmoids and tanh."""
    with torch.no_grad():
        g = lambda n: getattr(ref, 'conv_x_' + n)(X, ei, ew) + getattr(ref, 'conv_h_' + n)(H, ei, ew)
        pi = g('i') + ref.w_c_i * C + ref.b_i
        pf = g('f') + ref.w_c_f * C + ref.b_f
        pc = g('c') + ref.b_c
        Cn = torch.sigmoid(pf) * C + torch.sigmoid(pi) * torch.tanh(pc)
        po = g('o') + ref.w_c_o * Cn + ref.b_o
    return pi, pf, pc, po


def _assert_live(pre):
    """Saturated gates would make the gradient comparison vacuous: pre-activations of a moderate spread, most sigmoids away
    from 0 and 1."""
    allp = torch.cat([p.reshape(-1) for p in pre])
    sd = float(allp.std()) if allp.numel() > 1 else float(allp.abs().max())
    assert 0.25 <= sd <= 4.0, f'gate pre-activation std {sd:.3f}'
    sig = torch.sigmoid(torch.cat([pre[0].reshape(-1), pre[1].reshape(-1), pre[3].reshape(-1)]))
    sat = float(((sig < 0.02) | (sig > 0.98)).double().mean())
    assert sat < 0.5, f'{sat:.2%} of the sigmoid gates saturated'


def _expect_launches(names, fwd, h, conv, kc, widths, mesh):
    from qtmpnn import ops
    if h in (8, 16, 32):
        assert 'qt_dense_lstm' in fwd and 'qt_lstm_fwd' not in fwd, fwd
    else:
        assert 'qt_dense2' in fwd and 'qt_lstm_fwd' in fwd and 'qt_dense_lstm' not in fwd, fwd
    if ops._tile_resident(mesh, widths, kc):
        assert 'qt_cheb_tile_fwd' in fwd, fwd
    elif ops._clip_resident(mesh, widths, kc):
        assert 'qt_cheb_clip_fwd' in fwd, fwd
    else:
        assert 'qt_cheb_clip_fwd' not in fwd and 'qt_cheb_tile_fwd' not in fwd, fwd
    bwd = names[len(fwd):]
    nb = kc * sum(widths)
    if h in (8, 16) and 16 < nb <= 128:
        assert 'qt_lstm_bwd_dgrad' in bwd and 'qt_lstm_bwd' not in bwd, bwd
    else:
        assert 'qt_lstm_bwd' in bwd and 'qt_lstm_bwd_dgrad' not in bwd, bwd


def _grads_close(got, ref, names):
    """Gradients by name; a parameter the HIP path leaves untouched (grad None) must have an exactly-zero reference gradient."""
    for a, r, name in zip(got, ref, names):
        if a is None:
            assert r is None or not r.any(), f'{name}: no gradient on the HIP path, reference max {float(r.abs().max())}'
            continue
        grad_close(a, r, msg=name)


@pytest.mark.parametrize('conv,h,n_conv,cin,K,kind,first', [c[:7] for c in CASES], ids=[c[7] for c in CASES])
def test_gconvlstm_cell_vs_float64_oracle(conv, h, n_conv, cin, K, kind, first, launched):
    """Forward (O, H', C'), the gradients of X, H, C and every parameter under random cotangents on all three outputs, and a
    second backward with a cotangent on H' alone (gO, gC' arrive as None); the first step (H = C = None) where `first`."""
    from model.model import GConvLSTM
    from oracle import qt_oracle as O
    mesh = _mesh(kind)
    if kind == 'single':
        assert mesh.N == 2
    if kind == 'pixel':
        assert mesh.N == 3 * 64 * 64
    ei, ew = _oracle_graph(mesh)
    ew = ew.double()
    ref = O.GConvLSTM(cin, h, n_conv, conv)
    _init(ref, conv)
    mine = GConvLSTM(cin, h, n_conv, conv)
    mine.load_state_dict(ref.state_dict())
    mine.to(dev())
    ref.double()
    pad4 = lambda v: v + (-v) % 4
    kc = (2 * n_conv if conv == 'ChebConv' else n_conv) + 1
    ks = kc - 2 if conv == 'ChebConv' else kc - 1          # bias rows: the inner biases pass through the later layers' hops
    rows = mine.pack(pad4(cin), None, (True,))[0].W.shape[0]
    assert rows == kc * (pad4(cin) + h) + pad4(ks), rows
    if K is not None:
        assert rows == K, f'packed gate matrix has {rows} rows, the case is meant for {K}'
    if kind == 'quad64':
        from qtmpnn import ops
        assert ops._clip_resident(mesh, [pad4(cin), h], kc)

    torch.manual_seed(7)
    N = mesh.N
    X, H, C = torch.randn(N, cin), torch.randn(N, h), torch.randn(N, h)
    LN = torch.stack([1 + 0.3 * torch.randn(h), 0.3 * torch.randn(h), 1 + 0.3 * torch.randn(h), 0.3 * torch.randn(h)])
    names = ['X', 'H', 'C'] + [k for k, _ in ref.named_parameters()]
    for step in ('full', 'h_only', 'layernorm') + (('first',) if first else ()):
        with_state, with_ln = step != 'first', step == 'layernorm'
        xr = X.double().requires_grad_(True)
        hr, cr = ((H.double().requires_grad_(True), C.double().requires_grad_(True)) if with_state else (None, None))
        lnr = LN.double().requires_grad_(True) if with_ln else None
        with _float64():
            outs_r = ref(xr, ei, ew, hr, cr)
            if with_ln:              # the encoder's norm_h / norm_c, fused onto H' and C' by the cell kernels
                lnf = torch.nn.functional.layer_norm
                outs_r = (outs_r[0], lnf(outs_r[1], (h,), lnr[0], lnr[1], 1e-5), lnf(outs_r[2], (h,), lnr[2], lnr[3], 1e-5))
            if step == 'full':
                _assert_live(_gate_preacts(ref, xr, ei, ew, hr, cr))
        xg = X.to(dev()).requires_grad_(True)
        hg, cg = ((H.to(dev()).requires_grad_(True), C.to(dev()).requires_grad_(True)) if with_state else (None, None))
        lng = LN.to(dev()).requires_grad_(True) if with_ln else None
        launched.clear()
        if with_ln:
            xp = torch.nn.functional.pad(xg, (0, pad4(cin) - cin))
            outs_g = mine.step(xp, mesh, hg, cg, mine.pack(pad4(cin), lng, (True,))[0])
        else:
            outs_g = mine(xg, mesh, None, hg, cg)
        fwd = list(launched)
        for a, b, nm in zip(outs_g, outs_r, ('O', "H'", "C'")):
            close(a, b, msg=f'{step} {nm}')
        torch.manual_seed(11)
        if step == 'h_only':
            gs = [torch.randn(N, h, dtype=torch.float64)]
            og, orf = outs_g[1:2], outs_r[1:2]
        else:
            gs = [torch.randn(N, h, dtype=torch.float64) for _ in range(3)]
            og, orf = outs_g, outs_r
        ins_r = [xr] + ([hr, cr] if with_state else []) + list(ref.parameters()) + ([lnr] if with_ln else [])
        ins_g = [xg] + ([hg, cg] if with_state else []) + list(mine.parameters()) + ([lng] if with_ln else [])
        with _float64():
            gr = torch.autograd.grad(orf, ins_r, gs, allow_unused=True)
        gg = torch.autograd.grad(og, ins_g, [g.float().to(dev()) for g in gs], allow_unused=True)
        nm = (names if with_state else names[:1] + names[3:]) + (['ln'] if with_ln else [])
        assert len(gg) == len(gr) == len(nm)
        _grads_close(gg, gr, [f'{step} {n}' for n in nm])
        _expect_launches(launched, fwd, h, conv, kc, [pad4(cin)] + ([h] if with_state else []), mesh)
