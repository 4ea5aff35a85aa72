"""Host checks of the float64 TransformerConv cell model (tests/tcell_f64.py) on its own: without dropout against the oracle's
GConvLSTM in float64 on the oracle's own graph of the same frame; with dropout the head order of the masks (against the same model
evaluated stack by stack, one head at a time), their change with the epoch and the kept share.  No GPU, nothing of qtmpnn."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tcell_f64
from attn_f64 import attention_f64

THRESH = 0.1


def _frame():
    """(The 24 x 32 frame of tests/test_gpu_attn_f64.py's mesh S.)"""
    f = np.zeros((1, 24, 32), np.float32)
    f[0, 5:9, 9:14] = 1.0
    f[0, 17, 20:27] = 1.0
    f[0, 12:21, 2:4] = 1.0
    return f


@contextlib.contextmanager
def _float64():
    """The oracle allocates its zero states with the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _graph():
    """The oracle's graph of the frame (edge list with self pairs, attributes [angle, dist]) and the same as the model's geometry:
    CSR by target of the pairs i != j, col = source, the attributes of that very edge; selfpair = 1 where (i, i) is an edge."""
    from oracle import qt_oracle as O
    img = O.add_positional_encoding(torch.from_numpy(_frame()).double().unsqueeze(-1))
    g = O.image_to_graph(img, thresh=THRESH, use_edge_attrs=True)
    ei, ea = g['edge_index'].numpy(), g['edge_attrs'].double().numpy()
    N = int(g['n_pixels_per_node'].numel())
    src, dst = ei
    loop = src == dst
    assert not ea[loop].any(), 'a self pair carries the attributes 0'
    order = np.lexsort((src[~loop], dst[~loop]))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst[~loop], minlength=N))]).astype(np.int64)
    selfpair = np.zeros(N, np.float32)
    selfpair[src[loop]] = 1.0
    geo = SimpleNamespace(N=N, rowptr=rowptr, col=src[~loop][order], eattr=ea[~loop][order], selfpair=selfpair)
    assert (selfpair > 0).any() and (selfpair == 0).any()
    return g['edge_index'], g['edge_attrs'].double(), geo


def _init(ref, s=0.7):
    gen = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name.endswith('lin_edge.weight'):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
            elif name.endswith('weight'):
                p.copy_(torch.randn(p.shape, generator=gen) * s * p.shape[1] ** -0.5)
            elif name.startswith('w_c_'):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.2)


def _same(a, b, what, rel=1e-10, floor=1e-3):
    """max |a - b| <= rel x the tensor's largest entry (at least `floor`: the key-bias gradients are exact zeros, both sides noise)."""
    a, b = a.detach().numpy(), b.detach().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()), floor)
    assert np.abs(a - b).max() <= rel * scale, (what, float(np.abs(a - b).max()), scale)


@pytest.mark.parametrize('with_state', [True, False], ids=['state', 'first'])
@pytest.mark.parametrize('cin,h,L', [(5, 32, 3), (4, 8, 2), (1, 4, 1)])
def test_model_equals_the_oracle_cell_without_dropout(cin, h, L, with_state):
    """keep = 1: (O, H', C') and the gradients of X, H, C and every parameter under random cotangents on all three equal
    oracle.qt_oracle.GConvLSTM in float64 to 1e-10 relative (both sides float64, another summation order)."""
    from oracle import qt_oracle as O
    ei, ea, geo = _graph()
    ref = O.GConvLSTM(cin, h, L, 'TransformerConv')
    _init(ref)
    ref.double().eval()
    gen = torch.Generator().manual_seed(7)
    N = geo.N
    X, H, C = (torch.randn(N, w, generator=gen, dtype=torch.float64) for w in (cin, h, h))
    gs = [torch.randn(N, h, generator=gen, dtype=torch.float64) for _ in range(3)]
    xr = X.clone().requires_grad_(True)
    hr, cr = (H.clone().requires_grad_(True), C.clone().requires_grad_(True)) if with_state else (None, None)
    ins_r = [xr] + ([hr, cr] if with_state else []) + list(ref.parameters())
    with _float64():
        outs_r = ref(xr, ei, ea, hr, cr)
        gr = torch.autograd.grad(outs_r, ins_r, gs, allow_unused=True)

    params = tcell_f64.leaves(ref.state_dict())
    assert list(params) == [k for k, _ in ref.named_parameters()]
    xm = tcell_f64.leaf(X)
    hm, cm = (tcell_f64.leaf(H), tcell_f64.leaf(C)) if with_state else (None, None)
    r = tcell_f64.cell(params, geo, xm, hm, cm, h)
    ins_m = [xm] + ([hm, cm] if with_state else []) + list(params.values())
    gm = torch.autograd.grad([r.O, r.H, r.C], ins_m, gs, allow_unused=True)
    names = ['X'] + (['H', 'C'] if with_state else []) + list(params)
    for a, b, nm in zip((r.O, r.H, r.C), outs_r, ('O', "H'", "C'")):
        _same(a, b, nm)
    assert len(gm) == len(gr) == len(names)
    for a, b, nm in zip(gm, gr, names):
        assert a is not None and b is not None, nm
        _same(a, b, nm)
    live = [nm for a, nm in zip(gm, names) if float(a.abs().max()) > 1e-6]
    assert 'X' in live and any(n.endswith('lin_edge.weight') for n in live) and any(n.endswith('lin_query.weight') for n in live)
    # T = 1 of the chain is the single update
    s = tcell_f64.steps(params, geo, [xm], hm, cm, h)
    assert len(s) == 1 and all(torch.equal(getattr(s[0], k), getattr(r, k)) for k in ('O', 'H', 'C'))


def _stack_by_stack(params, geo, X, H, C, h, keep, epoch, seeds):
    """The model's forward with every stack evaluated on its own, one head per attention_f64 call, stack g of layer l under the seed
    (seed_l + g 0x632BE5AB) mod 2^32 -- the head offset of attn_f64.dropout_mask."""
    L = tcell_f64.n_layers(params)
    outs, mults = {}, {}
    with torch.no_grad():
        for g, name in enumerate(f'{br}_{gt}' for br in ('conv_x', 'conv_h') for gt in 'ifco'):
            x = X if name.startswith('conv_x') else H
            for l in range(L):
                lin = lambda n: x @ params[f'{name}.convolutions.{l}.{n}.weight'].T + params[f'{name}.convolutions.{l}.{n}.bias']
                proj = torch.cat([lin('lin_query'), lin('lin_key'), lin('lin_value'), lin('lin_skip')], dim=1)
                We = params[f'{name}.convolutions.{l}.lin_edge.weight']
                r = attention_f64(geo.rowptr, geo.col, geo.selfpair, geo.eattr, proj.numpy(), We.detach().numpy(), h, 1, keep,
                                  (seeds[l] + g * 0x632BE5AB) & 0xFFFFFFFF, epoch)
                x = r.out.detach()
                mults[g, l] = r.mult[:, 0]
            outs[name] = x
        p = {k: v.detach() for k, v in params.items()}
        gate = lambda n: outs['conv_x_' + n] + outs['conv_h_' + n]
        I = torch.sigmoid(gate('i') + p['w_c_i'] * C + p['b_i'])
        F = torch.sigmoid(gate('f') + p['w_c_f'] * C + p['b_f'])
        Cn = F * C + I * torch.tanh(gate('c') + p['b_c'])
        O = torch.sigmoid(gate('o') + p['w_c_o'] * Cn + p['b_o'])
    return (O, O * torch.tanh(Cn), Cn), mults


@pytest.mark.parametrize('keep', [0.9, 0.5])
def test_dropout_masks_follow_the_head_order(keep):
    """keep < 1 at (cin, h, L) = (5, 8, 3): the eight-head model equals the stack-by-stack evaluation with per-stack seeds, mask by
    mask and in (O, H', C'); two epochs draw different masks; the kept share of all pairs is within 3 sigma of keep."""
    from oracle import qt_oracle as O
    _, _, geo = _graph()
    cin, h, L = 5, 8, 3
    ref = O.GConvLSTM(cin, h, L, 'TransformerConv')
    _init(ref)
    params = tcell_f64.leaves(ref.state_dict())
    gen = torch.Generator().manual_seed(9)
    X, H, C = (torch.randn(geo.N, w, generator=gen, dtype=torch.float64) for w in (cin, h, h))
    seeds = [0xDEADBEEF, 1234, 2654435768]
    r = tcell_f64.cell(params, geo, X, H, C, h, keep=keep, epoch=3, seeds=seeds)
    (O2, H2, C2), mults = _stack_by_stack(params, geo, X, H, C, h, keep, 3, seeds)
    for a, b, nm in zip((r.O, r.H, r.C), (O2, H2, C2), ('O', "H'", "C'")):
        _same(a, b, nm, rel=1e-12)
    for l in range(L):
        for g in range(8):
            assert torch.equal(r.attn[l].mult[:, g], mults[g, l]), (l, g)
        assert any(not torch.equal(r.attn[l].mult[:, 0], r.attn[l].mult[:, g]) for g in range(1, 8))
    nxt = tcell_f64.cell(params, geo, X, H, C, h, keep=keep, epoch=4, seeds=seeds)
    assert all(not torch.equal(a.mult, b.mult) for a, b in zip(r.attn, nxt.attn))
    assert not torch.equal(r.O, nxt.O)
    kept = torch.cat([(a.mult > 0).reshape(-1) for a in r.attn]).double()
    assert abs(float(kept.mean()) - keep) <= 3 * (keep * (1 - keep) / kept.numel()) ** 0.5, float(kept.mean())
    full = tcell_f64.cell(params, geo, X, H, C, h)
    assert all(bool((a.mult == 1).all()) for a in full.attn) and not torch.equal(full.O, r.O)


def test_float32_model_runs_the_same_statements():
    """dtype = float32: the same update in single precision, within 1e-4 of the float64 one and not equal to it."""
    from oracle import qt_oracle as O
    _, _, geo = _graph()
    cin, h, L = 4, 8, 2
    ref = O.GConvLSTM(cin, h, L, 'TransformerConv')
    _init(ref)
    gen = torch.Generator().manual_seed(5)
    X, H, C = (torch.randn(geo.N, w, generator=gen) for w in (cin, h, h))
    res = {}
    for dt in (torch.float64, torch.float32):
        params = tcell_f64.leaves(ref.state_dict(), dt)
        x, hh, cc = (tcell_f64.leaf(t, dt) for t in (X, H, C))
        r = tcell_f64.cell(params, geo, x, hh, cc, h, dtype=dt)
        assert r.O.dtype == dt and r.pre[0].dtype == dt
        g = torch.autograd.grad([r.O, r.H, r.C], [x, params['conv_h_f.convolutions.1.lin_value.weight']], [torch.ones_like(r.O)] * 3)
        res[dt] = [r.O, r.H, r.C, *g]
    for a, b in zip(res[torch.float32], res[torch.float64]):
        a, b = a.detach(), b.detach()
        err = float((a.double() - b).abs().max()) / float(b.abs().max())
        assert 0 < err < 1e-4, err
