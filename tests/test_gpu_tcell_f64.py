"""The TransformerConv LSTM cell as every TransformerConv model trains through it -- GConvLSTM.step -> ops.multi_conv (qt_proj_group,
qt_attn_fwd / qt_attn_bwd with 8 heads, qt_proj_bwd or the deferred qt_wgrad_groups) -> ops.lstm_cell -- against the float64 model
tests/tcell_f64.py: (O, H', C') and the gradients of X, H, C, every parameter by name and the LayerNorm parameters, at every lane
width, depth and input width, on the meshes of tests/test_gpu_attn_f64.py and a two-node mesh, over chained uses of one pack, under
partial differentiation, and in training mode with the dropout masks the specification gives every stack of every layer.

Bounds (the reference is float64, so all of the error is the GPU path's): outputs helpers.close with its defaults, gradients
helpers.grad_close with its defaults per tensor.  The one exception is the gradient of lin_key.bias, an exact zero (a shift of every
key moves all scores of a target equally), so that both sides hold rounding noise: per case (over its key-bias tensors and its
cotangent steps) the float32 run of the model is measured against the float64 one and the GPU is allowed 4 x that magnitude
(another summation order over 64-row tiles and per-workgroup slabs).  Every case prints its worst error / bound ratios before it asserts (profiles/tcell_f64.txt: a recorded run).
The launch names each case asserts say which branch served it."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tcell_f64
import test_gpu_attn_f64 as A
from helpers import ATOL, RTOL, close, dev, grad_close
from test_gpu_cell_oracle import _assert_live

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
STEP = 2654435761                       # (the seed of attention launch number k is k STEP + torch.initial_seed() mod 2^32)
pad4 = lambda v: v + (-v) % 4


# ------------------------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    if kind == 'single':                # two constant clips: each is ONE 64 x 64 node, no stored edge, only the self pair
        from qtmpnn.mesh import build_mesh
        return build_mesh(src=torch.zeros(2, 64, 64, device=dev()), thresh=A.THRESH)
    return A._mesh(kind)


@functools.lru_cache(maxsize=None)
def _geo(kind):
    if kind != 'single':
        return A._geo(kind)
    mesh = _mesh(kind)
    _, selfpair, eattr, _ = mesh.attn_geometry()
    N = mesh.N
    return SimpleNamespace(N=N, E=0, cap=N, rowptr=mesh.rowptr[:N + 1].cpu().numpy(), col=np.zeros(0, np.int32),
                           eattr=np.zeros((0, 2), np.float32), selfpair=selfpair[:N].cpu().numpy())


def _props(kind, h):
    """What each mesh is for (asserted, so that a change of the constructors cannot empty a case)."""
    geo, mesh = _geo(kind), _mesh(kind)
    if kind == 'S':
        assert geo.N == 138 and geo.N % 64 == 10            # ragged; the last 64-row tile of qt_proj_bwd has 10 rows
        if h <= 32:
            assert A._blocks(geo.N, h) < 8, (geo.N, h)       # the unsplit source sweep
    elif kind in ('D', 'T'):
        A._assert_kind(kind, h)     # rows of >= 32 edges, nodes with and without a self pair, >= 8 workgroups; T: static, N < capacity
        if kind == 'T':
            assert mesh.n_dev is not None and mesh.N == 3 * 4096 > geo.N
    elif kind == 'P':
        assert geo.selfpair is None and mesh.pixelwise
    else:
        assert geo.N == 2 and int(geo.rowptr[-1]) == 0 and bool((geo.selfpair > 0).all())
    return geo, mesh


# ------------------------------------------------------------------------------------------------------------------ launches
class _Launches:
    def __init__(self):
        self.calls = []

    def clear(self):
        self.calls.clear()

    def names(self, start=0):
        return [n for n, _ in self.calls[start:]]

    def args(self, name, start=0):
        return [a for n, a in self.calls[start:] if n == name]


@pytest.fixture
def launched(monkeypatch):
    from qtmpnn import _lib
    rec, call = _Launches(), _lib.call

    def wrapped(name, *a):
        rec.calls.append((name, a))
        return call(name, *a)
    monkeypatch.setattr(_lib, 'call', wrapped)
    return rec


def _expect_forward(fwd, L):
    """Per layer one projection launch per input segment (layer 0 has two) and ONE attention launch of 8 heads, then the cell."""
    assert fwd.count('qt_attn_fwd') == L and fwd.count('qt_proj_group') == L + 1, fwd
    assert fwd.count('qt_lstm_fwd') == 1 and 'qt_dense_lstm' not in fwd and 'qt_mhattn_fwd' not in fwd, fwd


def _expect_attention_backward(rec, nf, L, h, alias_before):
    """qt_attn_bwd per layer, last layer first: the summed pair (gmod = 4 of G = 8, rows (N, 2, 4C)), then L - 1 inner layers that
    complete the gradient array the layer above started (accumulate bit 1, _STATS['skip_alias'])."""
    from qtmpnn import ops
    ab = rec.args('qt_attn_bwd', nf)
    assert len(ab) == L, rec.names(nf)
    assert ab[0][26] == 8 and ab[0][27] == 4 and ab[0][19] == 8 * h and not ab[0][22] & 2, ab[0][16:]
    for a in ab[1:]:
        assert a[26] == 8 and a[27] == 8 and a[22] & 2, a[16:]
    assert ops._STATS['skip_alias'] == alias_before + L - 1


def _expect_projection_backward(rec, nf, L, h, cin, with_state, x_grad=True):
    """Which launch serves each input segment's backward: the one-pass qt_proj_bwd where cin = C = 32 and the input needs a gradient,
    else the data gradient by qt_proj_group and the weight gradient by the deferred qt_wgrad_groups."""
    bwd = rec.names(nf)
    n_pb, n_wg = bwd.count('qt_proj_bwd'), bwd.count('qt_wgrad_groups')
    if h != 32:
        assert n_pb == 0 and n_wg == L + 1, bwd
        return
    fused = (L - 1) + int(with_state) + int(pad4(cin) == 32 and x_grad)
    assert n_pb == fused and n_wg == L + 1 - fused, (n_pb, n_wg, bwd)


# ------------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _state(cin, h, L, s=0.7):
    """A cell's state dict: weights N(0, s / sqrt(fan_in)), lin_edge 0.3, peepholes 0.5, biases 0.2 (live gates: _assert_live)."""
    from model.model import GConvLSTM
    cell = GConvLSTM(cin, h, L, 'TransformerConv')
    gen = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for name, p in cell.named_parameters():
            sd = 0.3 if name.endswith('lin_edge.weight') else s * p.shape[1] ** -0.5 if name.endswith('weight') else \
                0.5 if name.startswith('w_c_') else 0.2
            p.copy_(torch.randn(p.shape, generator=gen) * sd)
    return {k: v.detach().clone() for k, v in cell.state_dict().items()}


def _cell(cin, h, L, train=False, dropout=None):
    from model.model import GConvLSTM
    mine = GConvLSTM(cin, h, L, 'TransformerConv')
    mine.load_state_dict(_state(cin, h, L))
    mine.to(dev())
    mine.train(train)
    if dropout is not None:
        for c in mine._convs():
            c.dropout = dropout
    assert mine._layer_by_layer
    return mine


def _inputs(N, cin, h, seed=7, T=1):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    X, H, C = [r(N, cin) for _ in range(T)], r(N, h), r(N, h)
    LN = torch.stack([1 + 0.3 * r(h), 0.3 * r(h), 1 + 0.3 * r(h), 0.3 * r(h)])
    gs = [r(N, h) for _ in range(T + 2)]
    return (X[0] if T == 1 else X), H, C, LN, gs


def _model(dt, cin, h, L, geo, X, H, C, LN, keep=1.0, epoch=0, seeds=None):
    """The model's update at dtype `dt` with its leaves; normed: (O, layer_norm(H'), layer_norm(C')) on the same graph."""
    params = tcell_f64.leaves(_state(cin, h, L), dt)
    x, hh, cc, ln = (tcell_f64.leaf(t, dt) for t in (X, H, C, LN))
    r = tcell_f64.cell(params, geo, x, hh, cc, h, None, keep, epoch, seeds, dt)
    return SimpleNamespace(r=r, params=params, x=x, h=hh, c=cc, ln=ln, plain=(r.O, r.H, r.C),
                           normed=(r.O,) + tuple(tcell_f64.layer_norms(r.H, r.C, ln)))


def _model_grads(m, step, gs):
    dt = m.x.dtype
    outs = m.normed if step == 'layernorm' else m.plain
    ins = [m.x] + ([m.h, m.c] if m.h is not None else []) + list(m.params.values()) + ([m.ln] if step == 'layernorm' else [])
    if step == 'h_only':
        outs, gs = outs[1:2], gs[1:2]
    grads = torch.autograd.grad(outs, ins, [g.to(dt) for g in gs[:len(outs)]], retain_graph=True, allow_unused=True)
    return [o.detach() for o in outs], list(grads)


def _names(m, step):
    return ['X'] + (['H', 'C'] if m.h is not None else []) + list(m.params) + (['ln'] if step == 'layernorm' else [])


def _gpu_update(mine, mesh, cin, X, H, C, LN, gs, step, rec):
    """One update on the device, the rows above the valid ones (a static mesh's capacity) filled with NaN in every operand and
    cotangent.  -> (outs, grads, first launch index of the backward)."""
    put = lambda t: None if t is None else A._pad(t, mesh.N).requires_grad_(True)
    xg, hg, cg = put(X), put(H), put(C)
    rec.clear()
    if step == 'layernorm':
        lng = LN.to(dev()).requires_grad_(True)
        xp = torch.nn.functional.pad(xg, (0, pad4(cin) - cin))
        outs = mine.step(xp, mesh, hg, cg, mine.pack(pad4(cin), lng, (True,))[0])
    else:
        outs = mine(xg, mesh, None, hg, cg)
    nf = len(rec.calls)
    ins = [xg] + ([hg, cg] if hg is not None else []) + list(mine.parameters()) + ([lng] if step == 'layernorm' else [])
    if step == 'h_only':
        outs, gs = outs[1:2], gs[1:2]
    grads = torch.autograd.grad(outs, ins, [A._pad(g, mesh.N) for g in gs[:len(outs)]], allow_unused=True)
    torch.cuda.synchronize()
    return list(outs), list(grads), nf


# ------------------------------------------------------------------------------------------------------------------ checks
KINDS = ('lin_key.weight', 'lin_query.weight', 'lin_query.bias', 'lin_value.weight', 'lin_value.bias', 'lin_edge.weight',
         'lin_skip.weight', 'lin_skip.bias', 'w_c', 'b')


def _kind(name):
    for k in KINDS[:-2]:
        if name.endswith(k):
            return k
    return 'w_c' if name.startswith('w_c_') else 'b' if name.startswith('b_') else name


def _out_ratio(a, b):
    return float(((a - b).abs() / (ATOL + RTOL * b.abs())).max())


def _kb_noise(names, grads_r, grads_32):
    """The largest |float32 model - float64 model| over the key-bias gradients (exact zeros: both are rounding noise)."""
    return max(float((g32.double() - g64).abs().max()) for n, g64, g32 in zip(names, grads_r, grads_32) if n.endswith('lin_key.bias'))


def _check(tag, N, out_names, outs_g, outs_r, names, grads_g, grads_r, grads_32, kb_mag=None):
    """Print the worst error / bound ratio per output, per input and per kind of parameter (over the stacks and layers), and the
    key-bias noise with its measured float32 magnitude; then assert every tensor on its own."""
    fig, fails = [], []
    for a, b, nm in zip(outs_g, outs_r, out_names):
        a = a[:N].detach().double().cpu()
        assert not torch.isnan(a).any(), f'{tag}: NaN in a valid row of {nm}'
        fig.append((nm, _out_ratio(a, b)))
    kb = [i for i, n in enumerate(names) if n.endswith('lin_key.bias')]
    kb_mag = _kb_noise(names, grads_r, grads_32) if kb_mag is None else kb_mag      # (a case of several steps: the case's largest)
    kb_err = 0.0
    worst = {}
    for i, (a, r, nm) in enumerate(zip(grads_g, grads_r, names)):
        if a is None:       # a parameter the HIP path leaves untouched must have an exactly-zero reference gradient
            assert r is None or not r.any(), f'{tag} {nm}: no gradient on the HIP path, reference max {float(r.abs().max())}'
            continue
        a = (a[:N] if a.shape[0] != r.shape[0] else a).detach().double().cpu()
        assert not torch.isnan(a).any(), f'{tag}: NaN in the gradient of {nm}'
        if i in kb:
            kb_err = max(kb_err, float((a - r).abs().max()))
            continue
        ratio = A._grad_ratio(a, r)
        k = _kind(nm)
        worst[k] = max(worst.get(k, 0.0), ratio)
        if ratio > 1.0:
            fails.append(f'{nm}: {ratio:.3g} x the grad_close bound (the float32 model: {A._grad_ratio(grads_32[i], r):.3g} x)')
    fig += sorted(worst.items(), key=lambda kv: (kv[0] not in ('X', 'H', 'C'), kv[0]))
    fig.append(('key_bias', 0.0 if kb_err == 0 else kb_err / (4 * kb_mag) if kb_mag > 0 else float('inf')))
    print(f'tcell_f64 {tag}: ' + ' '.join(f'{n}={v:.3g}' for n, v in fig) + f' key_bias_f32={kb_mag:.3g}')
    for a, b, nm in zip(outs_g, outs_r, out_names):
        close(a[:N], b, msg=f'{tag} {nm}')
    assert not fails, f'{tag}: ' + '; '.join(fails)
    for i, (a, r, nm) in enumerate(zip(grads_g, grads_r, names)):
        if a is not None and i not in kb:
            grad_close(a[:N] if a.shape[0] != r.shape[0] else a, r, msg=f'{tag} {nm}')
    assert kb_err <= 4 * kb_mag, f'{tag}: key-bias gradient noise {kb_err:.3g}, 4 x the float32 model\'s is {4 * kb_mag:.3g}'


# ------------------------------------------------------------------------------------------------------------------ one update
# (id, mesh, cin, hidden, layers, also the first step H = C = None)
CASES = [(f'width-h{h}', 'S', 4, h, 2, False) for h in (8, 16, 32, 64)] + [('width-h128', 'S', 4, 128, 1, False)]
CASES += [(f'depth-L{L}', 'D', 4, 8, L, False) for L in (1, 2, 3)]
CASES += [(f'cin{c}', 'D', c, 8, 2, False) for c in (1, 5, 6)]
CASES += [(f'h32-{k}-cin{c}', k, c, 32, 3, k in ('S', 'D')) for k in ('S', 'D', 'T', 'P', 'single') for c in (5, 32)]


@pytest.mark.parametrize('kind,cin,h,L,first', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_cell_update_vs_float64_model(kind, cin, h, L, first, launched):
    """Forward and every gradient under random cotangents on (O, H', C') (`full`), on H' alone (`h_only`: gO, gC' arrive as None),
    with the fused LayerNorm (`layernorm`: step() with one pack), and from no state (`first`) where flagged.

    On the two-node mesh every target has one pair, alpha = 1, so the gradients of lin_query and lin_key (weights and biases) are
    exact zeros, in the float32 model too (its key-bias yardstick is 0): the kernels must return exact zeros there."""
    from qtmpnn import ops
    geo, mesh = _props(kind, h)
    N = geo.N
    X, H, C, LN, gs = _inputs(N, cin, h)
    mine = _cell(cin, h, L)
    assert pad4(cin) == {1: 4, 4: 4, 5: 8, 6: 8, 32: 32}[cin]
    for with_state in (True, False) if first else (True,):
        hs, cs = (H, C) if with_state else (None, None)
        m64, m32 = (_model(dt, cin, h, L, geo, X, hs, cs, LN) for dt in (torch.float64, torch.float32))
        if with_state:
            _assert_live(m64.r.pre)
        steps = ('full', 'h_only', 'layernorm') if with_state else ('first',)
        ref = {step: (_model_grads(m64, step, gs), _model_grads(m32, step, gs)[1]) for step in steps}
        kb_mag = max(_kb_noise(_names(m64, step), ref[step][0][1], ref[step][1]) for step in steps)
        for step in steps:
            (outs_r, grads_r), grads_32 = ref[step]
            alias = ops._STATS['skip_alias']
            outs_g, grads_g, nf = _gpu_update(mine, mesh, cin, X, hs, cs, LN, gs, step, launched)
            _expect_forward(launched.names()[:nf], L)
            _expect_attention_backward(launched, nf, L, h, alias)
            _expect_projection_backward(launched, nf, L, h, cin, with_state)
            _check(f'{kind} cin={cin} h={h} L={L} {step}', N, ("H'",) if step == 'h_only' else ('O', "H'", "C'"), outs_g, outs_r,
                   _names(m64, step), grads_g, grads_r, grads_32, kb_mag)


def test_hidden_4_is_refused_by_the_cell_kernel():
    """Hidden 4 is a lane-group width of the attention kernels only: qt_lstm_fwd takes 8, 16, 32, 64 or 128 and says so (no case of
    this file can run a hidden-4 cell)."""
    geo, mesh = _props('S', 4)
    X, H, C, _, _ = _inputs(geo.N, 4, 4)
    with pytest.raises(RuntimeError, match='hidden size must be 8, 16, 32, 64 or 128'):
        _cell(4, 4, 2)(X.to(dev()).requires_grad_(True), mesh, None, H.to(dev()), C.to(dev()))


# ------------------------------------------------------------------------------------------------------------------ chained uses
@pytest.mark.parametrize('start', ['none', 'state'])
@pytest.mark.parametrize('h', [32, 8])
@pytest.mark.parametrize('kind', ['S', 'T'])
def test_three_chained_uses_of_one_pack(kind, h, start, launched):
    """T = 3 updates with one pack (the GradAcc slabs of every layer and of the cell serve all three uses), cotangents on every O and
    on the last H', C', one backward.  start = none: H = C = None, X_t is data; state: H, C given and X_t needs a gradient.
    Hidden 32 from no state: the H segment of layer 0 is deferred at step 1 (its zero state needs no gradient) and fused at steps 2
    and 3, so its weight gradient is the sum of the qt_proj_bwd slabs and a one-use qt_wgrad_groups launch."""
    from qtmpnn import ops
    cin, L, T = 5, 3, 3
    geo, mesh = _props(kind, h)
    N = geo.N
    Xs, H, C, _, gs = _inputs(N, cin, h, seed=21, T=T)
    with_state = start == 'state'
    hs, cs = (H, C) if with_state else (None, None)
    refs = {}
    for dt in (torch.float64, torch.float32):
        params = tcell_f64.leaves(_state(cin, h, L), dt)
        xs = [tcell_f64.leaf(x, dt, grad=with_state) for x in Xs]
        h0, c0 = tcell_f64.leaf(hs, dt), tcell_f64.leaf(cs, dt)
        rs = tcell_f64.steps(params, geo, xs, h0, c0, h, dtype=dt)
        outs = [r.O for r in rs] + [rs[-1].H, rs[-1].C]
        ins = (xs + [h0, c0] if with_state else []) + list(params.values())
        grads = torch.autograd.grad(outs, ins, [g.to(dt) for g in gs], allow_unused=True)
        refs[dt] = ([o.detach() for o in outs], list(grads))
    names = ([f'X{t}' for t in range(T)] + ['H', 'C'] if with_state else []) + list(params)

    mine = _cell(cin, h, L)
    put = lambda t, grad: None if t is None else A._pad(t, mesh.N).requires_grad_(grad)
    xg, hg, cg = [put(x, with_state) for x in Xs], put(hs, True), put(cs, True)
    alias = ops._STATS['skip_alias']
    launched.clear()
    pk = mine.pack(pad4(cin), None, (True,))[0]
    Os, Hc, Cc = [], hg, cg
    for x in xg:
        o, Hc, Cc = mine.step(torch.nn.functional.pad(x, (0, pad4(cin) - cin)), mesh, Hc, Cc, pk)
        Os.append(o)
    nf = len(launched.calls)
    outs_g = Os + [Hc, Cc]
    ins_g = (xg + [hg, cg] if with_state else []) + list(mine.parameters())
    grads_g = torch.autograd.grad(outs_g, ins_g, [A._pad(g, mesh.N) for g in gs], allow_unused=True)
    torch.cuda.synchronize()
    assert ops._STATS['skip_alias'] == alias + T * (L - 1)
    bwd = launched.names(nf)
    uses = [a[0] for a in launched.args('qt_wgrad_groups', nf)]
    if h == 32 and not with_state:      # steps 3, 2: H segment + 2 layers fused; step 1: the 2 deeper layers; X (cin 8) always deferred
        assert bwd.count('qt_proj_bwd') == 2 * L + (L - 1) and uses == [T, 1], (bwd.count('qt_proj_bwd'), uses)
    elif h == 32:
        assert bwd.count('qt_proj_bwd') == T * L and uses == [T], (bwd.count('qt_proj_bwd'), uses)
    else:
        assert 'qt_proj_bwd' not in bwd and uses == [T] * (L + 1), uses
    _check(f'chain T=3 {kind} h={h} start={start}', N, [f'O{t}' for t in range(T)] + ["H'", "C'"], outs_g, refs[torch.float64][0],
           names, list(grads_g), refs[torch.float64][1], refs[torch.float32][1])


# ------------------------------------------------------------------------------------------------------------------ partial differentiation
def test_parameters_frozen_input_gradients_only(launched):
    """Mesh S, hidden 32, two layers, every parameter without a gradient: the input gradients match, no weight-gradient launch and no
    reduction runs (the early returns), and the backward can run twice with the same bits."""
    cin, h, L = 5, 32, 2
    geo, mesh = _props('S', h)
    X, H, C, LN, gs = _inputs(geo.N, cin, h)
    m64, m32 = (_model(dt, cin, h, L, geo, X, H, C, LN) for dt in (torch.float64, torch.float32))
    outs_r, grads_r = _model_grads(m64, 'full', gs)
    _, grads_32 = _model_grads(m32, 'full', gs)
    mine = _cell(cin, h, L)
    for p in mine.parameters():
        p.requires_grad_(False)
    xg, hg, cg = (t.to(dev()).requires_grad_(True) for t in (X, H, C))
    launched.clear()
    outs_g = mine(xg, mesh, None, hg, cg)
    nf = len(launched.calls)
    gg = [g.to(dev()) for g in gs]
    first = torch.autograd.grad(outs_g, [xg, hg, cg], gg, retain_graph=True)
    bwd = launched.names(nf)
    assert 'qt_proj_bwd' not in bwd and 'qt_wgrad_groups' not in bwd and 'qt_colsum' not in bwd, bwd
    assert bwd.count('qt_proj_group') == L + 1 and bwd.count('qt_attn_bwd') == L, bwd
    second = torch.autograd.grad(outs_g, [xg, hg, cg], gg)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    fig = [(nm, A._grad_ratio(a, r)) for a, r, nm in zip(first, grads_r[:3], 'XHC')]
    print('tcell_f64 frozen parameters S cin=5 h=32 L=2: ' + ' '.join(f'{n}={v:.3g}' for n, v in fig))
    for a, b, nm in zip(outs_g, outs_r, ('O', "H'", "C'")):
        close(a, b, msg=nm)
    for a, r, nm in zip(first, grads_r[:3], 'XHC'):
        grad_close(a, r, msg=nm)


def test_weights_only_no_input_gradients(launched):
    """Mesh S, hidden 32, two layers, X, H, C without gradients: layer 0 computes no data gradient (no qt_proj_group in the backward)
    and both its segments go to the deferred qt_wgrad_groups; every weight gradient matches.  The only qt_proj_bwd launch is layer
    1's (8 groups): its input is layer 0's output, whose gradient layer 0's weights need -- no launch serves a segment of layer 0."""
    cin, h, L = 5, 32, 2
    geo, mesh = _props('S', h)
    N = geo.N
    X, H, C, LN, gs = _inputs(N, cin, h)
    m64, m32 = (_model(dt, cin, h, L, geo, X, H, C, LN) for dt in (torch.float64, torch.float32))
    outs_r, grads_r = _model_grads(m64, 'full', gs)
    _, grads_32 = _model_grads(m32, 'full', gs)
    mine = _cell(cin, h, L)
    launched.clear()
    outs_g = mine(X.to(dev()), mesh, None, H.to(dev()), C.to(dev()))
    nf = len(launched.calls)
    grads_g = torch.autograd.grad(outs_g, list(mine.parameters()), [g.to(dev()) for g in gs], allow_unused=True)
    bwd = launched.names(nf)
    pb = launched.args('qt_proj_bwd', nf)
    assert len(pb) == L - 1 and all(a[-5] == 8 for a in pb), (len(pb), [a[-5] for a in pb])
    assert 'qt_proj_group' not in bwd and [a[0] for a in launched.args('qt_wgrad_groups', nf)] == [1, 1], bwd
    _check('weights only S cin=5 h=32 L=2', N, ('O', "H'", "C'"), list(outs_g), outs_r, list(m64.params), list(grads_g), grads_r[3:],
           grads_32[3:])


# ------------------------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize('keep', [0.9, 0.5])
@pytest.mark.parametrize('h', [8, 32])
@pytest.mark.parametrize('kind', ['S', 'D'])
def test_training_mode_draws_the_specified_masks(kind, h, keep, launched):
    """mine.train(): layer l of the step is attention launch number calls + 1 + l, so its seed is (calls + 1 + l) STEP + initial_seed
    mod 2^32, head g of that launch is stack g, and the epoch is the device counter.  Outputs and all gradients match the model with
    those masks; a second step after advance_dropout_epoch matches the model at epoch + 1 and differs from the first."""
    from qtmpnn import ops
    cin, L, epoch = 5, 3, 5
    geo, mesh = _props(kind, h)
    N = geo.N
    X, H, C, LN, gs = _inputs(N, cin, h, seed=31)
    mine = _cell(cin, h, L, train=True, dropout=None if keep == 0.9 else 0.5)
    assert mine.conv_x_i.convolutions[0].dropout == (0.1 if keep == 0.9 else 0.5)
    keep = 1.0 - mine.conv_x_i.convolutions[0].dropout
    ep = ops.dropout_epoch(dev())
    saved = int(ep.item())
    results = []
    try:
        ep.fill_(epoch)
        for k in range(2):
            calls, s0 = ops._ATTN_CALLS[0], int(torch.initial_seed())
            seeds = [((calls + 1 + l) * STEP + s0) & M32 for l in range(L)]
            outs_g, grads_g, nf = _gpu_update(mine, mesh, cin, X, H, C, LN, gs, 'full', launched)
            assert ops._ATTN_CALLS[0] == calls + L and int(ep.item()) == epoch + k
            fwd_args = launched.args('qt_attn_fwd')
            assert [a[13] for a in fwd_args] == seeds and all(abs(a[12] - keep) < 1e-12 for a in fwd_args)
            m64, m32 = (_model(dt, cin, h, L, geo, X, H, C, LN, keep, epoch + k, seeds) for dt in (torch.float64, torch.float32))
            outs_r, grads_r = _model_grads(m64, 'full', gs)
            _, grads_32 = _model_grads(m32, 'full', gs)
            for l, a in enumerate(m64.r.attn):
                kept = (a.mult > 0)
                assert torch.equal(kept, m32.r.attn[l].mult > 0)
                if kind == 'D':
                    assert bool(kept.any(dim=0).all()) and bool((~kept).any(dim=0).all()), f'layer {l}: a head kept or dropped every pair'
            _check(f'dropout {kind} h={h} keep={keep:.1f} epoch={epoch + k}', N, ('O', "H'", "C'"), outs_g, outs_r, _names(m64, 'full'),
                   grads_g, grads_r, grads_32)
            results.append((outs_g, [a.mult for a in m64.r.attn]))
            ops.advance_dropout_epoch(dev())
    finally:
        ep.fill_(saved)
    assert all(not torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))
    assert not torch.allclose(results[0][0][1], results[1][0][1], rtol=1e-3, atol=1e-4)
