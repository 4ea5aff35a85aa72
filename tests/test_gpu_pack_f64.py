"""Weight-space composition -- qt_compose_step_fwd / _bwd, qt_compose2_fwd / _bwd (csrc/pack.hip) through ops._ComposeStep,
ops._Compose2, ops.compose_pack and the raw C ABI -- and clip + Adam on the flat vector -- qt_flat_adam through optim.FlatAdam and
the raw ABI -- against the float64 model tests/pack_f64.py.

Every comparison is kernel against model, never kernel against kernel.  Exact composition cases draw every operand and cotangent
from {-2, -1, 1, 2}: every partial sum of ONE product is a half-integer far below 2^24, the bound is 0 and W, WT (== W.T bit for
bit), P, B and all eight gradients equal the model entry for entry; the products of a deeper stack are therefore run one by one
on fresh operands at the (Ka, Kb0) the stack reaches (pack_f64.stages), and ops.compose_pack end to end where the whole stack
stays exact (pack_f64.stack_exact), else real-valued with the folded series' inherited error.  Real cases draw
sign * (0.5 + U[0, 1)) and use the bounds derived beside the model.  Outputs of raw ABI calls are pre-filled with the sentinel
-7.25 (never a half-integer: an unwritten element fails the exact comparison).  Adam compares one step at a time from float32
inputs against pack_f64.adam_step with pack_f64.adam_bound; step counts are reached by writing t - 1 into the device counter.
Every case prints its worst error / bound before it asserts (pytest -s; a recorded run: profiles/head_pack_f64.txt).
tests/test_pack_f64_host.py names, per mutation, the case here that sees it."""
import numpy as np
import pytest
import torch

import pack_f64 as M
from helpers import dev
from test_gpu_cheb_f64 import compare

pytestmark = pytest.mark.gpu

SENT = -7.25
WORST = {}
ENTRIES = []
GRADS = ('gP0', 'gB0', 'gP1', 'gB1')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


def check(family, name, got, ref, bound=0.0):
    ratio = compare(got, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f'  [{family}] {name}: {ratio:.3g}')
    assert ratio <= 1.0, f'{family} {name}: worst error / bound = {ratio:.4g}'
    return ratio


def call(name, *args):
    from qtmpnn import _lib
    ENTRIES.append(name)
    _lib.call(name, *args)


def p(t):
    return None if t is None else t.data_ptr()


def filled(*shape):
    return torch.full(shape, SENT, device=dev())


@pytest.fixture
def recording(monkeypatch):
    from qtmpnn import _lib
    names, inner = [], _lib.call

    def rec(name, *a):
        names.append(name)
        ENTRIES.append(name)
        return inner(name, *a)
    monkeypatch.setattr(_lib, 'call', rec)
    return names


# ----------------------------------------------------------------------------------------------------- 1. single products
def run_step(kind, tag, b, rng, raw):
    """One natural-layout product, forward and backward, through ops._ComposeStep or the raw ABI."""
    from qtmpnn import ops
    gen = M.ints if kind == 'exact' else M.draw
    P, B = M.step_fwd(*b)
    eP, eB = M.step_bounds(*b) if kind == 'real' else (0.0, 0.0)
    gP, gB = gen(rng, *P.shape), gen(rng, *B.shape)
    ref = M.step_bwd(b[0], b[1], b[2], gP, gB)
    bnd = M.step_bwd_bounds(b[0], b[1], b[2], gP, gB) if kind == 'real' else (0.0,) * 4
    d = [_t(a) for a in b]
    _, Ka, cin, h = b[0].shape
    Kb0, K = b[1].shape[1], b[2].shape[1]
    if raw:
        Pd, Bd = filled(*P.shape), filled(*B.shape)
        call('qt_compose_step_fwd', *[p(t) for t in d], Ka, Kb0, K, cin, h, p(Pd), p(Bd))
        outs = [filled(*a.shape) for a in b]
        gPd, gBd = _t(gP), _t(gB)
        call('qt_compose_step_bwd', *[p(t) for t in d], Ka, Kb0, K, cin, h, p(gPd), p(gBd), *[p(t) for t in outs])
    else:
        for t in d:
            t.requires_grad_(True)
        Pd, Bd = ops._ComposeStep.apply(*d)
        outs = torch.autograd.grad([Pd, Bd], d, [_t(gP), _t(gB)])
    fam = f'step {kind}'
    check(fam, f'{tag} P', Pd, P, eP)
    check(fam, f'{tag} B', Bd, B, eB)
    for n, o, r, e in zip(GRADS, outs, ref, bnd):
        check(fam, f'{tag} {n}', o, r, e)


def run_compose2(kind, tag, x, hb, cin_pad, variants, rng, raw):
    """The packed product of both branches, forward (W, WT per variant) and backward (eight gradients)."""
    from qtmpnn import ops
    gen = M.ints if kind == 'exact' else M.draw
    Ws, Es = M.compose2_fwd(x, hb, cin_pad, variants)
    gWs = [gen(rng, *W.shape) for W in Ws]
    g = dict(zip(variants, gWs))
    ref, bnd = M.compose2_bwd(x, hb, cin_pad, g.get(True), g.get(False))
    d = [_t(a) for a in x + hb]
    _, Ka, cin, h = x[0].shape
    Kb0, K = x[1].shape[1], x[2].shape[1]
    if raw:
        W = {v: filled(*Wm.shape) for v, Wm in zip(variants, Ws)}
        WT = {v: filled(*Wm.T.shape) for v, Wm in zip(variants, Ws)}
        call('qt_compose2_fwd', *[p(t) for t in d], Ka, Kb0, K, cin, cin_pad, h, p(W.get(True)), p(W.get(False)), p(WT.get(True)), p(WT.get(False)))
        got, gotT = [W[v] for v in variants], [WT[v] for v in variants]
        outs = [filled(*a.shape) for a in x + hb]
        gd = {v: _t(a) for v, a in g.items()}
        call('qt_compose2_bwd', *[p(t) for t in d], Ka, Kb0, K, cin, cin_pad, h, p(gd.get(True)), p(gd.get(False)), *[p(t) for t in outs])
    else:
        for t in d:
            t.requires_grad_(True)
        res = ops._Compose2.apply(*d, cin_pad, tuple(variants))
        got, gotT = res[:len(variants)], res[len(variants):]
        outs = torch.autograd.grad(list(got), d, [_t(a) for a in gWs])
    fam = f'compose2 {kind}'
    for v, Wg, WTg, Wm, E in zip(variants, got, gotT, Ws, Es):
        check(fam, f'{tag} W[{int(v)}]', Wg, Wm, E if kind == 'real' else 0.0)
        assert torch.equal(WTg, Wg.t()), f'{tag}: WT[{int(v)}] is not W^T bit for bit'
    for n, o, r, e in zip([f'x {n}' for n in GRADS] + [f'h {n}' for n in GRADS], outs, ref, bnd):
        check(fam, f'{tag} {n}', o, r, e if kind == 'real' else 0.0)


@pytest.mark.parametrize('variants', M.VARIANTS)
@pytest.mark.parametrize('shape', M.SHAPES)
@pytest.mark.parametrize('kind', ['exact', 'real'])
def test_products(kind, shape, variants):
    """Every product of the stack `shape` on fresh operands: the natural-layout steps at their (Ka, Kb0) for both branches (with the
    two-variant case only: they do not depend on the variants), the packed product for the variants.  Through the autograd
    wrappers; exact cases also through the raw ABI into sentinel-filled outputs."""
    cin, cin_pad, h, K, L = shape
    gen = M.ints if kind == 'exact' else M.draw
    rng = np.random.default_rng(sum(shape) + len(variants))
    st = M.stages(K, L)
    for raw in ((False, True) if kind == 'exact' else (False,)):
        if len(variants) == 2:
            for Ka, Kb0 in st[:-1]:
                for width in (cin, h):
                    run_step(kind, f'{shape} Ka={Ka} Kb0={Kb0} in={width} raw={int(raw)}', M.branch(gen, rng, Ka, Kb0, K, width, h), rng, raw)
        Ka, Kb0 = st[-1]
        x, hb = M.branch(gen, rng, Ka, Kb0, K, cin, h), M.branch(gen, rng, Ka, Kb0, K, h, h)
        run_compose2(kind, f'{shape} {variants} Ka={Ka} Kb0={Kb0} raw={int(raw)}', x, hb, cin_pad, variants, rng, raw)


# ------------------------------------------------------------------------------------------------- 2. ops.compose_pack
@pytest.mark.parametrize('shape', M.SHAPES)
def test_compose_pack_end_to_end(recording, shape):
    """The whole stack through ops.compose_pack: L - 2 steps per branch and one packed product.  Where the stack stays exact on
    {-2, -1, 1, 2}: W, WT and every layer's gradient entry for entry.  Else (Ka = 29): real-valued operands scaled to keep the
    series O(1), W against the model with the folded series' error carried through |P1| (the gradients of every product of that
    stack are held one by one in test_products)."""
    from qtmpnn import ops
    cin, cin_pad, h, K, L = shape
    rng = np.random.default_rng(sum(shape))
    mk = lambda gen, s: ([gen(rng, 4, K, cin if l == 0 else h, h) * np.float32(s) for l in range(L)], [gen(rng, 4, h) for _ in range(L)],
                         [gen(rng, 4, K, h, h) * np.float32(s) for l in range(L)], [gen(rng, 4, h) for _ in range(L)])
    Px, Bx, Ph, Bh = mk(M.ints, 1.0)
    exact = M.stack_exact(Px, Bx, Ph, Bh)
    if not exact:
        Px, Bx, Ph, Bh = mk(M.draw, 1.0 / (h * K) ** 0.5)
    variants = (True, False)
    flat = [_t(a).requires_grad_(True) for a in Px + Bx + Ph + Bh]
    d = [flat[i * L:(i + 1) * L] for i in range(4)]
    Ws, WTs, Kc, Ksc = ops.compose_pack(*d, cin_pad, variants)
    ref, (sx, sh) = M.stack_pack(Px, Bx, Ph, Bh, cin_pad, variants)
    assert (Kc, Ksc) == (L * (K - 1) + 1, (L - 1) * (K - 1) + 1)
    assert recording.count('qt_compose_step_fwd') == 2 * (L - 2) and recording.count('qt_compose2_fwd') == 1
    bounds = [0.0, 0.0]
    if not exact:
        inh = []
        for Ps, Bs in ((Px, Bx), (Ph, Bh)):                # the folded series' error: every step's own bound + the earlier ones through |P1|
            P, B = M.f64(Ps[0]), M.f64(Bs[0])[:, None]
            eP, eB = 0.0 * P, 0.0 * B
            for Wl, bl in zip(Ps[1:-1], Bs[1:-1]):
                oP, oB = M.step_bounds(P, B, Wl, bl)
                iP, iB = M.step_fwd(eP, eB, Wl, 0.0 * bl, maj=True)
                (P, B), (eP, eB) = M.step_fwd(P, B, Wl, bl), (oP + iP, oB + iB)
            inh.append(M.step_fwd(eP, eB, Ps[-1], 0.0 * M.f64(Bs[-1]), maj=True))
        x, hb = (*sx[-1], Px[-1], Bx[-1]), (*sh[-1], Ph[-1], Bh[-1])
        own = M.compose2_fwd(x, hb, cin_pad, variants)[1]
        bounds = [o + M.packed(inh[0][0], inh[1][0], inh[0][1] + inh[1][1], cin_pad, v) for o, v in zip(own, variants)]
    fam = 'compose_pack exact' if exact else 'compose_pack real'
    for v, W, WT, r, b in zip(variants, Ws, WTs, ref, bounds):
        check(fam, f'{shape} W[{int(v)}]', W, r, b)
        assert torch.equal(WT, W.t())
    if exact:
        gWs = [M.ints(rng, *r.shape) for r in ref]
        grads = torch.autograd.grad(list(Ws), flat, [_t(g) for g in gWs])
        gm = [a for part in M.stack_bwd(Px, Bx, Ph, Bh, cin_pad, gWs[0], gWs[1]) for a in part]
        for i, (a, b) in enumerate(zip(grads, gm)):
            check(fam, f'{shape} gradient {i}', a, b)
        assert recording.count('qt_compose_step_bwd') == 2 * (L - 2) and recording.count('qt_compose2_bwd') == 1


# ----------------------------------------------------------------------------------------------------------------- 3. Adam
def adam_inputs(n, kind, t, p0, seed=0):
    rng = np.random.default_rng(seed + n + t)
    g = M.adam_gradient(rng, kind, n)
    w = np.zeros(n, np.float32) if p0 == 'zero' else rng.standard_normal(n).astype(np.float32)
    if kind == 'zeros' or t == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m, v = (0.01 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.random(n)).astype(np.float32)
    return w, g, m, v


def flat_adam(w, m, v, t, capturable=False, lr=0.01):
    """A FlatAdam on the weights w whose state says that t - 1 steps were taken."""
    from qtmpnn.optim import FlatAdam
    par = torch.nn.Parameter(_t(w))
    opt = FlatAdam(par, lr=lr, capturable=capturable)
    st = opt._state(par)
    st['step'].fill_(t - 1)
    st['exp_avg'].copy_(_t(m))
    st['exp_avg_sq'].copy_(_t(v))
    return par, opt, st


def check_step(fam, name, par, grad, st, last_norm, w, g, m, v, t, max_norm=10.0, lr=0.01):
    out = M.adam_step(w, g, m, v, t, lr=lr, max_norm=max_norm)
    bnd = M.adam_bound(w, g, m, v, t, out, clip=max_norm is not None)
    r = {k: compare(got, out[k], bnd[k]) for k, got in (('p', par), ('g', grad), ('m', st['exp_avg']), ('v', st['exp_avg_sq']))}
    r['norm'] = abs(float(last_norm) - out['norm']) / bnd['norm'] if bnd['norm'] > 0 else float(float(last_norm) != out['norm'])
    worst = max(r.values())
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    print(f'  [{fam}] {name}: ' + ', '.join(f'{k} {x:.3g}' for k, x in r.items()))
    assert worst <= 1.0, f'{fam} {name}: {r}'
    return out


@pytest.mark.parametrize('kind', ['clipped', 'unclipped', 'loguniform', 'below', 'above', 'zeros'])
@pytest.mark.parametrize('n', M.ADAM_N)
def test_adam_one_step(recording, n, kind):
    """One FlatAdam.step(max_norm=10) at step t from weights 0 (the stored weight IS the update) and randn, per gradient family."""
    for t in (M.ADAM_T if n <= 34513 else (1, 100000)):
        for p0 in ('zero', 'randn'):
            w, g, m, v = adam_inputs(n, kind, t, p0)
            par, opt, st = flat_adam(w, m, v, t)
            par.grad = _t(g)
            opt.step(max_norm=10.0)
            fam = 'adam zero-gradient' if kind == 'zeros' else 'adam real'
            check_step(fam, f'n={n} {kind} t={t} p0={p0}', par, par.grad, st, opt.last_norm[0], w, g, m, v, t)
            assert int(st['step']) == t
            if kind == 'zeros':                           # exact zeros with m = v = 0: those weights come back bit for bit, nothing is NaN
                got = _np(par)
                assert np.array_equal(got[0::2], w[0::2]) and np.isfinite(got).all() and not _np(par.grad)[0::2].any()
    assert set(recording) == {'qt_flat_adam'}


@pytest.mark.parametrize('n', [257, 34513])
def test_adam_without_clipping_and_strided_gradient(n):
    """max_norm=None: the gradient comes back bit for bit.  A non-contiguous p.grad (a [::2] view): the clipped values are copied
    back into it."""
    w, g, m, v = adam_inputs(n, 'clipped', 10, 'randn')
    par, opt, st = flat_adam(w, m, v, 10)
    par.grad = _t(g)
    opt.step()
    assert np.array_equal(_np(par.grad), g)
    check_step('adam real', f'n={n} no clipping', par, par.grad, st, opt.last_norm[0], w, g, m, v, 10, max_norm=None)
    par, opt, st = flat_adam(w, m, v, 10)
    wide = torch.full((2 * n,), SENT, device=dev())
    wide[::2] = _t(g)
    par.grad = wide[::2]
    assert not par.grad.is_contiguous()
    opt.step(max_norm=10.0)
    check_step('adam real', f'n={n} strided gradient', par, wide[::2], st, opt.last_norm[0], w, g, m, v, 10)
    assert bool((wide[1::2] == SENT).all())


def test_adam_capturable_gives_the_same_bits():
    n, t = 34513, 10
    w, g, m, v = adam_inputs(n, 'clipped', t, 'randn')
    res = []
    for cap in (False, True):
        par, opt, st = flat_adam(w, m, v, t, capturable=cap)
        par.grad = _t(g)
        opt.step(max_norm=10.0)
        res.append([_np(x).copy() for x in (par, par.grad, st['exp_avg'], st['exp_avg_sq'], opt.last_norm[:1])])
    check_step('adam real', 'capturable', par, par.grad, st, opt.last_norm[0], w, g, m, v, t)
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def test_adam_captured_graph_replays():
    """One eager step, then one captured graph of step(max_norm=10) on a single stream replayed three times: fresh gradients are
    copied into the static buffer and lr is changed in place between replays; each replay is within bound of the model stepped
    from the kernel's own previous outputs; the device step counter reads 1 + the number of replays."""
    n = 34513
    rng = np.random.default_rng(5)
    w = rng.standard_normal(n).astype(np.float32)
    par, opt, st = flat_adam(w, np.zeros(n), np.zeros(n), 1, capturable=True)
    static_g = torch.zeros(n, device=dev())
    par.grad = static_g
    lr = opt.param_groups[0]['lr']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    state = lambda: [_np(x).copy() for x in (par, st['exp_avg'], st['exp_avg_sq'])]
    with torch.cuda.stream(side):
        g = M.adam_gradient(rng, 'clipped', n)
        static_g.copy_(_t(g))
        before = state()
        opt.step(max_norm=10.0)
        check_step('adam graph', 'eager step 1', par, static_g, st, opt.last_norm[0], *before[:1], g, *before[1:], 1)
        with torch.cuda.graph(graph, stream=side):
            opt.step(max_norm=10.0)
        for i, (kind, rate) in enumerate((('unclipped', 0.01), ('clipped', 0.005), ('loguniform', 0.0025))):
            g = M.adam_gradient(rng, kind, n)
            static_g.copy_(_t(g))
            lr.fill_(rate)
            before = state()
            graph.replay()
            side.synchronize()
            check_step('adam graph', f'replay {i + 1} ({kind}, lr {rate})', par, static_g, st, opt.last_norm[0], before[0], g, before[1], before[2],
                       i + 2, lr=rate)
    torch.cuda.current_stream().wait_stream(side)
    assert int(st['step']) == 1 + 3
    ENTRIES.append('qt_flat_adam')


@pytest.mark.parametrize('n', [1, 255, 1025, 34513])
def test_adam_raw_abi_leaves_the_trailing_elements(n):
    """p, g, m, v as the first n elements of buffers of n + 4: the four trailing elements keep the sentinel -- for p the zeros that
    FlatParams.buffer relies on (the packing gather reads the first of them as its zero)."""
    t = 2
    w, g, m, v = adam_inputs(n, 'clipped', t, 'randn')
    bufs = [filled(n + 4) for _ in range(4)]
    bufs[0][n:] = 0.0
    for b, a in zip(bufs, (w, g, m, v)):
        b[:n] = _t(a)
    step, stat = torch.tensor([t - 1], dtype=torch.int32, device=dev()), filled(2)
    call('qt_flat_adam', *[p(b) for b in bufs], n, p(step), None, 0.01, 0.9, 0.999, 1e-8, 10.0, p(stat))
    check_step('adam real', f'raw n={n}', bufs[0][:n], bufs[1][:n], dict(exp_avg=bufs[2][:n], exp_avg_sq=bufs[3][:n]), stat[0], w, g, m, v, t)
    assert bool((bufs[0][n:] == 0).all()) and all(bool((b[n:] == SENT).all()) for b in bufs[1:]) and float(stat[1]) == SENT and int(step) == t


def test_adam_chain(recording):
    """Five steps at n = 34513 with gradients above and below the clipping norm: p, m, v and the clipped g against the model stepped
    from the kernel's own previous outputs -- the bound stays a one-step bound.  (The second step is compared at t = 2: a step
    counter that does not advance is >= 10 bounds away, tests/test_pack_f64_host.py.)"""
    n = 34513
    rng = np.random.default_rng(3)
    w = rng.standard_normal(n).astype(np.float32)
    par, opt, st = flat_adam(w, np.zeros(n), np.zeros(n), 1)
    for t in range(1, 6):
        g = M.adam_gradient(rng, 'clipped' if t % 2 else 'unclipped', n)
        before = [_np(x).copy() for x in (par, st['exp_avg'], st['exp_avg_sq'])]
        par.grad = _t(g)
        opt.step(max_norm=10.0)
        check_step('adam chain', f'step {t}', par, par.grad, st, opt.last_norm[0], before[0], g, before[1], before[2], t)
    assert int(st['step']) == 5 and recording == ['qt_flat_adam'] * 5


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per family of this session (the figures of profiles/head_pack_f64.txt), POW_ULPS and the entry
    points that ran; when the whole file ran, every entry point of the family was called."""
    for fam in sorted(WORST):
        print(f'  worst [{fam}]: {WORST[fam]:.3g}')
    print(f'  POW_ULPS = {M.POW_ULPS}')
    print('  entry points:', ', '.join(f'{n} x{ENTRIES.count(n)}' for n in sorted(set(ENTRIES))))
    assert all(v <= 1.0 for v in WORST.values())
    assert all(WORST[f] == 0.0 for f in WORST if f.endswith('exact'))
    want = {'step exact', 'step real', 'compose2 exact', 'compose2 real', 'compose_pack exact', 'compose_pack real', 'adam real',
            'adam zero-gradient', 'adam graph', 'adam chain'}
    if not want <= set(WORST):
        return                                         # (a selection of the file ran: nothing to say about what it covers)
    assert {'qt_compose_step_fwd', 'qt_compose_step_bwd', 'qt_compose2_fwd', 'qt_compose2_bwd', 'qt_flat_adam'} <= set(ENTRIES)
