"""Host checks of the float64 model of the weight-space composition and of clip + Adam (tests/pack_f64.py) on its own: the
composition agrees with float64 ops.compose_chebconvs + GConvLSTM._assemble on the CPU and with their autograd, Adam with
clip_grad_norm_ + torch.optim.Adam on float64 tensors; float32 emulations stay within one bound; single mutations land at >= 10
bounds on a named case of tests/test_gpu_pack_f64.py; and the known deviation from torch's double bias correction is stated.

Mutation -> the GPU case that sees it (shape (cin, cin_pad, h, K, L), variants; real-valued operands unless noted):
  cf without the |a - b| term            test_products[real, (4, 4, 8, 3, 2), (True, False)]          W
  B1 added at every order                test_products[real, (4, 4, 8, 3, 2), (True, False)]          bias rows of W
  pad rows non-zero                      test_products[exact, (5, 8, 8, 3, 2), (True, False)]         W (bound 0 there)
  x and h row blocks swapped             test_products[real, (4, 4, 16, 1, 2), (True,)]               W
  bias rows from one branch only         test_products[real, (1, 4, 16, 2, 2), (True, False)]         bias rows of W
  gb from one variant only               test_products[real, (4, 4, 8, 3, 2), (True, False)]          gP1, gB0, gB1
  WT != W^T                              every test_products case: WT == W.T bit for bit
  eps inside the square root             test_adam_one_step[34513, loguniform, t = 10]
  no bias correction on v                test_adam_one_step[34513, unclipped, t = 10]
  t - 1 in the corrections               test_adam_one_step[34513, unclipped, t = 2]
  clipped gradient not written back      test_adam_one_step[34513, clipped, t = 1]                    g
  coef without min(.., 1)                test_adam_one_step[34513, unclipped, t = 1]
  norm drops the tail n mod 1024         test_adam_one_step[1025, clipped, t = 1], [1023, clipped, t = 1]
  step counter does not advance          test_adam_chain (the second step compares against t = 2)
"""
import numpy as np
import pytest
import torch

import pack_f64 as M


def worst(got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(bound, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    pos = bound > 0
    if (err[~pos] != 0).any():
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def stack(gen, seed, cin, h, K, L):
    rng = np.random.default_rng(seed)
    Px = [gen(rng, 4, K, cin if l == 0 else h, h) for l in range(L)]
    Ph = [gen(rng, 4, K, h, h) for l in range(L)]
    return Px, [gen(rng, 4, h) for _ in range(L)], Ph, [gen(rng, 4, h) for _ in range(L)], rng


# ------------------------------------------------------------------------------------- composition against torch, float64
@pytest.mark.parametrize('cin,cin_pad,h,K,L', [(4, 4, 8, 3, 2), (5, 8, 8, 3, 2), (1, 4, 16, 2, 2), (4, 4, 16, 1, 2), (8, 8, 16, 3, 3), (5, 8, 8, 2, 4)])
def test_model_equals_float64_torch_composition_and_autograd(cin, cin_pad, h, K, L):
    from model.model import GConvLSTM
    from qtmpnn import ops
    Px, Bx, Ph, Bh, rng = stack(M.draw, cin + K + L, cin, h, K, L)
    t = lambda xs: [torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in xs]
    tPx, tBx, tPh, tBh = t(Px), t(Bx), t(Ph), t(Bh)
    cell = GConvLSTM(cin, h, 1, 'ChebConv')
    Mx, bx = ops.compose_chebconvs(tPx, tBx)
    Mh, bh = ops.compose_chebconvs(tPh, tBh)
    variants = (True, False)
    ref = [c.W for c in cell._assemble(Mx, bx, Mh, bh, None, None, cin_pad, None, variants, None)]
    Ws, _ = M.stack_pack(Px, Bx, Ph, Bh, cin_pad, variants)
    for W, r in zip(Ws, ref):
        assert W.shape == tuple(r.shape)
        np.testing.assert_allclose(W, r.detach().numpy(), rtol=1e-12, atol=1e-12)
    gW1, gW0 = M.draw(rng, *Ws[0].shape), M.draw(rng, *Ws[1].shape)
    for g1, g0 in ((gW1, gW0), (gW1, None), (None, gW0)):
        probe = sum((r * torch.from_numpy(g.astype(np.float64))).sum() for r, g in zip(ref, (g1, g0)) if g is not None)
        flat = tPx + tBx + tPh + tBh
        gr = torch.autograd.grad(probe, flat, retain_graph=True, allow_unused=True)
        gm = [a for part in M.stack_bwd(Px, Bx, Ph, Bh, cin_pad, g1, g0) for a in part]
        for a, b, ten in zip(gm, gr, flat):
            b = np.zeros(ten.shape) if b is None else b.numpy()
            np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-11)


def test_packed_layout_rows_and_pads():
    rng = np.random.default_rng(0)
    Mx, Mh, Bs = M.draw(rng, 4, 5, 5, 8), M.draw(rng, 4, 5, 8, 8), M.draw(rng, 4, 3, 8)
    W = M.packed(Mx, Mh, Bs, 8, True)
    assert W.shape == (5 * 16 + 4, 32)
    assert W[2 * 16 + 3, 1 * 8 + 5] == Mx[1, 2, 3, 5] and W[2 * 16 + 8 + 3, 3 * 8 + 5] == Mh[3, 2, 3, 5]
    assert (W.reshape(-1)[:5 * 16 * 32].reshape(5, 16, 32)[:, 5:8] == 0).all() and (W[-1] == 0).all() and W[5 * 16 + 2, 8 + 1] == Bs[1, 2, 1]
    assert M.stages(2, 4) == [(2, 1), (3, 2), (4, 3)] and M.stages(8, 5)[-1] == (29, 22) and M.pad4(22 + 7) == 32


# ------------------------------------------------------------------------------------------------ emulation and mutations
@pytest.mark.parametrize('cin,h,K,Ka,Kb0', [(4, 8, 3, 3, 1), (5, 8, 2, 4, 3), (8, 16, 3, 5, 3), (4, 8, 8, 29, 22), (4, 32, 3, 3, 1)])
def test_float32_emulation_of_a_product_within_one_bound(cin, h, K, Ka, Kb0):
    rng = np.random.default_rng(cin + h + Ka)
    b = M.branch(M.draw, rng, Ka, Kb0, K, cin, h)
    P, B = M.step_fwd(*b)
    eP, eB = M.step_bounds(*b)
    gP, gB = M.emulate_step_fwd(*b)
    r = worst(gP, P, eP), worst(gB, B, eB)
    print(f'  ({cin}, {h}, {K}) Ka={Ka} Kb0={Kb0}: P {r[0]:.3g}, B {r[1]:.3g}')
    assert max(r) <= 1.0
    bi = M.branch(M.ints, rng, Ka, Kb0, K, cin, h)
    Pi, Bi = M.emulate_step_fwd(*bi)
    assert np.array_equal(Pi, M.step_fwd(*bi)[0]) and np.array_equal(Bi, M.step_fwd(*bi)[1])       # exact operands: bound 0


def _product(gen, shape, seed=0):
    cin, cin_pad, h, K, L = shape
    Ka, Kb0 = M.stages(K, L)[-1]
    rng = np.random.default_rng(seed)
    return M.branch(gen, rng, Ka, Kb0, K, cin, h), M.branch(gen, rng, Ka, Kb0, K, h, h), rng


FWD_MUTATIONS = [
    ('cf without |a - b|', M.draw, (4, 4, 8, 3, 2), (True, False), dict(second_term=False)),
    ('B1 at every order', M.draw, (4, 4, 8, 3, 2), (True, False), dict(b1_every_order=True)),
    ('pad rows non-zero', M.ints, (5, 8, 8, 3, 2), (True, False), dict(pad_value=1e-30)),
    ('x and h blocks swapped', M.draw, (4, 4, 16, 1, 2), (True,), dict(swap=True)),
    ('bias rows from x only', M.draw, (1, 4, 16, 2, 2), (True, False), dict(bias_from_x_only=True)),
]


@pytest.mark.parametrize('what,gen,shape,variants,mut', FWD_MUTATIONS)
def test_forward_mutations_are_ten_bounds_away(what, gen, shape, variants, mut):
    assert shape in M.SHAPES and variants in M.VARIANTS
    x, hb, _ = _product(gen, shape)
    Ws, Es = M.compose2_fwd(x, hb, shape[1], variants)
    Wm, _ = M.compose2_fwd(x, hb, shape[1], variants, **mut)
    r = max(worst(a, b, 0.0 if gen is M.ints else e) for a, b, e in zip(Wm, Ws, Es))
    print(f'  {what} on {shape} {variants}: {r:.3g}')
    assert r >= 10.0


def test_gb_from_one_variant_is_ten_bounds_away():
    shape = (4, 4, 8, 3, 2)
    x, hb, rng = _product(M.draw, shape)
    Ws, _ = M.compose2_fwd(x, hb, shape[1], (True, False))
    g1, g0 = M.draw(rng, *Ws[0].shape), M.draw(rng, *Ws[1].shape)
    ref, bnd = M.compose2_bwd(x, hb, shape[1], g1, g0)
    mut, _ = M.compose2_bwd(x, hb, shape[1], g1, g0, one_variant_bias=True)
    r = [worst(a, b, e) for a, b, e in zip(mut, ref, bnd)]
    print('  gb from one variant:', ', '.join(f'{v:.3g}' for v in r))
    assert r[1] >= 10 and r[2] >= 10 and r[3] >= 10 and r[5] >= 10 and r[6] >= 10 and r[7] >= 10


def test_a_transpose_that_is_not_the_transpose_is_seen():
    """The GPU file asserts WT == W.T bit for bit: any misplaced entry of a matrix of distinct values fails."""
    x, hb, _ = _product(M.draw, (5, 8, 8, 3, 2))
    W = M.compose2_fwd(x, hb, 8, (True,))[0][0]
    WT = W.T.copy()
    WT[3, 1], WT[3, 2] = WT[3, 2], WT[3, 1]
    assert not np.array_equal(WT, W.T)


# -------------------------------------------------------------------------------------------------------------------- Adam
def test_adam_model_equals_torch_over_five_steps():
    rng = np.random.default_rng(0)
    n = 1000
    p = rng.standard_normal(n)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=0.01)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * (0.5 if t % 2 else 0.01)
        tp.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_([tp], 10.0)
        opt.step()
        out = M.adam_step(p, g, m, v, t, max_norm=10.0, exact_hyper=True)
        p, m, v = out['p'], out['m'], out['v']
        np.testing.assert_allclose(out['norm'], float(norm), rtol=1e-13)
        np.testing.assert_allclose(out['g'], tp.grad.numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-14)


def test_known_deviation_from_double_bias_correction():
    d1 = M.beta2_deviation(1)
    assert abs(d1 - abs(M.f32(0.999) - 0.999) / (2 * (1 - 0.999))) < 1e-18 and 6.0e-6 < d1 < 7.0e-6 and d1 < 1e-5
    ds = [M.beta2_deviation(t) for t in M.ADAM_T]
    assert all(a > b for a, b in zip(ds, ds[1:])), ds                      # it shrinks with t
    # the first-order figure is what the correction factor sqrt(1 - beta2^t) -- and with it the update for a given v -- moves by
    # (from a zero state at t = 1, v = (1 - beta2) g^2 carries the same factor and the two cancel: the deviation needs a history)
    for t, d in zip(M.ADAM_T, ds):
        rel = abs(np.sqrt(1.0 - M.f32(0.999) ** t) / np.sqrt(1.0 - 0.999 ** t) - 1.0)
        assert abs(rel - d) <= 0.02 * d + 1e-12, (t, rel, d)
    rng = np.random.default_rng(1)
    g, v0 = rng.standard_normal(100) * 0.01, rng.random(100) * 1e-2
    a = M.adam_step(np.zeros(100), g, np.zeros(100), v0, 1, max_norm=None, eps=0.0)
    b = M.adam_step(np.zeros(100), g, np.zeros(100), v0, 1, max_norm=None, eps=0.0, exact_hyper=True, lr=M.f32(0.01), beta1=M.f32(0.9))
    assert np.abs(a['upd'] / b['upd'] - 1).max() < 1e-5


def adam_case(n, kind, t, p0='zero', seed=0):
    rng = np.random.default_rng(seed + n + t)
    g = M.adam_gradient(rng, kind, n)
    p = np.zeros(n, np.float32) if p0 == 'zero' else rng.standard_normal(n).astype(np.float32)
    if kind == 'zeros' or t == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m, v = (0.01 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.random(n)).astype(np.float32)
    return p, g, m, v


def adam_ratios(n, kind, t, p0='zero', **mut):
    p, g, m, v = adam_case(n, kind, t, p0)
    out = M.adam_step(p, g, m, v, t)
    bnd = M.adam_bound(p, g, m, v, t, out)
    e = M.emulate_adam(p, g, m, v, t, **mut)
    return {k: worst(e[k], out[k], bnd[k]) for k in ('p', 'g', 'm', 'v', 'norm')}


@pytest.mark.parametrize('n', [1, 257, 1025, 34513])
@pytest.mark.parametrize('kind', ['clipped', 'unclipped', 'loguniform', 'below', 'above', 'zeros'])
def test_float32_adam_emulation_within_one_bound(n, kind):
    for t in M.ADAM_T:
        for p0 in ('zero', 'randn'):
            r = adam_ratios(n, kind, t, p0)
            assert max(r.values()) <= 1.0, (n, kind, t, p0, r)


ADAM_MUTATIONS = [
    ('eps inside the square root', 34513, 'loguniform', 10, dict(eps_inside=True), 'p'),
    ('no bias correction on v', 34513, 'unclipped', 10, dict(no_bc2=True), 'p'),
    ('t - 1 in the corrections', 34513, 'unclipped', 2, dict(t_minus_1=True), 'p'),
    ('clipped gradient not written back', 34513, 'clipped', 1, dict(no_writeback=True), 'g'),
    ('coef without min', 34513, 'unclipped', 1, dict(no_min=True), 'm'),
    ('norm drops the tail', 1025, 'clipped', 1, dict(drop_tail=True), 'norm'),
    ('norm drops the tail', 1023, 'clipped', 1, dict(drop_tail=True), 'norm'),
]


@pytest.mark.parametrize('what,n,kind,t,mut,out', ADAM_MUTATIONS)
def test_adam_mutations_are_ten_bounds_away(what, n, kind, t, mut, out):
    assert n in M.ADAM_N and t in M.ADAM_T
    r = adam_ratios(n, kind, t, **mut)
    print(f'  {what} on n={n} {kind} t={t}: {out} {r[out]:.3g}')
    assert r[out] >= 10.0


def test_a_step_counter_that_does_not_advance_is_ten_bounds_away():
    """test_adam_chain compares the second step against t = 2: a kernel that stays at t = 1 is this far off."""
    p, g, m, v = adam_case(34513, 'unclipped', 2)
    out = M.adam_step(p, g, m, v, 2)
    e = M.emulate_adam(p, g, m, v, 1)
    assert worst(e['p'], out['p'], M.adam_bound(p, g, m, v, 2, out)['p']) >= 10.0
