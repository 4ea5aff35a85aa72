"""The weighted training loss (qt_wsse_rollout / _bwd, ops.rollout_wsse_partials, masked_mse(weights=, lead_weights=) and the
trainer keywords loss_weights / lead_weights) against the float64 pixel model tests/wloss_f64.py, on the meshes of
tests/test_gpu_transfer_f64.py.

Bound: an entry whose exact value is sum_k t_k lies within LIMIT * 2^-24 * sum_k |t_k| of the model; an entry without terms (every
weight 0) is exactly 0.  LIMIT = 40 is derived, not measured: the longest rounding chain of the kernels as written is that of a
gradient row of a 64 x 64 cell -- the product w y at the load (1), the 2 x 2 sum (2), the four serial adds of the 4 x 4 sum (4),
four pyramid levels of a 4-way sum each (8), the product sw out and the subtraction (2), the factors 2 g, lam and the final
product (3): 20 roundings, doubled.  (A partial total: d, d^2, the w and lam products, 4 adds per thread, 6 butterfly steps, 2 adds
= 16.)  Inputs are sign * (0.5 + U[0, 1)) and weights 0.5 + U[0, 1): one missing pixel of a 4096-pixel cell is at least
0.25 / (4096 * 2.25) of sum |t|, eleven times the bound.  Every case prints its worst error / (2^-24 sum |t|) before it asserts
(pytest -s; a recorded run: profiles/wloss_f64.txt)."""
import numpy as np
import pytest
import torch

import wloss_f64 as WM
from helpers import close, dev, golden
from test_gpu_transfer_f64 import SENT, _draw, _labels, _mask, _np, _nv, _rows, _step_meshes, _t, mesh_of

pytestmark = pytest.mark.gpu

LIMIT = 40.0
T18 = 18


def check(name, got, ref, mag):
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64)
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite value in a compared entry'
    err = np.abs(got - ref)
    pos = mag > 0
    ratio = float((err[pos] / (WM.U * mag[pos])).max()) if pos.any() else 0.0
    print(f'  {name}: {ratio:.3g}')
    assert (got[~pos] == 0).all(), f'{name}: an entry whose terms all have weight 0 is not exactly 0'
    assert ratio <= LIMIT, f'{name}: worst error / (2^-24 sum|t|) = {ratio:.4g} > {LIMIT}'
    return ratio


def _weights(n, m, T, seed):
    """w (n, m) = 0.5 + U[0, 1) with one rectangle of exact zeros that is aligned to no cell border (it covers single-pixel cells
    whole and cuts through larger ones); lam (T,) = 0.5 + U[0, 1) with one exact 0 (in the second launch when T > 16)."""
    rng = np.random.default_rng(seed)
    w = (0.5 + rng.random((n, m))).astype(np.float32)
    w[n // 4 + 1:n // 4 + 1 + (n * 3) // 8, m // 8 + 1:m // 8 + 2 + m // 2] = 0.0
    lam = (0.5 + rng.random(T)).astype(np.float32)
    lam[T - 2 if T > 2 else 0] = 0.0
    return w, lam


@pytest.mark.parametrize('static', [False, True])
@pytest.mark.parametrize('tag', ['S', 'C', 'D', 'M'])
def test_rollout_wsse_over_two_launches(tag, static):
    """T_out = 18 = two launches (16 + 2), a different mesh at every step, outputs (N_t, 4): every step's partial sums and every
    gradient row against the model, columns 1.. exactly 0, a step of lead weight 0 and a node of pixel weights 0 exactly 0, two
    runs bit for bit.  S 24 x 32 (smaller than a tile), C 64 x 40 (ragged tile), D 64 x 64 B = 3 (one unsplit cell beside noise),
    M P = 15000 masked with an empty tile.  Static: NaN in the outputs' capacity rows, and through the raw entry points the capacity
    rows of the node sums and of the gradient keep their pre-fill."""
    from qtmpnn import _lib, ops
    import ctypes
    meshes = _step_meshes(tag, T18, static)
    B, P, n, m = meshes[0].B, meshes[0].P, meshes[0].n, meshes[0].m
    nvs = [_nv(ms) for ms in meshes]
    assert (not static) or all(ms.n_dev is not None and ms.n_valid < ms.N for ms in meshes)
    w, lam = _weights(n, m, T18, 71)
    assert lam[16] == 0 and (w == 0).any()
    rng = np.random.default_rng(72)
    os_ = [_draw(rng, nv, 4) for nv in nvs]
    yy = _draw(rng, B, T18, n, m, 1)
    wd, ld, yd = _t(w), _t(lam), _t(yy)
    gs = np.float32(0.37)
    nm = f'rollout_wsse {tag} static={int(static)}'

    def run():
        bases = [_rows(ms, o).requires_grad_(True) for ms, o in zip(meshes, os_)]
        part = ops.rollout_wsse_partials([b[:, :1] for b in bases], yd, meshes, wd, ld)
        assert part is not None and part.shape == (T18, B * -(-P // 1024))
        return part, torch.autograd.grad(part.sum() * float(gs), bases)
    part, grads = run()
    part2, grads2 = run()
    same = all(torch.equal(a[:nv], b[:nv]) for a, b, nv in zip(grads, grads2, nvs))        # (capacity rows are never written)
    assert torch.equal(part, part2) and same, f'{nm}: two runs differ'
    pt = _np(part.double().sum(dim=1))
    step_tot, zero_rows, cut_rows = [], 0, 0
    for t, ms in enumerate(meshes):
        lab = _labels(ms)
        total, tmag, gref, gmag = WM.wsse(os_[t][:, 0], lab, yy[:, t], w, lam[t], None, g=float(gs), W=4)
        step_tot.append(total)
        check(f'{nm} grad t={t}', grads[t][:nvs[t]], gref, gmag)
        if lam[t] > 0:
            zero_rows += int((gmag[:, 0] == 0).sum())
            ok = lab >= 0
            zw = np.broadcast_to(w.reshape(1, -1) == 0, lab.shape)
            has0 = np.bincount(lab[ok & zw], minlength=nvs[t]) > 0
            hasp = np.bincount(lab[ok & ~zw], minlength=nvs[t]) > 0
            cut_rows += int((has0 & hasp).sum())
    assert zero_rows > 0 and cut_rows > 0, f'{nm}: the zero rectangle covers whole cells and cuts through others'
    check(f'{nm} per-step partial sums', pt, step_tot, step_tot)
    assert pt[16] == 0 and (_np(grads[16])[:nvs[16]] == 0).all()
    check(f'{nm} total', part.double().sum().reshape(1), [sum(step_tot)], [sum(step_tot)])
    if static:
        # the raw entry points on steps 3, 4 into pre-filled buffers: rows beyond the device node count are not written
        sl = slice(3, 5)
        outs = [_rows(ms, o) for ms, o in zip(meshes[sl], os_[sl])]
        swys = [torch.full((ms.N, 2), SENT, device=dev()) for ms in meshes[sl]]
        gouts = [torch.full((ms.N, 4), SENT, device=dev()) for ms in meshes[sl]]
        praw = torch.full((2, B * -(-P // 1024)), SENT, device=dev())
        vp, ip = ctypes.c_void_p, ctypes.c_int
        g1 = _t(np.array([gs]))
        _lib.call('qt_wsse_rollout', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[ms.labels.data_ptr() for ms in meshes[sl]]), (vp * 2)(*[ms.level.data_ptr() for ms in meshes[sl]]),
                  (ip * 2)(*[ms.N for ms in meshes[sl]]), (vp * 2)(*[s.data_ptr() for s in swys]), yd.data_ptr() + 4 * 3 * P,
                  T18 * P, P, wd.data_ptr(), ld.data_ptr() + 4 * 3, B, n, m, praw.data_ptr())
        _lib.call('qt_wsse_rollout_bwd', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[s.data_ptr() for s in swys]), (ip * 2)(*[ms.N for ms in meshes[sl]]),
                  (vp * 2)(*[ms.n_dev.data_ptr() for ms in meshes[sl]]), g1.data_ptr(), ld.data_ptr() + 4 * 3, 4,
                  (vp * 2)(*[t_.data_ptr() for t_ in gouts]))
        assert torch.equal(praw, part[sl])
        for k, t in enumerate((3, 4)):
            nv = nvs[t]
            assert (_np(swys[k])[nv:] == SENT).all() and (_np(gouts[k])[nv:] == SENT).all(), f'{nm}: a capacity row was written'
            assert torch.equal(gouts[k][:nv], grads[t][:nv])


@pytest.mark.parametrize('form', ['rollout', 'per_step'])
@pytest.mark.parametrize('tag', ['S', 'D', 'M', 'H'])
def test_weighted_masked_mse_divisor(tag, form):
    """masked_mse(weights=, lead_weights=) == model total / (B * sum lam * sum of w over the unmasked pixels) in float64: B = 1 (S),
    B = 3 (D), with a mask (M) and on the loss_mask mesh H (always the composed path), through the rollout launches and through the
    composed per-step path (forced by a y that is not contiguous).  rollout_wsse_partials is None exactly where
    rollout_sse_partials is.  The composed path sums in torch's order; it is held to the same bound."""
    from model.mpnnlstm import masked_mse
    from qtmpnn import ops
    ms = mesh_of(tag)
    B, T, nv, lab = ms.B, 3, _nv(ms), _labels(ms)
    mask = {'S': None, 'D': None, 'M': _mask('M'), 'H': golden('fixed_homog48x64.npz')['mask']}[tag]
    w, lam = _weights(ms.n, ms.m, T, 81)
    unmasked = np.ones((ms.n, ms.m), bool) if mask is None else ~np.asarray(mask, bool)
    rng = np.random.default_rng(82)
    os_ = [_draw(rng, nv, 4) for _ in range(T)]
    yy = _draw(rng, B, 2 * T, ms.n, ms.m, 1)
    ysel = yy[:, ::2]
    y = _t(ysel) if form == 'rollout' else _t(yy)[:, ::2]
    assert y.is_contiguous() == (form == 'rollout')
    bases = [_t(o).requires_grad_(True) for o in os_]
    outs = [b[:, :1] for b in bases]
    took = ops.rollout_wsse_partials(outs, y, [ms] * T, _t(w), _t(lam)) is not None
    assert took == (ops.rollout_sse_partials(outs, y, [ms] * T) is not None) == (form == 'rollout' and tag != 'H')
    loss = masked_mse(outs, [ms] * T, y, mask, weights=w, lead_weights=lam)
    keep = None if tag != 'H' else unmasked.reshape(-1)
    div = float(B) * float(lam.astype(np.float64).sum()) * float(w.astype(np.float64)[unmasked].sum())
    res = [WM.wsse(os_[t][:, 0], lab, ysel[:, t], w, lam[t], keep, g=1.0 / div, W=4) for t in range(T)]
    ref = sum(r[0] for r in res) / div
    check(f'weighted masked_mse {tag} {form}', loss.reshape(1), [ref], [ref])
    if took:            # (the composed path's gradient runs through the transfer kernels, which have a bound of their own)
        grads = torch.autograd.grad(loss, bases)
        for t in range(T):
            check(f'weighted masked_mse {tag} {form} grad t={t}', grads[t][:nv], res[t][2], res[t][3])


def _golden_run(g, **kw):
    from model.mpnnlstm import masked_mse
    from test_gpu_rollout import _model_from_golden
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    model = _model_from_golden(g, g['x'])
    outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
    return model, masked_mse(outs, meshes, y, g['mask'], **kw)


def test_unit_weights_are_the_unweighted_loss_on_the_golden_rollout():
    from test_gpu_rollout import _check_grads
    g = golden('rollout_ice64_masked_h8.npz')
    n, m, T = g['y'].shape[1], g['y'].shape[2], g['y'].shape[0]
    model, loss = _golden_run(g, weights=np.ones((n, m), np.float32), lead_weights=np.ones(T, np.float32))
    close(loss, g['loss'], msg='unit weights')
    loss.backward()
    _check_grads(model, g)
    w = np.zeros((n, m), np.float32)
    w[:, :m // 2] = 2.0
    lw = _golden_run(g, weights=w)[1].detach()
    ref = float(g['loss'])
    assert np.isfinite(float(lw)) and abs(float(lw) - ref) > 10 * (1e-4 * abs(ref) + 1e-5), (float(lw), ref)


def test_graphed_weighted_step_bit_identical_to_eager():
    """make_graphed_step(..., loss_weights=, lead_weights=) replays to the eager train_step's loss and weights bit for bit over two
    batches (dropout 0, both in static mode), and two eager runs agree bit for bit."""
    from model.model import CONVOLUTION_KWARGS
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(1, 0, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    x2, y2 = synthetic.make_batch(1, 50, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    t = lambda a: torch.from_numpy(a).to(dev())
    mask = np.zeros((64, 64), dtype=bool)
    concat = torch.zeros(2, 3, 64, 64, 1, device=dev())
    w, lam = _weights(64, 64, 3, 91)
    kw = dict(loss_weights=w, lead_weights=lam)

    def fresh():
        torch.manual_seed(5)
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=3, device=dev(),
                                    model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=2,
                                                      convolution_type='MHTransformerConv'))
        nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=True)
        nfp.model.static_shapes = True
        return nfp
    old = dict(CONVOLUTION_KWARGS['MHTransformerConv'])
    try:
        CONVOLUTION_KWARGS['MHTransformerConv']['dropout'] = 0.0
        eager, eager2, graphed = fresh(), fresh(), fresh()
        for _ in range(2):
            la = eager.train_step(t(x), t(y), concat, mask, **kw)
            lb = eager2.train_step(t(x), t(y), concat, mask, **kw)
            assert float(la) == float(lb)
        step = graphed.make_graphed_step(t(x), t(y), concat, mask, warmup=2, **kw)
        for a, b in ((x2, y2), (x, y)):
            le, le2 = float(eager.train_step(t(a), t(b), concat, mask, **kw)), float(eager2.train_step(t(a), t(b), concat, mask, **kw))
            lg = float(step(t(a), t(b), concat))
            assert np.isfinite(le) and le == lg and le == le2, (le, le2, lg)
        for (k, p), (_, q), (_, r) in zip(eager.model.named_parameters(), graphed.model.named_parameters(),
                                          eager2.model.named_parameters()):
            assert torch.equal(p, q) and torch.equal(p, r), k
    finally:
        CONVOLUTION_KWARGS['MHTransformerConv'].update(old)


def _tiny(T_out):
    from helpers import TinyLoader
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(5, 0, 4, 3, T_out, n_digits=1, pixel_noise=0.0)
    items = [(torch.from_numpy(x[i:i + 2]), torch.from_numpy(y[i:i + 2]), torch.zeros(1)) for i in (0, 2)]
    return TinyLoader(items, (64, 64)), TinyLoader(items[:1], (64, 64)), items


def _predictor(T_out):
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(4)
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=T_out, device=dev(),
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


@pytest.mark.parametrize('use_graph', [False, True])
def test_trainer_runs_with_loss_weights(use_graph):
    train, test, _ = _tiny(2)
    w, lam = _weights(64, 64, 2, 95)
    lam[:] = (0.5, 1.5)
    mask = np.zeros((64, 64), dtype=bool)
    nfp = _predictor(2)
    nfp.train(train, test, n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask, truncated_backprop=0, use_graph=use_graph,
              loss_weights=w, lead_weights=lam)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)


def test_truncated_chunks_divide_by_their_own_lead_weights():
    """truncated_backprop = 2 with T_out = 3: chunks [0, 2) and [2, 3).  A chunk's loss is invariant under a factor on its own slice
    of lead_weights (it divides by the slice's sum, not by the whole vector's), and the one-step chunk does not see lam at all."""
    train, test, items = _tiny(3)
    w, _ = _weights(64, 64, 3, 96)
    mask = np.zeros((64, 64), dtype=bool)
    nfp = _predictor(3)
    nfp.train(train, test, n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask, truncated_backprop=2, loss_weights=w,
              lead_weights=[0.5, 1.5, 0.25])
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
    x, y = items[0][0].to(dev()), items[0][1].to(dev())
    run = lambda lam: [float(v) for v in nfp.truncated_backward(x, y, None, mask, truncated_backprop=2, loss_weights=w, lead_weights=lam)]
    a, b, c = run([0.5, 1.5, 0.25]), run([1.0, 3.0, 4.0]), run([1.0, 1.0, 1.0])
    assert len(a) == 2 and all(np.isfinite(a))
    assert a[0] == pytest.approx(b[0], rel=1e-5) and a[1] == pytest.approx(b[1], rel=1e-5) and a[1] == pytest.approx(c[1], rel=1e-5)
    assert abs(a[0] - c[0]) > 1e-4 * abs(c[0])
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        run([1.0, 1.0, 0.0])
