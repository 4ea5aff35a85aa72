"""The weighted binary cross-entropy (qt_wbce_rollout / _bwd, ops.rollout_wbce_partials, masked_bce and the trainer keywords
loss_weights / lead_weights / pos_weight of a binary=True predictor) against the float64 pixel model tests/wbce_f64.py, on the meshes
of tests/test_gpu_transfer_f64.py.

Bound: an entry whose exact value is sum_k t_k lies within LIMIT * 2^-24 * mag of the model, mag the model's sum of |t_k| (for a
partial sum lam w times the terms pw y L1, L0 and -y L0 of every pixel; for a gradient row
|g| lam (|o| sw + (pw + o (1 - pw)) sum w |y|) / max(o (1 - o), 1e-12)); an entry with mag = 0 -- a step of lead weight 0, a node
whose pixels all have weight 0, columns 1.. -- is exactly 0.  LIMIT = 50 is derived, not measured: 25 roundings, doubled, and both
kernels as written reach 25.
  A partial sum (k_loss_multi, the weighted term) is the unweighted term's chain of 22 with three more products: the logarithm
  (logf for L1, log1pf(-o) for
  L0; the device library follows the OpenCL accuracy table, log <= 3 ulp and log1p <= 2 ulp, and 3 ulp are 6 units of 2^-24), the
  difference 1 - y, the product pw y, the two products with the logarithms and their sum (5), the factors w and lam (2), four
  serial adds per thread (4), six butterfly steps (6), two adds of the four wave sums (2): 6 + 5 + 2 + 12 = 25.
  A gradient row of a 64 x 64 cell (k_pool_targets<true>, then k_loss_bwd_multi): the product w y at the load (1), the 2 x 2 sum
  (2),
  the four serial adds of the 4 x 4 sum (4), four pyramid levels of a 4-way sum each (8); the factor o + pw (1 - o), which is
  pw + o (1 - pw) as a sum of two non-negative terms (3), its product with swy (1), the subtraction from o sw (1; o sw is the
  shorter branch), 1 - o and the product o (1 - o) of the denominator (2), the factors g and lam and the division (3): 25.
Outputs are drawn from [0.02, 0.98], targets are exact 0, exact 1 and fractions, pixel weights are exact 0 or from [0.25, 4], lead
weights 0.5 + U[0, 1) with one exact 0, pw is 1, 3 and 0.5: a kernel that drops w, lam or pw is off by tens of percent of mag,
against a bound of 3e-6.  Every case prints its worst error / (2^-24 mag) before it asserts (pytest -s; a recorded run:
profiles/wbce_f64.txt)."""
import numpy as np
import pytest
import torch

import wbce_f64 as WB
from helpers import dev, golden
from test_gpu_transfer_f64 import SENT, _labels, _mask, _np, _nv, _rows, _step_meshes, _t, mesh_of

pytestmark = pytest.mark.gpu

LIMIT = 50.0
T18 = 18
PWS = (1.0, 3.0, 0.5)


def check(name, got, ref, mag):
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64)
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite value in a compared entry'
    err = np.abs(got - ref)
    pos = mag > 0
    ratio = float((err[pos] / (WB.U * mag[pos])).max()) if pos.any() else 0.0
    print(f'  {name}: {ratio:.3g}')
    assert (got[~pos] == 0).all(), f'{name}: an entry without terms is not exactly 0'
    assert ratio <= LIMIT, f'{name}: worst error / (2^-24 mag) = {ratio:.4g} > {LIMIT}'
    return ratio


def _probs(rng, *shape):
    """Outputs (..., W): column 0 from [0.02, 0.98], the other columns anything."""
    a = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    a[..., 0] = rng.uniform(0.02, 0.98, shape[:-1]).astype(np.float32)
    return a


def _targets(rng, *shape):
    """A mix of exact 0, exact 1 and fractions."""
    kind = rng.integers(0, 3, shape)
    return np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.random(shape))).astype(np.float32)


def _weights(n, m, T, seed, zeros=True):
    """w (n, m) from [0.25, 4] with, when `zeros`, one pixel in eight at exactly 0 and one rectangle of exact zeros that is aligned
    to no cell border (it covers small cells whole and cuts through larger ones); lam (T,) = 0.5 + U[0, 1) with one exact 0 (in the
    second launch when T > 16)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, (n, m)).astype(np.float32)
    lam = (0.5 + rng.random(T)).astype(np.float32)
    if zeros:
        w[rng.random((n, m)) < 0.125] = 0.0
        w[n // 4 + 1:n // 4 + 1 + (n * 3) // 8, m // 8 + 1:m // 8 + 2 + m // 2] = 0.0
        lam[T - 2 if T > 2 else 0] = 0.0
    return w, lam


@pytest.mark.parametrize('static', [False, True])
@pytest.mark.parametrize('tag', ['S', 'C', 'D', 'M'])
def test_rollout_wbce_over_two_launches(tag, static):
    """T_out = 18 = two launches (16 + 2), a different mesh at every step, outputs (N_t, 4), pw = 1, 3 and 0.5: every step's partial
    sums and every gradient row against the model, columns 1.., the step of lead weight 0 and the nodes of pixel weights 0 exactly
    0, two runs bit for bit.  S 24 x 32 (smaller than a tile), C 64 x 40 (ragged tile), D 64 x 64 B = 3 (one unsplit cell beside
    noise), M P = 15000 masked with an empty tile.  Static: NaN in the outputs' capacity rows, and through the raw entry points the
    capacity rows of the node sums and of the gradient keep their pre-fill."""
    from qtmpnn import _lib, ops
    import ctypes
    meshes = _step_meshes(tag, T18, static)
    B, P, n, m = meshes[0].B, meshes[0].P, meshes[0].n, meshes[0].m
    nvs = [_nv(ms) for ms in meshes]
    labs = [_labels(ms) for ms in meshes]
    assert (not static) or all(ms.n_dev is not None and ms.n_valid < ms.N for ms in meshes)
    w, lam = _weights(n, m, T18, 271)
    assert lam[16] == 0 and (w == 0).any() and w[w > 0].min() >= 0.25 and w.max() <= 4.0
    rng = np.random.default_rng(272)
    os_ = [_probs(rng, nv, 4) for nv in nvs]
    yy = _targets(rng, B, T18, n, m, 1)
    assert (yy == 0).any() and (yy == 1).any() and ((yy > 0) & (yy < 1)).any()
    wd, ld, yd = _t(w), _t(lam), _t(yy)
    gs = np.float32(0.37)

    def run(pw):
        bases = [_rows(ms, o).requires_grad_(True) for ms, o in zip(meshes, os_)]
        assert (not static) or all(bool(torch.isnan(b[nv:]).all()) for b, nv in zip(bases, nvs))
        part = ops.rollout_wbce_partials([b[:, :1] for b in bases], yd, meshes, wd, ld, pw)
        assert part is not None and part.shape == (T18, B * -(-P // 1024))
        return part, torch.autograd.grad(part.sum() * float(gs), bases)
    for pw in PWS:
        nm = f'rollout_wbce {tag} static={int(static)} pw={pw}'
        part, grads = run(pw)
        part2, grads2 = run(pw)
        same = all(torch.equal(a[:nv], b[:nv]) for a, b, nv in zip(grads, grads2, nvs))        # (capacity rows are never written)
        assert torch.equal(part, part2) and same, f'{nm}: two runs differ'
        assert bool(torch.isfinite(part).all()), f'{nm}: a partial sum is not finite'
        pt = _np(part.double().sum(dim=1))
        step_tot, step_mag, zero_rows, worst = [], [], 0, 0.0
        for t in range(T18):
            total, tmag, gref, gmag = WB.wbce(os_[t][:, 0], labs[t], yy[:, t], w, lam[t], pw, None, g=float(gs), W=4)
            step_tot.append(total)
            step_mag.append(tmag)
            worst = max(worst, check(f'{nm} grad t={t}', grads[t][:nvs[t]], gref, gmag))
            assert (_np(grads[t])[:nvs[t], 1:] == 0).all(), f'{nm}: columns 1.. of the gradient are not exactly 0'
            if lam[t] > 0:
                zero_rows += int((gmag[:, 0] == 0).sum())
        assert zero_rows > 0, f'{nm}: no node has all its pixels at weight 0'
        assert step_mag[16] == 0 and pt[16] == 0 and (_np(grads[16])[:nvs[16]] == 0).all()
        check(f'{nm} per-step partial sums', pt, step_tot, step_mag)
        check(f'{nm} total', part.double().sum().reshape(1), [sum(step_tot)], [sum(step_mag)])
        print(f'  {nm} worst gradient row: {worst:.3g}')
    if static:
        # the raw entry points on steps 3, 4 into pre-filled buffers: rows beyond the device node count are not written
        sl = slice(3, 5)
        outs = [_rows(ms, o) for ms, o in zip(meshes[sl], os_[sl])]
        swys = [torch.full((ms.N, 2), SENT, device=dev()) for ms in meshes[sl]]
        gouts = [torch.full((ms.N, 4), SENT, device=dev()) for ms in meshes[sl]]
        praw = torch.full((2, B * -(-P // 1024)), SENT, device=dev())
        vp, ip = ctypes.c_void_p, ctypes.c_int
        g1 = _t(np.array([gs]))
        _lib.call('qt_wbce_rollout', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[ms.labels.data_ptr() for ms in meshes[sl]]), (vp * 2)(*[ms.level.data_ptr() for ms in meshes[sl]]),
                  (ip * 2)(*[ms.N for ms in meshes[sl]]), (vp * 2)(*[s.data_ptr() for s in swys]), yd.data_ptr() + 4 * 3 * P,
                  T18 * P, P, wd.data_ptr(), ld.data_ptr() + 4 * 3, B, n, m, praw.data_ptr(), PWS[-1])
        _lib.call('qt_wbce_rollout_bwd', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[s.data_ptr() for s in swys]), (ip * 2)(*[ms.N for ms in meshes[sl]]),
                  (vp * 2)(*[ms.n_dev.data_ptr() for ms in meshes[sl]]), g1.data_ptr(), ld.data_ptr() + 4 * 3, 4,
                  (vp * 2)(*[t_.data_ptr() for t_ in gouts]), PWS[-1])
        assert torch.equal(praw, part[sl])            # (part, grads: the last pw of the loop above)
        for k, t in enumerate((3, 4)):
            nv = nvs[t]
            assert (_np(swys[k])[nv:] == SENT).all() and (_np(gouts[k])[nv:] == SENT).all(), 'a capacity row was written'
            assert np.isfinite(_np(swys[k])[:nv]).all() and torch.equal(gouts[k][:nv], grads[t][:nv])


def test_saturated_outputs():
    """Mesh S with nodes at o = 0 and o = 1, positive weights, pw = 3: the partial sums are finite and the model's with its -100
    clamp, the gradient rows are finite, and a node with o = 0 whose targets are all 0 has a gradient of exactly 0 (so has one with
    o = 1 under targets 1)."""
    from qtmpnn import ops
    ms = mesh_of('S')
    nv, lab, T, pw = _nv(ms), _labels(ms), 2, 3.0
    rng = np.random.default_rng(281)
    os_ = [_probs(rng, nv, 4) for _ in range(T)]
    yy = _targets(rng, ms.B, T, ms.n, ms.m, 1)
    w, lam = _weights(ms.n, ms.m, T, 282, zeros=False)
    zero, one = [0, 5, nv - 1], [1, 6, nv - 2]
    for o in os_:
        o[zero, 0], o[one, 0] = 0.0, 1.0
    yv = yy.reshape(ms.B, T, -1)
    yv[:, :, (lab == zero[0]).any(axis=0)] = 0.0          # o = 0 under targets that are all 0
    yv[:, :, (lab == one[0]).any(axis=0)] = 1.0           # o = 1 under targets that are all 1
    for i in zero[1:]:
        yv[:, :, np.flatnonzero((lab == i).any(axis=0))[:1]] = 1.0      # o = 0 under a target of 1: the clamp, pw * 100 per pixel
    for i in one[1:]:
        yv[:, :, np.flatnonzero((lab == i).any(axis=0))[:1]] = 0.0
    bases = [_t(o).requires_grad_(True) for o in os_]
    part = ops.rollout_wbce_partials([b[:, :1] for b in bases], _t(yy), [ms] * T, _t(w), _t(lam), pw)
    assert part is not None and bool(torch.isfinite(part).all())
    grads = torch.autograd.grad(part.sum(), bases)
    res = [WB.wbce(os_[t][:, 0], lab, yy[:, t], w, lam[t], pw, None, g=1.0, W=4) for t in range(T)]
    # four saturated pixels per step, each at least lam_min * w_min * 100 = 0.5 * 0.25 * 100
    assert all(r[0] >= 4 * 12.5 for r in res), 'the clamp is reached'
    check('saturated per-step partial sums', _np(part.double().sum(dim=1)), [r[0] for r in res], [r[1] for r in res])
    for t in range(T):
        assert bool(torch.isfinite(grads[t]).all())
        check(f'saturated grad t={t}', grads[t], res[t][2], res[t][3])
        gr = _np(grads[t])
        assert gr[zero[0], 0] == 0 and gr[one[0], 0] == 0 and abs(gr[zero[1], 0]) >= 1e10 and (gr[:, 1:] == 0).all()


@pytest.mark.parametrize('tag,form', [('D', 'rollout'), ('M', 'rollout'), ('M', 'per_step'), ('H', 'rollout')])
def test_masked_bce_divisor_and_scaling(tag, form):
    """masked_bce == model total / (B * sum lam * sum of w over the unmasked pixels) in float64 (pw does not enter the divisor): B = 3
    (D), with a mask (M), on the loss_mask mesh H (always the composed path) and through the composed per-step path (forced by a y
    that is not contiguous); rollout_wbce_partials is None exactly where rollout_wsse_partials is.  The composed path sums in
    torch's order; it is held to the same bound.  Scaling: w * 2 and lam * 4 leave the loss bit-identical (the partial sums and the
    float64 divisor both scale by exact powers of two)."""
    from model.mpnnlstm import masked_bce
    from qtmpnn import ops
    ms = mesh_of(tag)
    B, T, nv, lab, pw = ms.B, 3, _nv(ms), _labels(ms), 3.0
    mask = {'D': None, 'M': _mask('M'), 'H': golden('fixed_homog48x64.npz')['mask']}[tag]
    w, lam = _weights(ms.n, ms.m, T, 291)
    unmasked = np.ones((ms.n, ms.m), bool) if mask is None else ~np.asarray(mask, bool)
    rng = np.random.default_rng(292)
    os_ = [_probs(rng, nv, 4) for _ in range(T)]
    yy = _targets(rng, B, 2 * T, ms.n, ms.m, 1)
    ysel = yy[:, ::2]
    y = _t(ysel) if form == 'rollout' else _t(yy)[:, ::2]
    assert y.is_contiguous() == (form == 'rollout')
    bases = [_t(o).requires_grad_(True) for o in os_]
    outs = [b[:, :1] for b in bases]
    took = ops.rollout_wbce_partials(outs, y, [ms] * T, _t(w), _t(lam), pw) is not None
    assert took == (ops.rollout_wsse_partials(outs, y, [ms] * T, _t(w), _t(lam)) is not None) == (form == 'rollout' and tag != 'H')
    loss = masked_bce(outs, [ms] * T, y, mask, weights=w, lead_weights=lam, pos_weight=pw)
    keep = None if tag != 'H' else unmasked.reshape(-1)
    div = float(B) * float(lam.astype(np.float64).sum()) * float(w.astype(np.float64)[unmasked].sum())
    res = [WB.wbce(os_[t][:, 0], lab, ysel[:, t], w, lam[t], pw, keep, g=1.0 / div, W=4) for t in range(T)]
    nm = f'masked_bce {tag} {form}'
    check(nm, loss.reshape(1), [sum(r[0] for r in res) / div], [sum(r[1] for r in res) / div])
    if took:            # (the composed path's gradient runs through the transfer kernels, which have a bound of their own)
        grads = torch.autograd.grad(loss, bases)
        for t in range(T):
            check(f'{nm} grad t={t}', grads[t][:nv], res[t][2], res[t][3])
    scaled = masked_bce(outs, [ms] * T, y, mask, weights=2.0 * w, lead_weights=4.0 * lam, pos_weight=pw)
    assert torch.equal(loss.detach(), scaled.detach()), (nm, float(loss.detach()), float(scaled.detach()))
    other = masked_bce(outs, [ms] * T, y, mask, weights=w, lead_weights=lam, pos_weight=1.0)
    assert abs(float(other.detach()) - float(loss.detach())) > 0.05 * abs(float(loss.detach())), f'{nm}: pos_weight does not reach the loss'


def test_unit_weights_are_the_reference_loss_on_the_golden_rollout():
    """variant_binary.npz: masked_bce at unit weights and pw = 1 (and with every argument left out) meets the reference loss and
    gradients at the tolerances tests/test_gpu_bce.py holds the fused loss to."""
    from model.mpnnlstm import masked_bce
    from test_gpu_rollout import _check_grads, _variant_model
    g = golden('variant_binary.npz')
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    n, m, T = g['y'].shape[-3], g['y'].shape[-2], g['y'].shape[-4]
    for kw in (dict(weights=np.ones((n, m), np.float32), lead_weights=np.ones(T, np.float32), pos_weight=1.0), dict()):
        model = _variant_model(g, binary=True)
        outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
        loss = masked_bce(outs, meshes, y, g['mask'], **kw)
        print(f'  golden {float(g["loss"]):.8f} masked_bce {float(loss.detach()):.8f}')
        assert abs(float(loss.detach()) - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
        loss.backward()
        _check_grads(model, g)


def _binary_predictor(T_out):
    """The tiny binary predictor of tests/test_gpu_bce.py."""
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(4)
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=T_out, device=dev(), binary=True,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


def test_graphed_weighted_binary_step_bit_identical_to_eager():
    """make_graphed_step(..., loss_weights=, lead_weights=, pos_weight=3.0) on a binary=True predictor replays three steps whose
    losses are finite and, with all parameters, bit-identical to eager static-mode train_step with the same weights from the same
    seed; two eager runs agree bit for bit; and the weights reach the step (the unweighted loss of the same start differs)."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(1, 0, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    x2, y2 = synthetic.make_batch(1, 50, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    t = lambda a: torch.from_numpy(a).to(dev())
    mask = np.zeros((64, 64), dtype=bool)
    concat = torch.zeros(2, 3, 64, 64, 1, device=dev())
    w, lam = _weights(64, 64, 3, 295)
    kw = dict(loss_weights=w, lead_weights=lam, pos_weight=3.0)

    def fresh():
        nfp = _binary_predictor(3)
        nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=True)
        nfp.model.static_shapes = True
        return nfp
    eager, eager2, graphed, plain = fresh(), fresh(), fresh(), fresh()
    first = float(eager.train_step(t(x), t(y), concat, mask, **kw))
    assert first == float(eager2.train_step(t(x), t(y), concat, mask, **kw))
    unweighted = float(plain.train_step(t(x), t(y), concat, mask, fused=True))
    assert abs(first - unweighted) > 1e-3 * abs(unweighted), (first, unweighted)
    la, lb = eager.train_step(t(x), t(y), concat, mask, **kw), eager2.train_step(t(x), t(y), concat, mask, **kw)
    assert float(la) == float(lb)
    step = graphed.make_graphed_step(t(x), t(y), concat, mask, warmup=2, **kw)
    assert step.loss_weights.pos_weight == 3.0
    for a, b in ((x2, y2), (x, y), (x2, y2)):
        le = float(eager.train_step(t(a), t(b), concat, mask, **kw))
        le2 = float(eager2.train_step(t(a), t(b), concat, mask, **kw))
        lg = float(step(t(a), t(b), concat))
        print(f'  eager {le:.8f} graphed {lg:.8f}')
        assert np.isfinite(lg) and le == lg and le == le2, (le, le2, lg)
    for (k, p), (_, q), (_, r) in zip(eager.model.named_parameters(), graphed.model.named_parameters(),
                                      eager2.model.named_parameters()):
        assert torch.equal(p, q) and torch.equal(p, r), k


def test_trainer_runs_a_weighted_binary_predictor():
    """train(use_graph=True, truncated_backprop=0) with all three weights runs 2 epochs with finite losses; truncated_backprop = 2 on
    T_out = 3 (chunks [0, 2) and [2, 3)) runs eagerly, and a lead_weights whose second chunk sums to 0 is refused before the first
    chunk runs (no training step is counted)."""
    from test_gpu_wloss import _tiny
    mask = np.zeros((64, 64), dtype=bool)
    train, test, _ = _tiny(2)
    w, lam = _weights(64, 64, 2, 296)
    lam[:] = (0.5, 1.5)
    nfp = _binary_predictor(2)
    nfp.train(train, test, n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask, truncated_backprop=0, use_graph=True,
              loss_weights=w, lead_weights=lam, pos_weight=3.0)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
    train, test, items = _tiny(3)
    w, _ = _weights(64, 64, 3, 297)
    nfp = _binary_predictor(3)
    nfp.train(train, test, n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask, truncated_backprop=2, loss_weights=w,
              lead_weights=[0.5, 1.5, 0.25], pos_weight=0.5)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
    x, y = items[0][0].to(dev()), items[0][1].to(dev())
    run = lambda lam_: [float(v) for v in nfp.truncated_backward(x, y, None, mask, truncated_backprop=2, loss_weights=w,
                                                                 lead_weights=lam_, pos_weight=0.5)]
    a, b = run([0.5, 1.5, 0.25]), run([1.0, 3.0, 4.0])          # a chunk divides by its own slice's sum
    assert len(a) == 2 and all(np.isfinite(a)) and a[0] == pytest.approx(b[0], rel=1e-5) and a[1] == pytest.approx(b[1], rel=1e-5)
    before = [p.detach().clone() for p in nfp.model.parameters()]
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        nfp.train(train, test, n_epochs=1, mask=mask, truncated_backprop=2, loss_weights=w, lead_weights=[1.0, 1.0, 0.0], pos_weight=0.5)
    assert all(torch.equal(p, q) for p, q in zip(nfp.model.parameters(), before))
