"""The fused binary cross-entropy (qt_bce_rollout / _bwd, ops.rollout_bce_partials, masked_mse(binary=True, fused=True) and the
captured training step of a binary=True predictor) against the float64 pixel model tests/bce_f64.py, on the meshes of
tests/test_gpu_transfer_f64.py.

Bound: an entry whose exact value is sum_k t_k lies within LIMIT * 2^-24 * mag of the model, mag the model's sum of |t_k| (for a
partial sum the terms y L1, L0 and -y L0 of every pixel; for a gradient row |g| (npix |o| + sum |y|) / max(o (1 - o), 1e-12)); an
entry with mag = 0 is exactly 0.  LIMIT = 44 is derived, not measured.  The longest rounding chain of the kernels as written is
that of a partial sum: the logarithm (logf for L1, log1pf(-o) for L0; the device library follows the OpenCL accuracy table, log
<= 3 ulp and log1p <= 2 ulp, and 3 ulp are 6 units of 2^-24), the difference 1 - y, the two products and their sum (4), four
serial adds per thread (4), six butterfly steps (6), two adds of the four wave sums (2): 22 roundings, doubled.  (A gradient row
of a 64 x 64 cell: the 2 x 2 sum (2), the four serial adds of the 4 x 4 sum (4), four pyramid levels of a 4-way sum each (8), the
product npix o and the subtraction (2), 1 - o and the product o (1 - o) (2), the factor g and the division (2) = 20.)  Outputs are
drawn from [0.02, 0.98] and targets are exact 0, exact 1 and fractions: a pixel's terms are at least 0.02, so one missing pixel of a
15000-pixel step is 2e-7 of its mag at the least, against a bound of 2.6e-6 -- the per-step sums guard the rounding, the gradient
rows (a 4096-pixel cell: one pixel is 1 / 4096 of the row) guard the pixels.  Every case prints its worst error / (2^-24 mag)
before it asserts (pytest -s; a recorded run: profiles/bce_f64.txt)."""
import numpy as np
import pytest
import torch

import bce_f64 as BM
from helpers import dev, golden, grad_close
from test_gpu_transfer_f64 import SENT, _labels, _np, _nv, _rows, _step_meshes, _t, mesh_of

pytestmark = pytest.mark.gpu

LIMIT = 44.0
T18 = 18


def check(name, got, ref, mag):
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64)
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite value in a compared entry'
    err = np.abs(got - ref)
    pos = mag > 0
    ratio = float((err[pos] / (BM.U * mag[pos])).max()) if pos.any() else 0.0
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


@pytest.mark.parametrize('static', [False, True])
@pytest.mark.parametrize('tag', ['S', 'C', 'D', 'M'])
def test_rollout_bce_over_two_launches(tag, static):
    """T_out = 18 = two launches (16 + 2), a different mesh at every step, outputs (N_t, 4): every step's partial sums and every
    gradient row against the model, columns 1.. exactly 0, two runs bit for bit.  S 24 x 32 (smaller than a tile), C 64 x 40 (ragged
    tile), D 64 x 64 B = 3 (one unsplit cell beside noise), M P = 15000 masked with an empty tile.  Static: NaN in the outputs'
    capacity rows, and through the raw entry points the capacity rows of the node sums and of the gradient keep their pre-fill."""
    from qtmpnn import _lib, ops
    import ctypes
    meshes = _step_meshes(tag, T18, static)
    B, P, n, m = meshes[0].B, meshes[0].P, meshes[0].n, meshes[0].m
    nvs = [_nv(ms) for ms in meshes]
    assert (not static) or all(ms.n_dev is not None and ms.n_valid < ms.N for ms in meshes)
    rng = np.random.default_rng(172)
    os_ = [_probs(rng, nv, 4) for nv in nvs]
    yy = _targets(rng, B, T18, n, m, 1)
    assert (yy == 0).any() and (yy == 1).any() and ((yy > 0) & (yy < 1)).any()
    yd = _t(yy)
    gs = np.float32(0.37)
    nm = f'rollout_bce {tag} static={int(static)}'

    def run():
        bases = [_rows(ms, o).requires_grad_(True) for ms, o in zip(meshes, os_)]
        assert (not static) or all(bool(torch.isnan(b[nv:]).all()) for b, nv in zip(bases, nvs))
        part = ops.rollout_bce_partials([b[:, :1] for b in bases], yd, meshes)
        assert part is not None and part.shape == (T18, B * -(-P // 1024))
        return part, torch.autograd.grad(part.sum() * float(gs), bases)
    part, grads = run()
    part2, grads2 = run()
    same = all(torch.equal(a[:nv], b[:nv]) for a, b, nv in zip(grads, grads2, nvs))        # (capacity rows are never written)
    assert torch.equal(part, part2) and same, f'{nm}: two runs differ'
    assert bool(torch.isfinite(part).all()), f'{nm}: a partial sum is not finite'
    pt = _np(part.double().sum(dim=1))
    step_tot, step_mag = [], []
    for t, ms in enumerate(meshes):
        total, tmag, gref, gmag = BM.bce(os_[t][:, 0], _labels(ms), yy[:, t], None, g=float(gs), W=4)
        step_tot.append(total)
        step_mag.append(tmag)
        check(f'{nm} grad t={t}', grads[t][:nvs[t]], gref, gmag)
        assert (_np(grads[t])[:nvs[t], 1:] == 0).all(), f'{nm}: columns 1.. of the gradient are not exactly 0'
    check(f'{nm} per-step partial sums', pt, step_tot, step_mag)
    check(f'{nm} total', part.double().sum().reshape(1), [sum(step_tot)], [sum(step_mag)])
    if static:
        # the raw entry points on steps 3, 4 into pre-filled buffers: rows beyond the device node count are not written
        sl = slice(3, 5)
        outs = [_rows(ms, o) for ms, o in zip(meshes[sl], os_[sl])]
        sys_ = [torch.full((ms.N,), SENT, device=dev()) for ms in meshes[sl]]
        gouts = [torch.full((ms.N, 4), SENT, device=dev()) for ms in meshes[sl]]
        praw = torch.full((2, B * -(-P // 1024)), SENT, device=dev())
        vp, ip = ctypes.c_void_p, ctypes.c_int
        g1 = _t(np.array([gs]))
        _lib.call('qt_bce_rollout', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[ms.labels.data_ptr() for ms in meshes[sl]]), (vp * 2)(*[ms.level.data_ptr() for ms in meshes[sl]]),
                  (ip * 2)(*[ms.N for ms in meshes[sl]]), (vp * 2)(*[s.data_ptr() for s in sys_]), yd.data_ptr() + 4 * 3 * P,
                  T18 * P, P, B, n, m, praw.data_ptr())
        _lib.call('qt_bce_rollout_bwd', 2, (vp * 2)(*[o.data_ptr() for o in outs]), (ip * 2)(4, 4),
                  (vp * 2)(*[ms.npix.data_ptr() for ms in meshes[sl]]), (vp * 2)(*[s.data_ptr() for s in sys_]),
                  (ip * 2)(*[ms.N for ms in meshes[sl]]), (vp * 2)(*[ms.n_dev.data_ptr() for ms in meshes[sl]]), g1.data_ptr(), 4,
                  (vp * 2)(*[t_.data_ptr() for t_ in gouts]))
        assert torch.equal(praw, part[sl])
        for k, t in enumerate((3, 4)):
            nv = nvs[t]
            assert (_np(sys_[k])[nv:] == SENT).all() and (_np(gouts[k])[nv:] == SENT).all(), f'{nm}: a capacity row was written'
            assert np.isfinite(_np(sys_[k])[:nv]).all() and torch.equal(gouts[k][:nv], grads[t][:nv])


def test_saturated_outputs():
    """Mesh S with nodes at o = 0 and o = 1: the partial sums are finite and the model's with its -100 clamp, the gradient rows are
    finite, and a node with o = 0 whose targets are all 0 has a gradient of exactly 0 (so has one with o = 1 under targets 1)."""
    from qtmpnn import ops
    ms = mesh_of('S')
    nv, lab, T = _nv(ms), _labels(ms), 2
    rng = np.random.default_rng(181)
    os_ = [_probs(rng, nv, 4) for _ in range(T)]
    yy = _targets(rng, ms.B, T, ms.n, ms.m, 1)
    zero, one = [0, 5, nv - 1], [1, 6, nv - 2]
    for o in os_:
        o[zero, 0], o[one, 0] = 0.0, 1.0
    yv = yy.reshape(ms.B, T, -1)
    yv[:, :, (lab == zero[0]).any(axis=0)] = 0.0          # o = 0 under targets that are all 0
    yv[:, :, (lab == one[0]).any(axis=0)] = 1.0           # o = 1 under targets that are all 1
    for i in zero[1:]:
        yv[:, :, np.flatnonzero((lab == i).any(axis=0))[:1]] = 1.0      # o = 0 under a target of 1: the clamp, 100 per pixel
    for i in one[1:]:
        yv[:, :, np.flatnonzero((lab == i).any(axis=0))[:1]] = 0.0
    bases = [_t(o).requires_grad_(True) for o in os_]
    part = ops.rollout_bce_partials([b[:, :1] for b in bases], _t(yy), [ms] * T)
    assert part is not None and bool(torch.isfinite(part).all())
    grads = torch.autograd.grad(part.sum(), bases)
    res = [BM.bce(os_[t][:, 0], lab, yy[:, t], None, g=1.0, W=4) for t in range(T)]
    assert all(r[0] >= 400.0 for r in res), 'the clamp is reached: four saturated pixels of 100 each per step'
    check('saturated per-step partial sums', _np(part.double().sum(dim=1)), [r[0] for r in res], [r[1] for r in res])
    for t in range(T):
        assert bool(torch.isfinite(grads[t]).all())
        check(f'saturated grad t={t}', grads[t], res[t][2], res[t][3])
        gr = _np(grads[t])
        assert gr[zero[0], 0] == 0 and gr[one[0], 0] == 0 and abs(gr[zero[1], 0]) >= 1e11 and (gr[:, 1:] == 0).all()


def _binary_golden(fused):
    from model.mpnnlstm import masked_mse
    from test_gpu_rollout import _variant_model
    g = golden('variant_binary.npz')
    model = _variant_model(g, binary=True)
    x, y, concat = (torch.from_numpy(g[k]).to(dev()) for k in ('x', 'y', 'concat'))
    outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
    kw = dict(fused=True) if fused else {}
    return g, model, outs, meshes, y, masked_mse(outs, meshes, y, g['mask'], binary=True, **kw)


def test_fused_loss_is_the_torch_paths_on_the_golden_rollout():
    """variant_binary.npz: masked_mse(binary=True, fused=True) meets the reference loss and gradients at the tolerances of
    test_gpu_rollout.py::test_binary_head_golden, the parameter gradients of the two paths agree at that gradient tolerance, and the
    plain call is torch's formula as written before, bit for bit."""
    from model.graph_functions import unflatten
    from test_gpu_rollout import _check_grads
    g, model, outs, meshes, y, plain = _binary_golden(False)
    mesh0 = meshes[0]
    y_hat = torch.stack([unflatten(o, ms, (ms.n, ms.m)).reshape(ms.B, ms.n, ms.m, 1) for o, ms in zip(outs, meshes)], 1)
    keep = ~torch.as_tensor(np.asarray(g['mask'], bool))
    assert tuple(keep.shape) == (mesh0.n, mesh0.m)
    inline = torch.nn.functional.binary_cross_entropy(y_hat[:, :, keep], y.unsqueeze(0)[:, :, keep] if y.dim() == 4 else y[:, :, keep])
    assert torch.equal(plain, inline), (float(plain.detach()), float(inline.detach()))
    plain.backward()
    ref_grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    g, model, outs, meshes, y, fused = _binary_golden(True)
    print(f'  golden {float(g["loss"]):.8f} torch path {float(plain.detach()):.8f} fused {float(fused.detach()):.8f}')
    assert abs(float(fused.detach()) - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
    fused.backward()
    _check_grads(model, g)
    for k, p in model.named_parameters():
        assert (p.grad is None) == (k not in ref_grads), k
        if p.grad is not None:
            grad_close(p.grad, ref_grads[k], msg=k, floor=0.05 if k.endswith('lin_key.bias') else 1e-3)


def _binary_predictor(T_out):
    """test_gpu_wloss.py::_predictor with the binary head."""
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(4)
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=T_out, device=dev(), binary=True,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


def test_graphed_binary_step_bit_identical_to_eager():
    """make_graphed_step on a binary=True predictor captures (torch's BCELoss path cannot: it indexes with a host mask) and replays
    three steps whose losses are finite and, with all parameters, bit-identical to eager static-mode train_step(fused=True) from the
    same seed; two eager runs agree bit for bit."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(1, 0, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    x2, y2 = synthetic.make_batch(1, 50, 2, 3, 3, n_digits=1, pixel_noise=0.02)
    t = lambda a: torch.from_numpy(a).to(dev())
    mask = np.zeros((64, 64), dtype=bool)
    concat = torch.zeros(2, 3, 64, 64, 1, device=dev())

    def fresh():
        nfp = _binary_predictor(3)
        nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=True)
        nfp.model.static_shapes = True
        return nfp
    eager, eager2, graphed = fresh(), fresh(), fresh()
    for _ in range(2):
        la = eager.train_step(t(x), t(y), concat, mask, fused=True)
        lb = eager2.train_step(t(x), t(y), concat, mask, fused=True)
        assert float(la) == float(lb)
    step = graphed.make_graphed_step(t(x), t(y), concat, mask, warmup=2)
    for a, b in ((x2, y2), (x, y), (x2, y2)):
        le = float(eager.train_step(t(a), t(b), concat, mask, fused=True))
        le2 = float(eager2.train_step(t(a), t(b), concat, mask, fused=True))
        lg = float(step(t(a), t(b), concat))
        print(f'  eager {le:.8f} graphed {lg:.8f}')
        assert np.isfinite(lg) and le == lg and le == le2, (le, le2, lg)
    for (k, p), (_, q), (_, r) in zip(eager.model.named_parameters(), graphed.model.named_parameters(),
                                      eager2.model.named_parameters()):
        assert torch.equal(p, q) and torch.equal(p, r), k


def test_trainer_runs_a_binary_predictor_as_a_captured_graph():
    from test_gpu_wloss import _tiny
    train, test, _ = _tiny(2)
    mask = np.zeros((64, 64), dtype=bool)
    nfp = _binary_predictor(2)
    nfp.train(train, test, n_epochs=2, lr=0.01, lr_decay=0.5, mask=mask, truncated_backprop=0, use_graph=True)
    assert len(nfp.train_loss) == 2 and np.isfinite(nfp.train_loss + nfp.test_loss).all(), (nfp.train_loss, nfp.test_loss)
