"""CPU-side checks of the input attribution maps (no GPU): qtmpnn.sensitivity.Sensitivity on hand-made arrays -- every reduction
against a plain numpy restatement, completeness on a linear toy, every constructor refusal by field name -- and the argument
checks of NextFramePredictorS2S.sensitivity on a CPU-constructed predictor: every refusal under its argument's name and before
any launch."""
import inspect

import numpy as np
import pytest
import torch

from qtmpnn.sensitivity import METHODS, Request, Sensitivity

B, L, T, W, H, C = 2, 3, 4, 5, 6, 2


def _maps(seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, L, T, W, H, C)).astype(np.float32)


def _result(method='gradient', **kw):
    maps = _maps()
    J = np.arange(B * L, dtype=np.float64).reshape(B, L)
    Jb = 0.5 * J if method == 'integrated' else None
    return Sensitivity(maps, (0, 2, 5), method, np.ones((W, H), np.float32), J, Jb, **kw), maps


def test_reductions_against_plain_numpy():
    s, maps = _result()
    m = maps.astype(np.float64)
    assert s.maps is not None and s.maps.dtype == np.float32 and s.maps.shape == (B, L, T, W, H, C)
    assert s.leads == (0, 2, 5) and s.method == 'gradient' and s.J.shape == (B, L) and s.J_baseline is None
    by_day = np.zeros((B, L, T))
    by_ch = np.zeros((B, L, C))
    for b in range(B):
        for l in range(L):
            for t in range(T):
                by_day[b, l, t] = np.abs(m[b, l, t]).sum()
            for c in range(C):
                by_ch[b, l, c] = np.abs(m[b, l, ..., c]).sum()
    np.testing.assert_allclose(s.by_day(), by_day, rtol=1e-12)
    np.testing.assert_allclose(s.by_channel(), by_ch, rtol=1e-12)
    np.testing.assert_allclose(s.by_day(lead=2), by_day[:, 1], rtol=1e-12)
    np.testing.assert_allclose(s.by_channel(lead=5), by_ch[:, 2], rtol=1e-12)
    assert s.by_day(lead=2).shape == (B, T) and s.by_channel(lead=0).shape == (B, C)
    np.testing.assert_allclose(s.by_day(absolute=False), m.sum(axis=(3, 4, 5)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s.by_channel(absolute=False), m.sum(axis=(2, 3, 4)), rtol=1e-12, atol=1e-12)
    # pixel maps: signed by default, summed over the axes that are not fixed
    np.testing.assert_allclose(s.pixel_map(2), m[:, 1].sum(axis=(1, 4)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s.pixel_map(2, day=3), m[:, 1, 3].sum(axis=-1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s.pixel_map(0, channel=1), m[:, 0, ..., 1].sum(axis=1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s.pixel_map(5, day=0, channel=0), m[:, 2, 0, ..., 0], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s.pixel_map(5, absolute=True), np.abs(m[:, 2]).sum(axis=(1, 4)), rtol=1e-12)
    assert s.pixel_map(0).shape == (B, W, H)
    with pytest.raises(KeyError, match='no lead 1'):
        s.pixel_map(1)
    with pytest.raises(KeyError, match='no lead 7'):
        s.by_day(lead=7)
    with pytest.raises(ValueError, match="completeness: defined for method='integrated' only"):
        s.completeness()
    p = s.pooled()
    assert p.maps.shape == (1, L, T, W, H, C) and p.maps.dtype == np.float32 and p.J.shape == (1, L) and p.leads == s.leads
    np.testing.assert_allclose(p.maps[0], m.mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(p.J[0], s.J.mean(axis=0), rtol=1e-12)


def test_completeness_on_a_linear_toy():
    """J = <a, x>, baseline 0: integrated gradients are a * x whatever the number of path points, so the maps sum to
    J(x) - J(0) and the residual is rounding (float32 maps summed in float64)."""
    rng = np.random.default_rng(1)
    a = rng.standard_normal((B, L, T, W, H, C))
    x = rng.standard_normal((B, 1, T, W, H, C))
    maps = (a * x).astype(np.float32)
    J = (a * x).sum(axis=(2, 3, 4, 5))
    s = Sensitivity(maps, range(L), 'integrated', np.ones((W, H)), J, np.zeros((B, L)))
    res = s.completeness()
    assert res.shape == (B, L)
    assert np.abs(res).max() <= 2.0 ** -23 * np.abs(a * x).sum(axis=(2, 3, 4, 5)).max()
    shifted = Sensitivity(maps, range(L), 'integrated', np.ones((W, H)), J + 1.0, np.full((B, L), 0.25))
    np.testing.assert_allclose(shifted.completeness(), res - 0.75, atol=1e-12)
    pooled = s.pooled()
    assert pooled.J_baseline.shape == (1, L) and pooled.completeness().shape == (1, L)


def test_constructor_refuses_by_field_name():
    maps, w = _maps(), np.ones((W, H), np.float32)
    J = np.zeros((B, L))
    ok = lambda **kw: Sensitivity(**{**dict(maps=maps, leads=(0, 1, 2), method='gradient', target=w, J=J), **kw})
    ok()
    for bad, name in ((dict(maps=maps.astype(np.float64)), 'maps: float32'), (dict(maps=maps[0]), 'maps: shape'),
                      (dict(leads=(0, 1)), 'leads:'), (dict(leads=(0, 2, 1)), 'leads:'), (dict(leads=(0, 1, 1.5)), 'leads:'),
                      (dict(leads=(-1, 0, 1)), 'leads:'), (dict(method='saliency'), 'method:'),
                      (dict(target=np.ones((W, H + 1), np.float32)), 'target:'), (dict(target=np.ones((W, H), np.int32)), 'target:'),
                      (dict(J=J.astype(np.float32)), 'J: float32'), (dict(J=J[:1]), 'J: float64 of shape'),
                      (dict(J_baseline=J), 'J_baseline: belongs'), (dict(method='integrated'), 'J_baseline: belongs'),
                      (dict(method='integrated', J_baseline=J[:, :2]), 'J_baseline: float64 of shape'),
                      (dict(method='integrated', J_baseline=J.astype(np.float32)), 'J_baseline: float32')):
        with pytest.raises(ValueError, match=name):
            ok(**bad)
    assert ok(method='integrated', J_baseline=J).J_baseline is not None


def test_request_normalises_what_it_accepts():
    mask = np.zeros((W, H), bool)
    mask[0] = True
    r = Request((T, W, H, C), 4, mask)
    assert r.leads == (0, 1, 2, 3) and r.method == 'gradient' and r.steps is None and r.baseline is None
    assert r.target.dtype == np.float32 and r.target[0].sum() == 0 and r.sum_w == (W - 1) * H
    t = np.arange(W * H, dtype=np.int64).reshape(W, H)
    r = Request((B, T, W, H, C), 4, mask, target=torch.from_numpy(t), leads=np.array([1, 3]), method='integrated', steps=4,
                baseline=np.zeros((T, W, H, C)))
    assert r.leads == (1, 3) and r.steps == 4 and r.baseline.shape == (T, W, H, C) and r.baseline.dtype == np.float32
    assert r.sum_w == float(t[1:].sum()) and t[0].sum() > 0                       # (the caller's array is not written to)
    assert Request((B, T, W, H, C), 4, None, method='gradient_x_input', baseline=np.ones((B, T, W, H, C))).baseline.shape[0] == B
    assert METHODS == ('gradient', 'gradient_x_input', 'integrated')


def _predictor(**kw):
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=C, input_timesteps=T, output_timesteps=4, device=None,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kw)


def test_sensitivity_signature():
    from model.mpnnlstm import NextFramePredictorS2S, PRODUCTS
    params = inspect.signature(NextFramePredictorS2S.sensitivity).parameters
    assert list(params) == ['self', 'x', 'concat_layers', 'mask', 'high_interest_region', 'graph_structure', 'target', 'leads',
                            'method', 'baseline', 'steps']
    assert params['method'].default == 'gradient' and params['steps'].default == 16
    assert all(params[k].default is None for k in ('concat_layers', 'mask', 'high_interest_region', 'graph_structure', 'target',
                                                   'leads', 'baseline'))
    assert 'use_graph' not in params and 'sensitivity' not in PRODUCTS
    doc = NextFramePredictorS2S.sensitivity.__doc__
    assert 'MESHES ARE HELD FIXED' in doc and 'state transfer' in doc


def test_sensitivity_refuses_by_argument_name_before_any_launch(monkeypatch):
    """No GPU here: every refusal comes before the library is touched."""
    from qtmpnn import _lib
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    nfp = _predictor()
    x = torch.zeros(B, T, W, H, C)
    mask = np.zeros((W, H), bool)
    mask[:, :2] = True
    ones = np.ones((W, H), np.float32)
    only_masked = np.zeros((W, H), np.float32)
    only_masked[:, :2] = 1.0
    nan, inf, neg = ones.copy(), ones.copy(), ones.copy()
    nan[1, 3], inf[2, 3], neg[3, 3] = np.nan, np.inf, -1.0
    cases = [
        (dict(target=np.ones((W, H + 1))), 'target: shape'),
        (dict(target=np.ones((1, W, H))), 'target: shape'),
        (dict(target=np.full((W, H), 'a')), 'target: a numeric array'),
        (dict(target=np.full((W, H), None)), 'target: a numeric array'),
        (dict(target=nan), 'target: NaN or infinite'),
        (dict(target=inf), 'target: NaN or infinite'),
        (dict(target=neg), 'target: negative'),
        (dict(target=np.zeros((W, H))), 'target: the weights of the unmasked pixels sum to 0'),
        (dict(target=only_masked), 'target: the weights of the unmasked pixels sum to 0'),
        (dict(leads=[]), 'leads: empty'),
        (dict(leads=[0.0, 1.0]), 'leads: output steps are integers'),
        (dict(leads=[True]), 'leads: output steps are integers'),
        (dict(leads=3), 'leads: a sequence'),
        (dict(leads=[0, 4]), r'leads: step 4 is outside \[0, 4\)'),
        (dict(leads=[-1]), 'leads: step -1 is outside'),
        (dict(leads=[1, 1]), 'leads: the steps must be strictly increasing'),
        (dict(leads=[2, 0]), 'leads: the steps must be strictly increasing'),
        (dict(method='saliency'), 'method: '),
        (dict(method=None), 'method: '),
        (dict(method='integrated', steps=0), 'steps: the number of path points'),
        (dict(method='integrated', steps=257), 'steps: the number of path points'),
        (dict(method='integrated', steps=4.0), 'steps: the number of path points'),
        (dict(method='integrated', steps=True), 'steps: the number of path points'),
        (dict(method='integrated', baseline=np.zeros((T, W, H))), 'baseline: shape'),
        (dict(method='gradient_x_input', baseline=np.zeros((B + 1, T, W, H, C))), 'baseline: shape'),
        (dict(method='gradient_x_input', baseline=np.zeros((T, W, H, C + 1))), 'baseline: shape'),
        (dict(method='gradient', baseline=np.zeros((T, W, H, C))), "baseline: method='gradient'"),
        (dict(method='gradient', steps=8), "steps: path points belong to method='integrated'"),
        (dict(method='gradient_x_input', steps=8), "steps: path points belong to method='integrated'"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            nfp.sensitivity(x, mask=mask, **kw)
    with pytest.raises(ValueError, match='mask: shape'):
        nfp.sensitivity(x, mask=np.zeros((W + 1, H), bool))
    for bad in (x.long(), x[0, 0], np.zeros((T, W, H, C), np.float32)):
        with pytest.raises(ValueError, match='x: a floating-point tensor'):
            nfp.sensitivity(bad)
    # the model's own state: a remesh_input=True model, static mode; then the device of x (the existing check of the HIP path)
    with pytest.raises(NotImplementedError, match='sensitivity: remesh_input=True'):
        _predictor(remesh_input=True).sensitivity(x)
    nfp.model.static_shapes = True
    with pytest.raises(RuntimeError, match='sensitivity: not in static mode'):
        nfp.sensitivity(x)
    nfp.model.static_shapes = False
    with pytest.raises(RuntimeError, match='x must live on the GPU'):
        nfp.sensitivity(x, mask=mask, target=ones, leads=[0, 3], method='integrated', steps=4)
    assert launched == []
    assert all(p.requires_grad and p.grad is None for p in nfp.model.parameters()) and not nfp.model.static_shapes
