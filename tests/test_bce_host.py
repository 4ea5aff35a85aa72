"""CPU-side checks of the fused binary cross-entropy (no GPU): the float64 model tests/bce_f64.py against torch's own
binary_cross_entropy in float64 (forward and autograd gradient, saturated rows included), the refusals of masked_mse by name and
before any launch, and the two entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bce_f64 as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, M_, T_ = 6, 8, 3


class StubMesh:
    """What masked_mse reads of a mesh before the first launch."""
    B, n, m, P, N, loss_mask = 1, N_, M_, N_ * M_, 5, None


def _torch_bce(o, lab, y, keep, g):
    """torch's BCELoss (sum) over the counted pixels in float64 and its autograd gradient with respect to the node values."""
    ot = torch.tensor(o, dtype=torch.float64, requires_grad=True)
    ok = lab >= 0
    if keep is not None:
        ok = ok & (np.asarray(keep).reshape(1, -1) != 0)
    img = ot[torch.from_numpy(np.where(ok, lab, 0))]
    okt = torch.from_numpy(ok)
    total = torch.nn.functional.binary_cross_entropy(img[okt], torch.from_numpy(np.asarray(y, np.float64))[okt], reduction='sum')
    (grad,) = torch.autograd.grad(total * g, ot)
    return float(total.detach()), grad.numpy()


@pytest.mark.parametrize('saturated', [False, True])
def test_float64_model_is_torchs_bce(saturated):
    rng = np.random.default_rng(11 + saturated)
    B, P, N = 2, 120, 19
    lab = rng.integers(-1, N, size=(B, P))
    o = rng.uniform(0.02, 0.98, N).astype(np.float32).astype(np.float64)
    y = rng.choice([0.0, 1.0, 0.3, 0.75], size=(B, P))
    if saturated:
        o[[0, 1, 2]] = 0.0
        o[[3, 4, 5]] = 1.0
        y[lab == 0] = 0.0                         # o = 0 under targets 0: no loss, gradient exactly 0
        y[lab == 3] = 1.0                         # o = 1 under targets 1: likewise
        assert ((lab == 1).sum() and (lab == 4).sum())
    keep = rng.random(P) < 0.8
    for kp in (None, keep):
        total, mag, grad, gmag = BM.bce(o, lab, y, kp, g=0.37, W=4)
        ref, gref = _torch_bce(o, lab, y, kp, 0.37)
        assert np.isfinite(total) and np.isfinite(grad).all() and mag >= abs(total)
        assert total == pytest.approx(ref, rel=1e-13)
        np.testing.assert_allclose(grad[:, 0], gref, rtol=1e-12, atol=1e-12 * np.abs(gref).max())
        assert (grad[:, 1:] == 0).all() and (gmag[:, 1:] == 0).all() and (gmag[:, 0] >= np.abs(grad[:, 0])).all()
        if saturated:
            assert grad[0, 0] == 0 and gref[0] == 0 and grad[3, 0] == 0 and gref[3] == 0
            assert abs(grad[1, 0]) > 1e9 or not ((lab == 1) & (y > 0)).any()      # o = 0 under a target > 0: the 1e-12 clamp rules


def test_the_clamp_is_torchs():
    """One pixel each: o = 0 under y = 1 and o = 1 under y = 0 cost exactly 100, as in torch."""
    lab = np.array([[0, 1]])
    total, mag, _, _ = BM.bce([0.0, 1.0], lab, [[1.0, 0.0]])
    ref = torch.nn.functional.binary_cross_entropy(torch.tensor([0.0, 1.0], dtype=torch.float64),
                                                   torch.tensor([1.0, 0.0], dtype=torch.float64), reduction='sum')
    assert total == 200.0 and float(ref) == 200.0 and mag == 200.0


def _call(binary=True, y=None, **kw):
    from model.mpnnlstm import masked_mse
    outs = [torch.full((StubMesh.N, 1), 0.5) for _ in range(T_)]     # CPU tensors: a launch would fail, a refusal comes first
    return masked_mse(outs, [StubMesh] * T_, torch.zeros(1, T_, N_, M_, 1) if y is None else y, None, binary, **kw)


def test_fused_without_binary_is_refused_by_name():
    with pytest.raises(ValueError, match='fused'):
        _call(binary=False, fused=True)
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    with pytest.raises(ValueError, match='fused'):
        nfp.forward_loss(torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1), fused=True)


def test_fused_binary_takes_no_weights():
    for kw in (dict(weights=np.ones((N_, M_), np.float32)), dict(lead_weights=np.ones(T_))):
        with pytest.raises(ValueError, match='binary'):
            _call(fused=True, **kw)


@pytest.mark.parametrize('shape', [(1, T_ + 1, N_, M_, 1), (1, T_, M_, N_, 1), (2, T_, N_, M_, 1), (T_, N_, M_, 2), (1, T_, N_, M_)])
def test_fused_refuses_wrong_target_shapes_before_any_launch(shape):
    with pytest.raises(ValueError, match='targets of shape'):
        _call(fused=True, y=torch.zeros(*shape))


def test_bce_entries_are_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    decls = header_decls()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('qt_bce_rollout', 'qt_bce_rollout_bwd'):
        assert re.match(r'int\s+%s\s*\(' % name, decls[name].text) and decls[name].times == 1, name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names(), name
    # the arguments of the squared-error pair
    assert _lib._SIGNATURES['qt_bce_rollout'] == _lib._SIGNATURES['qt_sse_rollout']
    assert _lib._SIGNATURES['qt_bce_rollout_bwd'] == _lib._SIGNATURES['qt_sse_rollout_bwd']
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme


def test_bce_entries_refuse_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_void_p * 64)()
    x = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16         # only ever validated, never dereferenced
    one = (ctypes.c_int * 16)(*([1] * 16))
    ptrs = (ctypes.c_void_p * 16)(*([x] * 16))

    def fwd(nseg=1, outs=ptrs, strides=one, labels=ptrs, levels=ptrs, Ns=one, sys_=ptrs, y=x, B=1, n=8, m=8, part=x):
        return lib.qt_bce_rollout(nseg, outs, strides, labels, levels, Ns, sys_, y, 64, 64, B, n, m, part, None)

    def bwd(nseg=1, outs=ptrs, strides=one, npixs=ptrs, sys_=ptrs, Ns=one, n_devs=ptrs, g=x, W=1, gouts=ptrs):
        return lib.qt_bce_rollout_bwd(nseg, outs, strides, npixs, sys_, Ns, n_devs, g, W, gouts, None)
    for kw in (dict(nseg=0), dict(nseg=17), dict(y=None), dict(part=None), dict(B=0), dict(n=0), dict(m=-8), dict(sys_=None),
               dict(sys_=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())):
        assert fwd(**kw) != 0 and b'qt_bce_rollout' in lib.qt_last_error(), kw
    for kw in (dict(nseg=0), dict(nseg=17), dict(g=None), dict(W=0), dict(gouts=None), dict(npixs=(ctypes.c_void_p * 16)()),
               dict(Ns=(ctypes.c_int * 16)(*([1 << 30] * 16)), W=4)):
        assert bwd(**kw) != 0 and b'qt_bce_rollout_bwd' in lib.qt_last_error(), kw
