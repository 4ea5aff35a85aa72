"""CPU-side checks of the weighted training loss (no GPU): every refusal by name and before any launch, the float64 model
tests/wloss_f64.py against tests/transfer_f64.py at unit weights, model.utils.cell_area_weights, and the two entry points in the
header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import transfer_f64 as M
import wloss_f64 as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, M_, T_ = 6, 8, 3


class StubMesh:
    """What masked_mse reads of a mesh before the first launch."""
    B, n, m, P, N, loss_mask = 1, N_, M_, N_ * M_, 5, None


def _call(binary=False, mask=None, **kw):
    from model.mpnnlstm import masked_mse
    outs = [torch.zeros(StubMesh.N, 1) for _ in range(T_)]           # CPU tensors: a launch would fail, a refusal comes first
    return masked_mse(outs, [StubMesh] * T_, torch.zeros(1, T_, N_, M_, 1), mask, binary, **kw)


def _w(fill=1.0):
    return np.full((N_, M_), fill, np.float32)


BAD_W = [('transposed', _w().T), ('flat', _w().reshape(-1)), ('frame stack', np.ones((1, N_, M_), np.float32)),
         ('nan', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, np.nan, 1.0)),
         ('inf', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, np.inf, 1.0)),
         ('negative', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, -0.5, 1.0)), ('zeros', _w(0.0))]
BAD_LAM = [('too long', np.ones(T_ + 1)), ('2-d', np.ones((T_, 1))), ('scalar', np.float32(1.0)), ('negative', [1.0, -1.0, 1.0]),
           ('nan', [1.0, np.nan, 1.0]), ('inf', [np.inf, 1.0, 1.0]), ('zeros', [0.0, 0.0, 0.0])]


@pytest.mark.parametrize('what,w', BAD_W, ids=[b[0] for b in BAD_W])
def test_masked_mse_refuses_bad_pixel_weights_by_name(what, w):
    with pytest.raises(ValueError, match='loss_weights'):
        _call(weights=w)
    with pytest.raises(ValueError, match='loss_weights'):
        _call(weights=torch.as_tensor(np.asarray(w)), lead_weights=np.ones(T_))


def test_pixel_weights_that_vanish_on_the_unmasked_pixels_are_refused():
    mask = np.zeros((N_, M_), bool)
    mask[:, :3] = True
    w = _w(0.0)
    w[:, :3] = 2.0                       # positive only under the mask
    with pytest.raises(ValueError, match='loss_weights.*sum to 0'):
        _call(mask=mask, weights=w)
    with pytest.raises(ValueError, match='mask'):
        _call(mask=mask.T, weights=_w())


@pytest.mark.parametrize('what,lam', BAD_LAM, ids=[b[0] for b in BAD_LAM])
def test_masked_mse_refuses_bad_lead_weights_by_name(what, lam):
    with pytest.raises(ValueError, match='lead_weights'):
        _call(lead_weights=lam)
    with pytest.raises(ValueError, match='lead_weights'):
        _call(weights=_w(), lead_weights=lam)


def test_binary_takes_no_weights():
    for kw in (dict(weights=_w()), dict(lead_weights=np.ones(T_)), dict(weights=_w(), lead_weights=np.ones(T_))):
        with pytest.raises(ValueError, match='binary'):
            _call(binary=True, **kw)


def test_a_truncated_chunk_whose_lead_weights_vanish_is_refused_and_divisors_come_from_the_slices():
    from model.mpnnlstm import LossWeights
    lw = LossWeights(_w(2.0), [0.0, 0.0, 3.0, 0.5], (N_, M_), 4)
    assert lw.sum_lam == 3.5 and lw.sum_w == 2.0 * N_ * M_
    c = lw.chunk(range(2, 4))
    assert c.T == 2 and c.sum_lam == 3.5 and c.sum_w == lw.sum_w and list(c.lam_host) == [3.0, 0.5]
    assert lw.chunk(range(1, 3)).sum_lam == 3.0
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        lw.chunk(range(0, 2))


def test_trainer_methods_refuse_before_the_rollout_starts():
    """forward_loss / train_step / truncated_backward / make_graphed_step / train check the weights before the model runs: on a
    CPU-only predictor every one of them ends in the refusal, not in a missing-GPU error."""
    from helpers import TinyLoader
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    bad_w, bad_l = np.ones((64, 63), np.float32), [1.0, -1.0, 1.0]
    for kw, name in ((dict(loss_weights=bad_w), 'loss_weights'), (dict(lead_weights=bad_l), 'lead_weights')):
        with pytest.raises(ValueError, match=name):
            nfp.forward_loss(x, y, **kw)
        with pytest.raises(ValueError, match=name):
            nfp.truncated_backward(x, y, None, None, truncated_backprop=2, **kw)
        loader = TinyLoader([(x[None], y[None], torch.zeros(1))], (64, 64))
        with pytest.raises(ValueError, match=name):
            nfp.train(loader, loader, n_epochs=1, **kw)
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        nfp.truncated_backward(x, y, None, None, truncated_backprop=2, lead_weights=[1.0, 1.0, 0.0])
    import inspect
    for meth in ('forward_loss', 'train_step', 'truncated_backward', 'make_graphed_step', 'train'):
        names = list(inspect.signature(getattr(NextFramePredictorS2S, meth)).parameters)
        assert names[-2:] == ['loss_weights', 'lead_weights'], (meth, names)


def test_float64_model_at_unit_weights_is_the_unweighted_model():
    rng = np.random.default_rng(3)
    B, P, N = 2, 90, 17
    lab = rng.integers(-1, N, size=(B, P))
    lab[1] = np.where(lab[1] >= 0, (lab[1] + 3) % N, -1)
    o, y = rng.standard_normal(N), rng.standard_normal((B, P))
    keep = rng.random(P) < 0.8
    for kp in (None, keep):
        a = M.sse(o, lab, y, kp, g=0.37, W=4)
        b = WM.wsse(o, lab, y, np.ones(P), 1.0, kp, g=0.37, W=4)
        assert a[0] == pytest.approx(b[0], rel=1e-14) and a[1] == pytest.approx(b[1], rel=1e-14)
        np.testing.assert_allclose(b[2], a[2], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(b[3], a[3], rtol=1e-13)
    # a pixel weight of 0 is the pixel left out, a lead weight scales total and gradient
    w = np.where(keep, 1.0, 0.0)
    a, b = M.sse(o, lab, y, keep, g=1.0), WM.wsse(o, lab, y, w, 2.5, None, g=1.0)
    assert b[0] == pytest.approx(2.5 * a[0], rel=1e-14)
    np.testing.assert_allclose(b[2], 2.5 * a[2], rtol=1e-13, atol=1e-13)


def test_cell_area_weights():
    from model.utils import cell_area_weights
    lat = np.array([0.0, 60.0, -60.0, 70.0])
    w = cell_area_weights(lat, 5)
    assert w.shape == (4, 5) and w.dtype == np.float32 and abs(float(w.astype(np.float64).mean()) - 1.0) < 1e-6
    c = np.cos(np.deg2rad(lat))
    np.testing.assert_allclose(w, np.repeat((c / c.mean())[:, None], 5, 1), rtol=1e-6)
    assert np.all(w[:, 0:1] == w) and w[1, 0] == w[2, 0]
    assert abs(w[3, 0] / w[0, 0] - np.cos(np.deg2rad(70.0))) < 1e-6          # about a third of an equatorial cell
    for bad in ([], [95.0], [np.nan], [90.0, -90.0]):
        with pytest.raises(ValueError, match='latitudes'):
            cell_area_weights(bad, 4)


def test_wsse_entries_are_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    decls = header_decls()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('qt_wsse_rollout', 'qt_wsse_rollout_bwd'):
        assert re.match(r'int\s+%s\s*\(' % name, decls[name].text) and decls[name].times == 1, name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names(), name
    assert re.search(r'const float\s*\*\s*w\s*,\s*const float\s*\*\s*lam', decls['qt_wsse_rollout'].text)
    sse, wsse = _lib._SIGNATURES['qt_sse_rollout'], _lib._SIGNATURES['qt_wsse_rollout']
    assert wsse == sse[:10] + [ctypes.c_void_p, ctypes.c_void_p] + sse[10:]            # qt_sse_rollout's with (w, lam) after the strides
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme


def test_wsse_entries_refuse_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_void_p * 64)()
    x = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16         # only ever validated, never dereferenced
    one = (ctypes.c_int * 16)(*([1] * 16))
    ptrs = (ctypes.c_void_p * 16)(*([x] * 16))

    def fwd(nseg=1, outs=ptrs, strides=one, labels=ptrs, levels=ptrs, Ns=one, swys=ptrs, y=x, w=x, lam=x, B=1, n=8, m=8, part=x):
        return lib.qt_wsse_rollout(nseg, outs, strides, labels, levels, Ns, swys, y, 64, 64, w, lam, B, n, m, part, None)

    def bwd(nseg=1, outs=ptrs, strides=one, swys=ptrs, Ns=one, n_devs=ptrs, g=x, lam=x, W=1, gouts=ptrs):
        return lib.qt_wsse_rollout_bwd(nseg, outs, strides, swys, Ns, n_devs, g, lam, W, gouts, None)
    for kw in (dict(nseg=0), dict(nseg=17), dict(w=None), dict(lam=None), dict(y=None), dict(part=None), dict(B=0), dict(n=0),
               dict(m=-8), dict(swys=None), dict(swys=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())):
        assert fwd(**kw) != 0 and b'qt_wsse_rollout' in lib.qt_last_error(), kw
    for kw in (dict(nseg=0), dict(nseg=17), dict(lam=None), dict(g=None), dict(W=0), dict(gouts=None),
               dict(swys=(ctypes.c_void_p * 16)()), dict(Ns=(ctypes.c_int * 16)(*([1 << 30] * 16)), W=4)):
        assert bwd(**kw) != 0 and b'qt_wsse_rollout_bwd' in lib.qt_last_error(), kw
