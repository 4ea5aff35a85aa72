"""CPU-side checks of the weighted binary cross-entropy (no GPU): the float64 model tests/wbce_f64.py against tests/bce_f64.py at
unit weights and against torch's own binary_cross_entropy_with_logits(weight=, pos_weight=) in float64, the clamp convention on
saturated outputs, every refusal of masked_bce and of the trainer methods by name and before any launch, and the two entry points
in their header, the library and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bce_f64 as BM
import wbce_f64 as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, M_, T_ = 6, 8, 3


class StubMesh:
    """What masked_bce reads of a mesh before the first launch."""
    B, n, m, P, N, loss_mask = 1, N_, M_, N_ * M_, 5, None


def _case(seed, B=2, P=120, N=19):
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, N, size=(B, P))
    o = rng.uniform(0.02, 0.98, N).astype(np.float32).astype(np.float64)
    y = rng.choice([0.0, 1.0, 0.3, 0.75], size=(B, P))
    w = np.where(rng.random(P) < 0.2, 0.0, rng.uniform(0.25, 4.0, P))
    keep = rng.random(P) < 0.8
    return rng, lab, o, y, w, keep


def test_unit_weights_are_the_unweighted_model():
    _, lab, o, y, _, keep = _case(21)
    P = lab.shape[1]
    for kp in (None, keep):
        a = BM.bce(o, lab, y, kp, g=0.37, W=4)
        b = WB.wbce(o, lab, y, np.ones(P), 1.0, 1.0, kp, g=0.37, W=4)
        assert a[0] == pytest.approx(b[0], rel=1e-14) and a[1] == pytest.approx(b[1], rel=1e-14)
        np.testing.assert_allclose(b[2], a[2], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(b[3], a[3], rtol=1e-13)
    # a pixel weight of 0 is the pixel left out, a lead weight scales total and gradient, and lam = 0 leaves no term at all
    a = BM.bce(o, lab, y, keep, g=1.0)
    b = WB.wbce(o, lab, y, np.where(keep, 1.0, 0.0), 2.5, 1.0, None, g=1.0)
    assert b[0] == pytest.approx(2.5 * a[0], rel=1e-14)
    np.testing.assert_allclose(b[2], 2.5 * a[2], rtol=1e-13, atol=1e-13)
    z = WB.wbce(o, lab, y, np.ones(P), 0.0, 3.0, None, g=1.0, W=2)
    assert z[0] == 0 and z[1] == 0 and (z[2] == 0).all() and (z[3] == 0).all()


@pytest.mark.parametrize('pw', [3.0, 0.5, 1.0])
def test_float64_model_is_torchs_bce_with_logits(pw):
    """Unsaturated outputs: o = sigmoid(x) with x = logit(o), so torch's binary_cross_entropy_with_logits(x, y, weight=lam w,
    pos_weight=pw, reduction='sum') in float64 is the model's total and its autograd gradient with respect to o the model's row."""
    _, lab, o, y, w, keep = _case(31)
    lam, g = 1.75, 0.37
    for kp in (None, keep):
        total, mag, grad, gmag = WB.wbce(o, lab, y, w, lam, pw, kp, g=g, W=4)
        ot = torch.tensor(o, dtype=torch.float64, requires_grad=True)
        ok = lab >= 0
        if kp is not None:
            ok = ok & kp.reshape(1, -1)
        okt = torch.from_numpy(ok)
        img = ot[torch.from_numpy(np.where(ok, lab, 0))][okt]
        wt = torch.from_numpy(np.broadcast_to(lam * w.reshape(1, -1), lab.shape).copy())[okt]
        ref = torch.nn.functional.binary_cross_entropy_with_logits(torch.logit(img), torch.from_numpy(y)[okt], weight=wt,
                                                                   pos_weight=torch.tensor(pw, dtype=torch.float64), reduction='sum')
        (gref,) = torch.autograd.grad(ref * g, ot)
        assert mag >= abs(total) and total == pytest.approx(float(ref.detach()), rel=1e-12)
        np.testing.assert_allclose(grad[:, 0], gref.numpy(), rtol=1e-10, atol=1e-12 * np.abs(gref.numpy()).max())
        assert (grad[:, 1:] == 0).all() and (gmag[:, 1:] == 0).all() and (gmag[:, 0] >= np.abs(grad[:, 0])).all()
        # a node whose counted pixels all have weight 0 has no terms
        sw = np.zeros(o.shape[0])
        np.add.at(sw, lab[ok], np.broadcast_to(w.reshape(1, -1), lab.shape)[ok])
        assert ((gmag[:, 0] == 0) == (sw == 0)).all()


def test_saturated_outputs_follow_the_clamp():
    """o = 0 and o = 1: the logarithms are clamped at -100 before the products (pw times 100 per unit of w for o = 0 under y = 1,
    100 for o = 1 under y = 0, nothing for o = 0 under y = 0), and the gradient's denominator at 1e-12."""
    lab = np.array([[0, 1, 2, 3]])
    w, pw, lam = np.array([2.0, 0.5, 3.0, 1.5]), 3.0, 0.25
    total, mag, grad, gmag = WB.wbce([0.0, 1.0, 0.0, 1.0], lab, [[1.0, 0.0, 0.0, 1.0]], w, lam, pw, g=1.0)
    assert total == lam * (2.0 * pw * 100.0 + 0.5 * 100.0)
    assert mag == total + lam * 1.5 * 200.0          # (o = 1 under y = 1: the terms L0 and -y L0 are added and cancel)
    assert np.isfinite(grad).all() and grad[2, 0] == 0 and grad[3, 0] == 0
    assert grad[0, 0] == pytest.approx(-lam * 2.0 * pw / BM.EPS) and grad[1, 0] == pytest.approx(lam * 0.5 / BM.EPS)
    # at pw = 1 and unit weights this is torch's BCELoss with its clamp
    ref = torch.nn.functional.binary_cross_entropy(torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float64),
                                                   torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=torch.float64), reduction='sum')
    assert WB.wbce([0.0, 1.0, 0.0, 1.0], lab, [[1.0, 0.0, 0.0, 1.0]], np.ones(4), 1.0, 1.0)[0] == float(ref) == 200.0


# ---- refusals: by name, before any launch (CPU tensors and a stub mesh: a launch would fail, a refusal comes first) ----
def _call(y=None, mask=None, **kw):
    from model.mpnnlstm import masked_bce
    outs = [torch.full((StubMesh.N, 1), 0.5) for _ in range(T_)]
    return masked_bce(outs, [StubMesh] * T_, torch.zeros(1, T_, N_, M_, 1) if y is None else y, mask, **kw)


def _w(fill=1.0):
    return np.full((N_, M_), fill, np.float32)


BAD_W = [('transposed', _w().T), ('flat', _w().reshape(-1)), ('frame stack', np.ones((1, N_, M_), np.float32)),
         ('nan', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, np.nan, 1.0)),
         ('inf', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, np.inf, 1.0)),
         ('negative', np.where(np.arange(N_ * M_).reshape(N_, M_) == 7, -0.5, 1.0)), ('zeros', _w(0.0))]
BAD_LAM = [('too long', np.ones(T_ + 1)), ('2-d', np.ones((T_, 1))), ('scalar', np.float32(1.0)), ('negative', [1.0, -1.0, 1.0]),
           ('nan', [1.0, np.nan, 1.0]), ('inf', [np.inf, 1.0, 1.0]), ('zeros', [0.0, 0.0, 0.0])]
BAD_PW = [('zero', 0.0), ('negative', -2.0), ('nan', float('nan')), ('inf', float('inf')), ('array', np.array([1.0, 2.0])),
          ('0-d array', np.array(2.0)), ('list', [3.0]), ('tensor', torch.tensor(3.0)), ('string', '3'), ('bool', True),
          ('beyond float32', 1e39), ('float32 underflow', 1e-46)]


@pytest.mark.parametrize('what,w', BAD_W, ids=[b[0] for b in BAD_W])
def test_masked_bce_refuses_bad_pixel_weights_by_name(what, w):
    with pytest.raises(ValueError, match='loss_weights'):
        _call(weights=w)
    with pytest.raises(ValueError, match='loss_weights'):
        _call(weights=torch.as_tensor(np.asarray(w)), lead_weights=np.ones(T_), pos_weight=3.0)


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
def test_masked_bce_refuses_bad_lead_weights_by_name(what, lam):
    with pytest.raises(ValueError, match='lead_weights'):
        _call(lead_weights=lam)
    with pytest.raises(ValueError, match='lead_weights'):
        _call(weights=_w(), lead_weights=lam)


@pytest.mark.parametrize('what,pw', BAD_PW, ids=[b[0] for b in BAD_PW])
def test_masked_bce_refuses_a_bad_pos_weight_by_name(what, pw):
    from qtmpnn import ops
    with pytest.raises(ValueError, match='pos_weight'):
        _call(pos_weight=pw)
    with pytest.raises(ValueError, match='pos_weight'):
        _call(weights=_w(), lead_weights=np.ones(T_), pos_weight=pw)
    outs = [torch.full((StubMesh.N, 1), 0.5)]
    with pytest.raises(ValueError, match='pos_weight'):
        ops.rollout_wbce_partials(outs, torch.zeros(1, 1, N_ * M_), [StubMesh], torch.ones(N_ * M_), torch.ones(1), pw)
    with pytest.raises(ValueError, match='pos_weight'):
        ops.step_wbce_partials(outs[0], torch.zeros(1, N_ * M_), StubMesh, torch.ones(N_ * M_), torch.ones(()), pw)


@pytest.mark.parametrize('shape', [(1, T_ + 1, N_, M_, 1), (1, T_, M_, N_, 1), (2, T_, N_, M_, 1), (T_, N_, M_, 2), (1, T_, N_, M_)])
def test_masked_bce_refuses_wrong_target_shapes_before_any_launch(shape):
    with pytest.raises(ValueError, match='targets of shape'):
        _call(y=torch.zeros(*shape), weights=_w(), pos_weight=2.0)


def test_good_arguments_reach_the_launch():
    """The refusals above are refusals of their arguments: with good ones it is the stub mesh that fails (it has no label map)."""
    for kw in (dict(), dict(weights=_w(), lead_weights=np.ones(T_), pos_weight=np.float32(2.0)), dict(pos_weight=3)):
        with pytest.raises(AttributeError, match='labels'):
            _call(**kw)


def _cpu_predictor(binary):
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None, binary=binary,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))


def _trainer_calls(nfp, **kw):
    """Every trainer method that takes the weights, as a thunk: on a CPU-only predictor each ends in its refusal, not in a
    missing-GPU error."""
    from helpers import TinyLoader
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    loader = TinyLoader([(x[None], y[None], torch.zeros(1))], (64, 64))
    return [lambda: nfp.forward_loss(x, y, **kw), lambda: nfp.train_step(x, y, **kw),
            lambda: nfp.truncated_backward(x, y, None, None, truncated_backprop=2, **kw),
            lambda: nfp.train(loader, loader, n_epochs=1, **kw)]


def test_binary_trainer_methods_refuse_before_the_rollout_starts():
    nfp = _cpu_predictor(True)
    bad_w, bad_l = np.ones((64, 63), np.float32), [1.0, -1.0, 1.0]
    for kw, name in ((dict(loss_weights=bad_w), 'loss_weights'), (dict(lead_weights=bad_l), 'lead_weights'),
                     (dict(pos_weight=0.0), 'pos_weight'), (dict(pos_weight=float('nan')), 'pos_weight'),
                     (dict(pos_weight=np.array([1.0, 2.0])), 'pos_weight'),
                     (dict(loss_weights=np.ones((64, 64), np.float32), pos_weight=-1.0), 'pos_weight')):
        for call in _trainer_calls(nfp, **kw):
            with pytest.raises(ValueError, match=name):
                call()
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        nfp.truncated_backward(x, y, None, None, truncated_backprop=2, lead_weights=[1.0, 1.0, 0.0], pos_weight=2.0)
    import inspect
    from model.mpnnlstm import NextFramePredictorS2S
    for meth in ('forward_loss', 'train_step', 'truncated_backward', 'make_graphed_step', 'train'):
        assert inspect.signature(getattr(NextFramePredictorS2S, meth)).parameters['pos_weight'].default is None, meth


def test_pos_weight_on_a_non_binary_predictor_is_refused_by_name():
    nfp = _cpu_predictor(False)
    for kw in (dict(pos_weight=2.0), dict(pos_weight=2.0, loss_weights=np.ones((64, 64), np.float32))):
        for call in _trainer_calls(nfp, **kw):
            with pytest.raises(ValueError, match='pos_weight.*binary'):
                call()


def test_loss_weights_carry_pos_weight_through_chunks():
    from model.mpnnlstm import LossWeights, bce_weights_of
    assert bce_weights_of(None, None, None, (N_, M_), 4) is None
    lw = bce_weights_of(None, [0.0, 0.0, 3.0, 0.5], 3, (N_, M_), 4)
    assert isinstance(lw, LossWeights) and lw.pos_weight == 3.0 and lw.sum_lam == 3.5 and lw.sum_w == N_ * M_
    c = lw.chunk(range(2, 4))
    assert c.pos_weight == 3.0 and c.sum_lam == 3.5 and list(c.lam_host) == [3.0, 0.5]
    assert bce_weights_of(lw, None, None, (N_, M_), 4) is lw
    other = bce_weights_of(lw, None, 0.5, (N_, M_), 4)
    assert other.pos_weight == 0.5 and lw.pos_weight == 3.0 and other.w_host is lw.w_host
    only_pw = bce_weights_of(None, None, 2.0, (N_, M_), 4)
    assert only_pw.pos_weight == 2.0 and (only_pw.w_host == 1).all() and (only_pw.lam_host == 1).all()
    with pytest.raises(ValueError, match='lead_weights.*chunk'):
        lw.chunk(range(0, 2))


# ---- the two entry points ----
def test_wbce_entries_are_declared_exported_and_bound():
    from helpers import binding_kinds, header_decls
    from qtmpnn import _lib
    decls = header_decls()
    assert {n for n in decls if 'wbce' in n} == {n for n in _lib._SIGNATURES if 'wbce' in n} == {'qt_wbce_rollout', 'qt_wbce_rollout_bwd'}
    lib, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, like in (('qt_wbce_rollout', 'qt_wsse_rollout'), ('qt_wbce_rollout_bwd', 'qt_wsse_rollout_bwd')):
        decl = decls[name]
        assert re.match(r'int\s+%s\s*\(' % name, decl.text) and decl.times == 1, name
        sig = _lib._SIGNATURES[name]
        assert decl.kinds == binding_kinds(sig), name
        assert re.match(r'float\s+pos_weight$', decl.params[-2]) and re.match(r'void\s*\*\s*stream$', decl.params[-1]), decl.params[-2:]
        # the arguments of the weighted squared-error pair, then pos_weight by value, then the stream
        assert sig == _lib._SIGNATURES[like][:-1] + [ctypes.c_float, ctypes.c_void_p]
        assert decl.params[:-2] == decls[like].params[:-1], name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names()
        assert getattr(bound, name).argtypes == sig and getattr(bound, name).restype is ctypes.c_int
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme and not re.search(r'qtmpnn_\w+\.h', readme)


def test_wbce_entries_refuse_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_void_p * 64)()
    x = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16         # only ever validated, never dereferenced
    one = (ctypes.c_int * 16)(*([1] * 16))
    ptrs = (ctypes.c_void_p * 16)(*([x] * 16))

    def fwd(nseg=1, outs=ptrs, strides=one, labels=ptrs, levels=ptrs, Ns=one, swys=ptrs, y=x, w=x, lam=x, B=1, n=8, m=8, part=x, pw=1.0):
        return lib.qt_wbce_rollout(nseg, outs, strides, labels, levels, Ns, swys, y, 64, 64, w, lam, B, n, m, part, pw, None)

    def bwd(nseg=1, outs=ptrs, strides=one, swys=ptrs, Ns=one, n_devs=ptrs, g=x, lam=x, W=1, gouts=ptrs, pw=1.0):
        return lib.qt_wbce_rollout_bwd(nseg, outs, strides, swys, Ns, n_devs, g, lam, W, gouts, pw, None)
    bad_pw = [dict(pw=0.0), dict(pw=-1.0), dict(pw=float('nan')), dict(pw=float('inf')), dict(pw=-float('inf'))]
    for kw in [dict(nseg=0), dict(nseg=17), dict(w=None), dict(lam=None), dict(y=None), dict(part=None), dict(B=0), dict(n=0),
               dict(m=-8), dict(swys=None), dict(swys=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())] + bad_pw:
        assert fwd(**kw) != 0 and b'qt_wbce_rollout' in lib.qt_last_error(), kw
        if 'pw' in kw:
            assert b'pos_weight' in lib.qt_last_error(), kw
    for kw in [dict(nseg=0), dict(nseg=17), dict(lam=None), dict(g=None), dict(W=0), dict(gouts=None),
               dict(swys=(ctypes.c_void_p * 16)()), dict(Ns=(ctypes.c_int * 16)(*([1 << 30] * 16)), W=4)] + bad_pw:
        assert bwd(**kw) != 0 and b'qt_wbce_rollout_bwd' in lib.qt_last_error(), kw
        if 'pw' in kw:
            assert b'pos_weight' in lib.qt_last_error(), kw
