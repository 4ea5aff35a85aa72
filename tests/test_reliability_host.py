"""CPU-side checks of the probability verification (no GPU): the qt_reliability_rollout entry and its argument checks, the numpy
restatement on a case worked out by hand, and qtmpnn.reliability.Reliability against numbers worked out by hand from a small
array of sums (curve, Brier score and its decomposition with the binning residual, skill, ROC, pooling, refusals)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from reliability_restated import bin_of, restated_reliability

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reliability_entry_is_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    name = 'qt_reliability_rollout'
    decls = header_decls()
    decl = decls[name]
    assert re.match(r'int\s+qt_reliability_rollout\s*\(', decl.text) and decl.times == 1
    assert re.search(r'int\s+m\s*,\s*int\s+bins\s*,\s*float\s*\*\s*partial\s*,\s*void\s*\*\s*stream\s*\)', decl.text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names()
    # the arguments up to m are qt_score_rollout's; then bins, partial, stream
    score, rel = _lib._SIGNATURES['qt_score_rollout'], _lib._SIGNATURES[name]
    assert decl.params[:20] == decls['qt_score_rollout'].params[:20]
    assert rel[:20] == score[:20] and rel[20:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert score[20:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_reliability_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.5, B=1, n=8, m=8, bins=10, partial=x):
        rc = lib.qt_reliability_rollout(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm,
                                        thr, B, n, m, bins, partial, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(outs=None), dict(strides=None), dict(labels=None), dict(Ns=None),
           dict(n_devs=None), dict(y=None), dict(partial=None),
           dict(B=0), dict(B=-3), dict(B=65536), dict(n=0), dict(m=0), dict(m=-8),
           dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1), dict(b1=x, b1ss=-1), dict(b2=x, b2cs=-1), dict(b2=x, b2ss=-1),
           dict(bins=1), dict(bins=0), dict(bins=-10), dict(bins=33), dict(bins=1 << 20),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_reliability_rollout' in err, (kw, rc, err)
    # the shared refusals carry this entry's name, its own say what is wrong
    assert b'qt_reliability_rollout: nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(b2=x, b2ss=-1)[1]
    assert b'bad segment' in call(strides=(ctypes.c_int * 16)())[1]
    assert b'bins must be 2..32' in call(bins=1)[1] and b'bins must be 2..32' in call(bins=33)[1]
    assert b'partial' in call(partial=None)[1]
    assert b'bad sizes' in call(B=0)[1]
    # all NULL, as every other entry is refused on a machine without a GPU
    assert lib.qt_reliability_rollout(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.5, 1, 8, 8,
                                      10, None, None) == -1
    assert b'qt_reliability_rollout' in lib.qt_last_error()


def test_bin_rule_at_the_edges():
    """K = 10: t = f * 10 in fp32.  Whether the product of an fp32 value near an edge reaches the integer is the fp32
    product's business; the rule only reads it."""
    f32, down = np.float32, lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    vals = np.array([0.0, -0.0, -0.25, -np.inf, np.nan, 0.05, down(0.1), 0.1, 0.25, 0.5, down(0.5), 0.9, down(1.0), 1.0, 1.5,
                     np.inf, 3.0e38], np.float32)
    got = bin_of(vals, 10).tolist()
    want = []
    for v in vals:                                   # the rule again, scalar by scalar, in np.float32
        with np.errstate(over='ignore', invalid='ignore'):
            t = f32(v) * f32(10)
        want.append(0 if not t >= f32(1) else 9 if t >= f32(10) else int(t))
    assert got == want
    # ... and by hand where the product is exact or far from an integer
    by_hand = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 8: 2, 9: 5, 11: 9, 13: 9, 14: 9, 15: 9, 16: 9}
    for i, k in by_hand.items():
        assert got[i] == k, (i, vals[i], got[i], k)
    # the value just below 0.5 is 0.5 - 2^-25; times 10 that is 5 - 1.25 * 2^-22, between the fp32 neighbours 5 - 2^-21 and 5
    # and nearer the lower one: bin 4
    assert got[10] == 4
    # K = 2 and K = 32 are powers of two: t is exact, so an edge k / K is in bin k and its lower neighbour in bin k - 1
    for K in (2, 32):
        edges = (np.arange(1, K, dtype=np.float32) / np.float32(K)).astype(np.float32)
        assert bin_of(edges, K).tolist() == list(range(1, K))
        assert bin_of(np.nextafter(edges, np.float32(-np.inf)), K).tolist() == list(range(0, K - 1))
        assert bin_of(np.array([1.0, 2.0, -1.0], np.float32), K).tolist() == [K - 1, K - 1, 0]


def test_restated_reliability_on_a_case_worked_out_by_hand():
    """2 x 4 frame, T = 1, K = 4 (t = 4 f is exact), thr = 0.5, pixel (1, 3) masked.
        f      0.25   0.25-   -0.5   1.5    | 0.5    0.75   0.0    (masked)
        bin    1      0       0      3      | 2      3      0
        y      0.5    0.9     0.1    0.7    | 0.6    0.2    0.5001
        o      0      1       0      1      | 1      0      1         (y == thr is no event: strict >)
    bin 0: f = 0.25-, -0.5, 0 with o = 1, 0, 1: n 3, events 2, sum f = 0.25- - 0.5, sum (f-o)^2 = (0.25- - 1)^2 + 0.25 + 1
    bin 1: f = 0.25, o = 0: n 1, events 0, 0.25, 0.0625
    bin 2: f = 0.5, o = 1: n 1, events 1, 0.5, 0.25
    bin 3: f = 1.5, 0.75 with o = 1, 0: n 2, events 1, 2.25, 0.25 + 0.5625"""
    lo = np.nextafter(np.float32(0.25), np.float32(0))
    f = np.array([[[0.25, lo, -0.5, 1.5], [0.5, 0.75, 0.0, 0.3]]], np.float32)
    y = np.array([[[0.5, 0.9, 0.1, 0.7], [0.6, 0.2, 0.5001, 0.9]]], np.float32)
    mask = np.array([[False] * 4, [False, False, False, True]])
    sums, absterms = restated_reliability(f, y, mask, 0.5, 4)
    assert sums.shape == (1, 4, 4) and absterms.shape == (1, 4, 2) and sums.dtype == np.float64
    lo64 = float(lo)
    want = [[3, 2, lo64 - 0.5, (lo64 - 1) ** 2 + 0.25 + 1.0], [1, 0, 0.25, 0.0625], [1, 1, 0.5, 0.25], [2, 1, 2.25, 0.8125]]
    np.testing.assert_array_equal(sums[0], np.array(want))
    np.testing.assert_array_equal(absterms[0, :, 0], [lo64 + 0.5, 0.25, 0.5, 2.25])
    np.testing.assert_array_equal(absterms[0, :, 1], sums[0, :, 3])
    # without the mask (1, 3) is counted: f = 0.3 -> bin 1, o = 1
    s2, _ = restated_reliability(f, y, None, 0.5, 4)
    assert s2[0, 1, :2].tolist() == [2, 1] and s2[0, :, 0].sum() == 8
    # a NaN forecast is counted in bin 0 and makes its float sums NaN, no other bin's
    fn = f.copy()
    fn[0, 0, 3] = np.nan
    s3, _ = restated_reliability(fn, y, mask, 0.5, 4)
    assert s3[0, :, 0].tolist() == [4, 1, 1, 1] and s3[0, :, 1].tolist() == [3, 0, 1, 0]
    assert np.isnan(s3[0, 0, 2:]).all() and np.isfinite(s3[0, 1:]).all()


def _hand_sums():
    """Two clips, one lead time, sources model / climatology, K = 4 (edges 0, .25, .5, .75, 1).  Pooled model sums per bin:
        bin   n    events  sum f   sum (f-o)^2
        0     10   1       1.0     1.0
        1     0    0       0       0            (empty)
        2     4    2       2.5     1.25
        3     6    5       5.5     1.25
    climatology: one constant forecast 0.4 in bin 1, n = 20, events = 8: sum f = 8, sum (f-o)^2 = 12 * 0.16 + 8 * 0.36 = 4.8."""
    s = np.zeros((2, 1, 2, 4, 4))
    s[0, 0, 0] = [[6, 1, 0.75, 0.875], [0, 0, 0, 0], [3, 1, 1.75, 0.75], [1, 1, 1.0, 0.0]]
    s[1, 0, 0] = [[4, 0, 0.25, 0.125], [0, 0, 0, 0], [1, 1, 0.75, 0.5], [5, 4, 4.5, 1.25]]
    s[0, 0, 1, 1] = [10, 3, 4.0, 7 * 0.16 + 3 * 0.36]
    s[1, 0, 1, 1] = [10, 5, 4.0, 5 * 0.16 + 5 * 0.36]
    return s


def test_curve_brier_and_decomposition_by_hand():
    from qtmpnn.reliability import SLOTS, Reliability
    assert SLOTS == ('n', 'events', 'sum_f', 'sum_sq_err')
    r = Reliability(_hand_sums(), ('model', 'climatology'), 0.5)
    assert r.bins == 4 and r.threshold == 0.5 and r.sums.dtype == np.float64
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        c = r.curve('model')
        lead = r.by_lead('model')
        b = r.brier('model')
    assert c['edges'].tolist() == [0, 0.25, 0.5, 0.75, 1.0]
    assert c['n'].tolist() == [[10, 0, 4, 6]]
    np.testing.assert_array_equal(c['mean_forecast'][0, [0, 2, 3]], [0.1, 0.625, 5.5 / 6])
    np.testing.assert_array_equal(c['observed_frequency'][0, [0, 2, 3]], [0.1, 0.5, 5 / 6])
    assert np.isnan(c['mean_forecast'][0, 1]) and np.isnan(c['observed_frequency'][0, 1])
    # per (clip, lead): clip 0 has 10 pixels and SSE 1.625, clip 1 has 10 and 1.875; pooled 3.5 / 20, not the mean of ratios
    # of unequal clips -- here the clips are equal in size, so pool a second Reliability with clip 1 doubled below
    assert b.shape == (2, 1) and b[:, 0].tolist() == [0.1625, 0.1875]
    assert lead['n'].tolist() == [20] and lead['brier'].tolist() == [0.175] and lead['base_rate'].tolist() == [0.4]
    # reliability = (10 (0.1 - 0.1)^2 + 4 (0.625 - 0.5)^2 + 6 (5.5/6 - 5/6)^2) / 20
    rel = (4 * 0.125 ** 2 + 6 * (5.5 / 6 - 5 / 6) ** 2) / 20
    # resolution = (10 (0.1 - 0.4)^2 + 4 (0.5 - 0.4)^2 + 6 (5/6 - 0.4)^2) / 20
    res = (10 * (0.1 - 0.4) ** 2 + 4 * (0.5 - 0.4) ** 2 + 6 * (5 / 6 - 0.4) ** 2) / 20
    np.testing.assert_allclose(lead['reliability'], [rel], rtol=1e-14)
    np.testing.assert_allclose(lead['resolution'], [res], rtol=1e-14)
    np.testing.assert_allclose(lead['uncertainty'], [0.24], rtol=1e-14)
    # the binned terms do not add up to the Brier score: what is left is reported, and it is not zero here
    np.testing.assert_allclose(lead['residual'], [0.175 - (rel - res + 0.24)], rtol=0, atol=1e-15)
    assert abs(lead['residual'][0]) > 1e-3
    # a constant forecast has no within-bin spread: the decomposition is exact, resolution 0
    cl = r.by_lead('climatology')
    np.testing.assert_allclose(cl['brier'], [0.24], rtol=1e-14)
    np.testing.assert_allclose([cl['reliability'][0], cl['resolution'][0], cl['uncertainty'][0]], [0.0, 0.0, 0.24], atol=1e-15)
    assert abs(cl['residual'][0]) < 1e-15
    # pooling is of sums: with clips of unequal size the pooled Brier score is not the mean of the clips'
    s = _hand_sums()
    s[1] *= 3
    r3 = Reliability(s, ('model', 'climatology'), 0.5)
    pooled = (1.625 + 3 * 1.875) / 40
    assert r3.by_lead('model')['brier'].tolist() == [pooled] and pooled != r3.brier('model').mean()


def test_skill_by_hand_and_where_the_reference_is_perfect():
    from qtmpnn.reliability import Reliability
    s = np.concatenate([_hand_sums(), _hand_sums()], axis=1)           # a second lead time ...
    s[:, 1, 1, :, 3] = 0                                              # ... at which the reference's Brier score is 0
    r = Reliability(s, ('model', 'climatology'), 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sk = r.skill()
        same = r.skill('model', 'model')
    np.testing.assert_allclose(sk[0], 1 - 0.175 / 0.24, rtol=1e-14)
    assert np.isnan(sk[1]) and sk.shape == (2,)
    assert same.tolist() == [0.0, 0.0]
    only = Reliability(s[:, :, :1], ('model',), 0.5)
    with pytest.raises(KeyError, match='skill: no source .climatology.'):
        only.skill()
    with pytest.raises(KeyError, match='skill: no source .persistence.'):
        r.skill('persistence')


def test_roc_by_hand():
    """Model of _hand_sums: events per bin 1, 0, 2, 5 (8), non-events 9, 0, 2, 1 (12).  "yes" iff bin >= k:
    k = 0: (1, 1); k = 1 and 2: pod 7/8, pofd 3/12; k = 3: 5/8, 1/12; k = 4: (0, 0)."""
    from qtmpnn.reliability import Reliability
    r = Reliability(_hand_sums(), ('model', 'climatology'), 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        roc = r.roc('model')
    assert roc['thresholds'].tolist() == [0, 0.25, 0.5, 0.75, 1.0]
    assert roc['pod'].tolist() == [[1.0, 7 / 8, 7 / 8, 5 / 8, 0.0]]
    assert roc['pofd'].tolist() == [[1.0, 3 / 12, 3 / 12, 1 / 12, 0.0]]
    assert (np.diff(roc['pod'], axis=-1) <= 0).all() and (np.diff(roc['pofd'], axis=-1) <= 0).all()
    auc = (1 - 3 / 12) * (1 + 7 / 8) / 2 + 0 + (3 / 12 - 1 / 12) * (7 / 8 + 5 / 8) / 2 + (1 / 12) * (5 / 8) / 2
    np.testing.assert_allclose(roc['auc'], [auc], rtol=1e-14)
    assert 'f * K >= k' in Reliability.roc.__doc__ and 'strict' in Reliability.roc.__doc__
    # a lead time without events (or without non-events) has no ROC
    s = _hand_sums()
    s[..., 1] = 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        none = Reliability(s, ('model', 'climatology'), 0.5).roc('model')
    assert np.isnan(none['pod']).all() and np.isnan(none['auc']).all() and none['pofd'][0, 0] == 1.0


def test_reliability_refuses_by_name():
    from qtmpnn.reliability import Reliability
    s = _hand_sums()
    src = ('model', 'climatology')
    for bad in (s[0], s[..., :3], s[:, :, :1], s.reshape(2, 1, 2, 16)):
        with pytest.raises(ValueError, match='Reliability: sums of shape'):
            Reliability(bad, src, 0.5)
    with pytest.raises(ValueError, match='Reliability: 1 bins'):
        Reliability(s[:, :, :, :1], src, 0.5)
    with pytest.raises(ValueError, match='Reliability: 33 bins'):
        Reliability(np.zeros((1, 1, 2, 33, 4)), src, 0.5)
    with pytest.raises(ValueError, match='Reliability: sources'):
        Reliability(s, ('model', 'model'), 0.5)
    r = Reliability(s, src, 0.5)
    for fn in (r.curve, r.brier, r.by_lead, r.roc):
        with pytest.raises(KeyError, match='persistence'):
            fn('persistence')


def test_bins_are_checked_on_the_host_by_name():
    from qtmpnn import ops
    for bad in (1, 33, 10.0, '10', None, True, 0, -4):
        with pytest.raises(ValueError, match='somewhere: bins must be an integer in 2..32'):
            ops.check_bins('somewhere', bad)
    assert ops.check_bins('x', 2) == 2 and ops.check_bins('x', 32) == 32
    # before anything else is looked at: no outputs, no meshes, no device
    with pytest.raises(ValueError, match='rollout_reliability: bins must be'):
        ops.rollout_reliability([], [], None, bins=33)


def test_reliability_is_a_method_beside_score():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    from qtmpnn.reliability import Reliability
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    rel = inspect.signature(NextFramePredictorS2S.reliability).parameters
    assert list(rel) == list(score) + ['bins']
    for name, p in score.items():
        assert rel[name].default == p.default, name
    assert rel['bins'].default == 10
    graphed = inspect.signature(NextFramePredictorS2S.make_graphed_reliability).parameters
    assert list(graphed)[:4] == ['self', 'x', 'y', 'concat_layers'] and list(graphed)[-2:] == ['threshold', 'bins']
    assert list(inspect.signature(ops.rollout_reliability).parameters) == ['outputs', 'meshes', 'y', 'threshold', 'bins',
                                                                           'persistence', 'climatology', 'per_tile']
    assert list(inspect.signature(mpnnlstm.reliability_product).parameters) == ['threshold', 'bins']
    assert list(inspect.signature(Reliability.__init__).parameters) == ['self', 'sums', 'sources', 'threshold']
