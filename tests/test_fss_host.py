"""CPU-side checks of the neighbourhood verification (no GPU): the numpy restatement of tests/fss_restated.py against a
brute-force triple loop and against score()'s table at scale 1, qtmpnn.fss.FSS on numbers worked out by hand (perfect forecast,
no ice, pooling, the useful scale, refusals), ops.check_scales, and the qt_fss_rollout entry with its argument checks."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from fss_restated import indicator, restated_fss, window_counts
from score_restated import restated_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (1, 3, 5, 9, 17, 33)


def _frame_7x9():
    """(T = 3, 7, 9) fields around thr = 0.5 with thr itself, NaN and inf in them, a mask and per-step uncounted pixels."""
    rng = np.random.default_rng(5)
    f = rng.random((3, 7, 9)).astype(np.float32)
    y = rng.random((3, 7, 9)).astype(np.float32)
    f[0, 0, 0], f[1, 3, 4], f[2, 6, 8], f[0, 2, 2] = 0.5, np.nan, np.inf, -np.inf
    y[0, 6, 0], y[1, 0, 8], y[2, 3, 3] = 0.5, np.nan, np.nextafter(np.float32(0.5), np.float32(1))
    mask = np.zeros((7, 9), dtype=bool)
    mask[0, 3:6] = mask[4, 4] = mask[6, 0] = True
    counted = rng.random((3, 7, 9)) > 0.15
    counted[:, 3, 4] = [True, True, False]
    return f, y, mask, counted


def _brute(field, truth, mask, thr, scales, counted):
    """The definition, pixel by pixel: for every counted centre, every scale, every window position."""
    T, W, H = field.shape
    t32 = np.float32(thr)
    out = np.zeros((T, len(scales), 5), dtype=np.int64)
    for t in range(T):
        ok = lambda r, c: 0 <= r < W and 0 <= c < H and bool(counted[t, r, c]) and not mask[r, c]
        for k, n in enumerate(scales):
            h = n // 2
            for r in range(W):
                for c in range(H):
                    if not ok(r, c):
                        continue
                    cs = co = 0
                    for dr in range(-h, h + 1):
                        for dc in range(-h, h + 1):
                            if ok(r + dr, c + dc):
                                cs += int(field[t, r + dr, c + dc] > t32)
                                co += int(truth[t, r + dr, c + dc] > t32)
                    out[t, k] += [1, int(truth[t, r, c] > t32), (cs - co) ** 2, cs * cs, co * co]
    return out


def test_restatement_equals_the_brute_force_loop():
    f, y, mask, counted = _frame_7x9()
    scales = (1, 3, 5, 33)                                   # 33: a window larger than the frame
    with np.errstate(invalid='ignore'):
        want = _brute(f, y, mask, 0.5, scales, counted)
    got = restated_fss(f, y, mask, 0.5, scales, counted)
    assert got.dtype == np.int64 and got.shape == (3, 4, 5)
    np.testing.assert_array_equal(got, want)
    keep = counted & ~mask
    assert (~keep).any() and (want[:, 0, 0] == keep.sum(axis=(1, 2))).all() and (want[:, :, 1] > 0).all()
    # the whole-frame window: every counted centre sees every ice pixel
    io = indicator(y[0], keep[0], 0.5)
    assert got[0, 3, 4] == keep[0].sum() * io.sum() ** 2
    # NaN, thr itself and -inf are not ice; +inf and the fp32 value above thr are
    assert indicator(f[1], keep[1], 0.5)[3, 4] == 0 and indicator(f[0], keep[0], 0.5)[0, 0] == 0
    assert indicator(f[2], keep[2], 0.5)[6, 8] == int(keep[2, 6, 8]) and indicator(y[2], keep[2], 0.5)[3, 3] == int(keep[2, 3, 3])
    # window_counts pads with zeros: a field of ones gives the window's area inside the frame
    np.testing.assert_array_equal(window_counts(np.ones((2, 3), np.int64), 3), [[4, 6, 4], [4, 6, 4]])


def test_scale_1_is_the_contingency_table():
    """n = 1: c = I, so sum (c_s - c_o)^2 = over + under, sum c_s^2 = hits + over, sum c_o^2 = hits + under = events."""
    f, y, mask, _ = _frame_7x9()
    f, y = np.nan_to_num(f, nan=0.25), np.nan_to_num(y, nan=0.75)
    got = restated_fss(f, y, mask, 0.5, (1, 3))[:, 0]
    table = restated_sums(f, y, mask, 0.5)[0]                # [n, ., ., ., hits, over, under, correct negatives]
    hits, over, under = table[:, 4], table[:, 5], table[:, 6]
    np.testing.assert_array_equal(got[:, 0], table[:, 0])
    np.testing.assert_array_equal(got[:, 2], over + under)
    np.testing.assert_array_equal(got[:, 3], hits + over)
    np.testing.assert_array_equal(got[:, 4], hits + under)
    np.testing.assert_array_equal(got[:, 1], got[:, 4])
    assert (over + under > 0).all() and (hits > 0).all()


def _sums(rows):
    """(n_clips, 1, 1, K, 5) from per-clip lists of K slot rows."""
    return np.array(rows, dtype=np.int64)[:, None, None]


def test_fss_perfect_forecast_no_ice_and_pooling():
    from qtmpnn.fss import SLOTS, FSS
    assert SLOTS == ('n', 'events', 'sum_sq_diff', 'sum_sq_f', 'sum_sq_o')
    # a perfect forecast through the restatement: the field is the truth
    f, y, mask, counted = _frame_7x9()
    s = restated_fss(y, y, mask, 0.5, (1, 5), counted)
    perfect = FSS(s[None, :, None], ('model',), 0.5, (1, 5))
    assert (perfect.fss('model') == 1.0).all() and perfect.fss().shape == (1, 3, 2)
    # no ice in either field: NaN, without a warning; ice in one of them only: 0
    none = FSS(_sums([[[50, 0, 0, 0, 0], [50, 0, 0, 0, 0]]]), ('model',), 0.5, (1, 3))
    only_f = FSS(_sums([[[50, 0, 7, 7, 0], [50, 0, 40, 40, 0]]]), ('model',), 0.5, (1, 3))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.isnan(none.fss()).all() and np.isnan(none.by_lead()['fss']).all()
        assert np.isnan(none.by_lead()['useful_scale']).all() and none.by_lead()['base_rate'].tolist() == [0.0]
        assert (only_f.fss() == 0.0).all()
    # two clips whose mean of ratios differs from the pooled ratio: clip 0 1 - 2 / (4 + 4) = 0.75, clip 1 1 - 30 / (20 + 20) = 0.25,
    # pooled 1 - 32 / 48 = 1 / 3 (mean of ratios 0.5)
    two = FSS(_sums([[[10, 4, 2, 4, 4]], [[30, 20, 30, 20, 20]]]), ('model',), 0.5, (1,))
    assert two.sums.dtype == np.int64 and two.sums.shape == (2, 1, 1, 1, 5)
    assert two.fss()[:, 0, 0].tolist() == [0.75, 0.25]
    lead = two.by_lead('model')
    assert lead['fss'].tolist() == [[1.0 - 32.0 / 48.0]] and lead['fss'][0, 0] != two.fss().mean()
    assert lead['n'].tolist() == [40.0] and lead['base_rate'].tolist() == [0.6] and lead['useful'].tolist() == [0.8]


def test_useful_scale_on_a_hand_made_table():
    """Three lead times, scales (1, 5, 9), n = 100 and 20 events each: useful = 0.5 + 0.2 / 2 = 0.6.
        lead 0: fss 0.5, 0.6, 0.9 -> 5 (>= is inclusive: 1 - 40/100 is exactly 0.6)
        lead 1: fss 0.7, 0.4, 0.9 -> 1 (the smallest scale that reaches it, whatever comes after)
        lead 2: fss 0.1, 0.2, 0.5 -> none: NaN"""
    from qtmpnn.fss import FSS
    row = lambda fss: [100, 20, round((1 - fss) * 100), 50, 50]
    table = [[row(0.5), row(0.6), row(0.9)], [row(0.7), row(0.4), row(0.9)], [row(0.1), row(0.2), row(0.5)]]
    s = np.array(table, dtype=np.int64)[None, :, None]                       # (1, 3, 1, 3, 5)
    s = np.concatenate([s, s], axis=2)
    s[:, :, 1, :, 2] = 50                                                   # persistence: fss 0.5 everywhere
    r = FSS(s, ('model', 'persistence'), 0.15, (1, 5, 9))
    lead = r.by_lead('model')
    assert lead['useful'].tolist() == [0.6, 0.6, 0.6]
    assert lead['useful_scale'][:2].tolist() == [5.0, 1.0] and np.isnan(lead['useful_scale'][2])
    np.testing.assert_array_equal(lead['fss'], 1 - np.array([[50, 40, 10], [30, 60, 10], [90, 80, 50]]) / 100)
    np.testing.assert_array_equal(r.skill(), lead['fss'] - 0.5)
    assert r.skill().shape == (3, 3) and (r.skill('model', 'model') == 0).all()
    with pytest.raises(KeyError, match='skill: no source .climatology.'):
        r.skill(reference='climatology')


def test_fss_refuses_by_name():
    from qtmpnn.fss import FSS
    s = np.zeros((2, 3, 2, 4, 5), dtype=np.int64)
    src, sc = ('model', 'persistence'), (1, 3, 5, 9)
    for bad in (s[0], s[..., :4], s[:, :, :1], s[:, :, :, :3], s.reshape(2, 3, 2, 20)):
        with pytest.raises(ValueError, match='FSS: sums of shape'):
            FSS(bad, src, 0.15, sc)
    with pytest.raises(ValueError, match='FSS: sums must be integers'):
        FSS(s.astype(np.float64), src, 0.15, sc)
    with pytest.raises(ValueError, match='FSS: sources'):
        FSS(s, ('model', 'model'), 0.15, sc)
    for bad in ((1, 3, 4, 9), (1, 3, 3, 9), (9, 5, 3, 1), (1, 3, 5, 35)):
        with pytest.raises(ValueError, match='FSS: scales must be'):
            FSS(s, src, 0.15, bad)
    r = FSS(s, src, 0.15, sc)
    assert r.scales == sc and r.threshold == 0.15
    for fn in (r.fss, r.by_lead):
        with pytest.raises(KeyError, match='climatology'):
            fn('climatology')


def test_scales_are_checked_on_the_host_by_name():
    from qtmpnn import ops
    cases = {'must be integers': [(1, 3.0), (1, '3'), (1, None), (True, 3), (1.5,)],
             'must be odd': [(1, 2), (4,), (0,)],
             'must be in 1..33': [(1, 35), (-1, 3), (33, 35)],
             'strictly increasing': [(3, 3), (5, 3), (1, 9, 5)],
             'scales is empty': [(), []],
             'at most 8': [(1, 3, 5, 7, 9, 11, 13, 15, 17)],
             'must be a sequence': [5, None]}
    for why, bads in cases.items():
        for bad in bads:
            with pytest.raises(ValueError, match=f'somewhere: .*{why}'):
                ops.check_scales('somewhere', bad)
    assert ops.check_scales('x', DEFAULT) == DEFAULT and ops.check_scales('x', [33]) == (33,)
    assert ops.check_scales('x', np.array([1, 3])) == (1, 3) and type(ops.check_scales('x', np.array([1, 3]))[0]) is int
    assert ops.check_scales('x', (1, 3, 5, 7, 9, 11, 13, 15)) == (1, 3, 5, 7, 9, 11, 13, 15)
    # before anything else is looked at: no outputs, no meshes, no device
    with pytest.raises(ValueError, match='rollout_fss: scales must be odd'):
        ops.rollout_fss([], [], None, scales=(1, 2))


def test_fss_entry_is_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    name = 'qt_fss_rollout'
    decls = header_decls()
    decl = decls[name]
    assert re.match(r'int\s+qt_fss_rollout\s*\(', decl.text) and decl.times == 1
    assert re.search(r'int\s+m\s*,\s*int\s+nscales\s*,\s*const\s+int\s*\*\s*scales\s*,\s*int32_t\s*\*\s*partial\s*,\s*void\s*\*\s*stream\s*\)',
                     decl.text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names()
    # the arguments up to m are qt_reliability_rollout's (and qt_score_rollout's); then nscales, scales, partial, stream
    rel, fss = _lib._SIGNATURES['qt_reliability_rollout'], _lib._SIGNATURES[name]
    assert fss[:20] == rel[:20] == _lib._SIGNATURES['qt_score_rollout'][:20]
    assert decl.params[:20] == decls['qt_score_rollout'].params[:20]
    assert fss[20:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert len(_lib.exported_names()) == 91 and '(91 entry points)' in readme


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_fss_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))
    ints = lambda *v: (ctypes.c_int * len(v))(*v)

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.5, B=1, n=8, m=8, scales=ints(1, 3, 33), nscales=None, partial=x):
        nscales = (len(scales) if scales is not None else 1) if nscales is None else nscales
        rc = lib.qt_fss_rollout(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm, thr, B,
                                n, m, nscales, scales, partial, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(outs=None), dict(strides=None), dict(labels=None), dict(Ns=None),
           dict(n_devs=None), dict(y=None), dict(partial=None),
           dict(B=0), dict(B=-3), dict(B=65536), dict(n=0), dict(m=0), dict(m=-8),
           dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1), dict(b1=x, b1ss=-1), dict(b2=x, b2cs=-1), dict(b2=x, b2ss=-1),
           dict(scales=None), dict(nscales=0), dict(nscales=-1), dict(nscales=9, scales=ints(1, 3, 5, 7, 9, 11, 13, 15, 17)),
           dict(scales=ints(1, 2)), dict(scales=ints(0,)), dict(scales=ints(-1, 3)), dict(scales=ints(1, 35)),
           dict(scales=ints(3, 3)), dict(scales=ints(5, 3)),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_fss_rollout' in err, (kw, rc, err)
    # the shared refusals carry this entry's name, its own say what is wrong
    assert b'qt_fss_rollout: nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(b2=x, b2ss=-1)[1]
    assert b'bad segment' in call(strides=(ctypes.c_int * 16)())[1]
    assert b'nscales must be 1..8' in call(nscales=0)[1] and b'nscales must be 1..8' in call(nscales=9, scales=ints(*range(1, 19, 2)))[1]
    assert b'odd and in 1..33' in call(scales=ints(1, 2))[1] and b'odd and in 1..33' in call(scales=ints(1, 35))[1]
    assert b'strictly increasing' in call(scales=ints(5, 3))[1] and b'strictly increasing' in call(scales=ints(3, 3))[1]
    assert b'null scales' in call(scales=None)[1]
    assert b'partial' in call(partial=None)[1]
    assert b'bad sizes' in call(B=0)[1]
    # all NULL, as every other entry is refused on a machine without a GPU
    assert lib.qt_fss_rollout(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.5, 1, 8, 8, 3, None,
                              None, None) == -1
    assert b'qt_fss_rollout' in lib.qt_last_error()


def test_fss_is_a_method_beside_score():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    from qtmpnn.fss import FSS
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    fss = inspect.signature(NextFramePredictorS2S.fss).parameters
    assert list(fss) == list(score) + ['scales']
    for name, p in score.items():
        assert fss[name].default == p.default, name
    assert fss['scales'].default == DEFAULT
    graphed = inspect.signature(NextFramePredictorS2S.make_graphed_fss).parameters
    assert list(graphed)[:4] == ['self', 'x', 'y', 'concat_layers'] and list(graphed)[-2:] == ['threshold', 'scales']
    assert graphed['scales'].default == DEFAULT
    assert list(inspect.signature(ops.rollout_fss).parameters) == ['outputs', 'meshes', 'y', 'threshold', 'scales', 'persistence',
                                                                   'climatology', 'per_tile']
    assert inspect.signature(ops.rollout_fss).parameters['scales'].default == DEFAULT
    assert list(inspect.signature(mpnnlstm.fss_product).parameters) == ['threshold', 'scales']
    assert list(inspect.signature(FSS.__init__).parameters) == ['self', 'sums', 'sources', 'threshold', 'scales']
