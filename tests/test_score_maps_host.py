"""CPU-side checks of the per-pixel verification maps (no GPU): the qt_score_maps entry and its argument checks, the
restatement on a case worked out by hand, and qtmpnn.score.ScoreMaps (derived maps, pooling with a region and with cell areas)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from score_maps_restated import restated_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_maps_entry_is_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    decls = header_decls()
    decl = decls['qt_score_maps']
    assert re.match(r'int\s+qt_score_maps\s*\(', decl.text) and decl.times == 1
    assert re.search(r'double\s*\*\s*maps\s*,\s*int64_t\s+maps_step_stride', decl.text)
    assert decl.params[:20] == decls['qt_score_rollout'].params[:20]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'qt_score_maps')
    assert 'qt_score_maps' in _lib._SIGNATURES and 'qt_score_maps' in _lib.exported_names()
    # qt_score_rollout's arguments with (double* maps, int64 stride) in place of (float* partial)
    assert _lib._SIGNATURES['qt_score_maps'] == _lib._SIGNATURES['qt_score_rollout'][:-2] + [ctypes.c_void_p, ctypes.c_int64,
                                                                                             ctypes.c_void_p]
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_score_maps_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.15, B=1, n=8, m=8, maps=x, mss=3 * 8 * 64):
        rc = lib.qt_score_maps(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm, thr,
                               B, n, m, maps, mss, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(maps=None), dict(outs=None), dict(labels=None), dict(y=None),
           dict(strides=None), dict(Ns=None), dict(n_devs=None), dict(B=0), dict(B=-3), dict(n=0), dict(m=0),
           dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1), dict(b2=x, b2ss=-1),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)()),
           # the step stride must hold S * 8 * P doubles: S = 1, 2, 3 with P = 64
           dict(mss=8 * 64 - 1), dict(mss=0), dict(mss=-8 * 64), dict(b1=x, mss=2 * 8 * 64 - 1),
           dict(b1=x, b2=x, mss=3 * 8 * 64 - 1), dict(b2=x, mss=8 * 64)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_score_maps' in err, (kw, rc, err)
    assert b'maps_step_stride' in call(mss=8 * 64 - 1)[1]
    assert b'nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(ycs=-1)[1]
    # all NULL, as every other entry is refused on a machine without a GPU
    assert lib.qt_score_maps(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.15, 1, 8, 8, None, 0,
                             None) == -1
    assert b'qt_score_maps' in lib.qt_last_error()


def test_restated_maps_on_a_case_worked_out_by_hand():
    """2 x 2, threshold 0.5, one step, two clips; pixel (1, 1) is masked, pixel (0, 1) has no node in clip 1 (NaN frame).
    clip 0: model [[.75, .25], [1, 9]], truth [[.5, .75], [1, 0]] -> d [0.25, -0.5, 0], classes over, under, hit
    clip 1: model [[0, nan], [.5, 9]],  truth [[0, 1],   [1, 0]]  -> d [0, -, -0.5],    classes correct negative, -, under"""
    nan = np.nan
    f = [{'model': np.array([[[.75, .25], [1, 9]]], np.float32)}, {'model': np.array([[[0, nan], [.5, 9]]], np.float32)}]
    t = [np.array([[[.5, .75], [1, 0]]], np.float32), np.array([[[0, 1], [1, 0]]], np.float32)]
    mask = np.array([[False, False], [False, True]])
    m = restated_maps(f, t, mask, 0.5)
    assert m.shape == (1, 1, 8, 2, 2) and m.dtype == np.float64
    got = {(i, j): m[0, 0, :, i, j].tolist() for i in range(2) for j in range(2)}
    assert got[0, 0] == [2, 0.25, 0.25, 0.0625, 0, 1, 0, 1]
    assert got[0, 1] == [1, -0.5, 0.5, 0.25, 0, 0, 1, 0]
    assert got[1, 0] == [2, -0.5, 0.5, 0.25, 1, 0, 1, 0]
    assert got[1, 1] == [0] * 8


def test_restated_maps_form_d_in_fp32():
    """0.1f - 1e-9f is 0.1f in fp32 (the difference is rounded once, as on the device), not the float64 difference."""
    f = [{'model': np.full((1, 1, 1), 0.1, np.float32)}]
    t = [np.full((1, 1, 1), 1e-9, np.float32)]
    m = restated_maps(f, t, None, 0.5)
    d32 = np.float32(0.1) - np.float32(1e-9)
    assert m[0, 0, 1, 0, 0] == float(d32) != float(np.float32(0.1)) - float(np.float32(1e-9))
    assert m[0, 0, 3, 0, 0] == float(d32) * float(d32)


def _hand_maps():
    """(T = 2, S = 2, 8, 2, 3): pixel (1, 2) is never counted; the persistence source is the model's steps swapped."""
    s = np.zeros((2, 2, 8, 2, 3))
    px = {(0, 0): [[4, 2, 6, 10, 1, 1, 1, 1], [4, -1, 1, .5, 0, 0, 2, 2]],
          (0, 1): [[4, 0, 0, 0, 2, 0, 0, 2], [4, 2, 2, 1, 1, 2, 1, 0]],
          (0, 2): [[3, 1, 1, 1, 1, 1, 1, 0], [3, 0, 3, 3, 0, 3, 0, 0]],
          (1, 0): [[4, -2, 2, 4, 0, 0, 4, 0], [4, 4, 4, 16, 0, 4, 0, 0]],
          (1, 1): [[1, .5, .5, .25, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1]]}
    for (i, j), v in px.items():
        s[:, 0, :, i, j] = v
    s[:, 1] = s[::-1, 0]
    return s


def test_score_maps_metrics_equal_derive_by_hand():
    from qtmpnn.score import METRICS, ScoreMaps, derive
    sums = _hand_maps()
    sm = ScoreMaps(sums, ('model', 'persistence'))
    assert sm.sums.dtype == np.float64 and sm.sums.shape == (2, 2, 8, 2, 3) and sm.sources == ('model', 'persistence')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for s, name in enumerate(sm.sources):
            got = sm.metrics(name)
            assert set(got) == set(METRICS)
            for i in range(2):
                for j in range(3):
                    want = derive(sums[:, s, :, i, j])                      # (T, 8) of this pixel
                    for k in METRICS:
                        assert got[k].shape == (2, 2, 3)
                        np.testing.assert_array_equal(got[k][:, i, j], want[k], err_msg=f'{name} {k} ({i}, {j})')
                        np.testing.assert_array_equal(getattr(sm, k)(name)[:, i, j], want[k])
    m = sm.metrics()
    assert m['bias'][0, 0, 0] == 0.5 and m['rmse'][0, 0, 0] == np.sqrt(2.5) and m['accuracy'][0, 0, 0] == 0.5
    assert m['iiee'][1, 0, 2] == 3 and sm.over('persistence')[0, 0, 2] == 3
    # the pixel no clip counts: n == 0, counts 0, ratios NaN
    for k in ('bias', 'mae', 'rmse', 'accuracy'):
        assert np.isnan(m[k][:, 1, 2]).all() and not np.isnan(m[k][:, :, :2]).any()
    assert (m['n'][:, 1, 2] == 0).all() and (m['iiee'][:, 1, 2] == 0).all()
    with pytest.raises(KeyError, match='climatology'):
        sm.metrics('climatology')


def test_score_maps_pooled_is_the_sum_over_pixels():
    from qtmpnn.score import ScoreMaps, derive
    sums = _hand_maps()
    sm = ScoreMaps(sums, ('model', 'persistence'))
    for s, name in enumerate(sm.sources):
        want = derive(sums[:, s].sum(axis=(-2, -1)))
        got = sm.pooled(name)
        for k, v in got.items():
            assert v.shape == (2,)
            np.testing.assert_array_equal(v, want[k], err_msg=f'{name} {k}')
    lead = sm.pooled()
    assert lead['n'].tolist() == [16, 16] and lead['over'].tolist() == [3, 9] and lead['rmse'][0] == np.sqrt(15.25 / 16)
    # weights of ones change nothing
    for k, v in sm.pooled(weights=np.ones((2, 3))).items():
        np.testing.assert_array_equal(v, lead[k])


def test_score_maps_pooled_over_a_region_pools_its_pixels_only():
    from qtmpnn.score import ScoreMaps, derive
    sums = _hand_maps()
    sm = ScoreMaps(sums, ('model', 'persistence'))
    region = np.array([[True, False, True], [False, True, True]])
    for s, name in enumerate(sm.sources):
        want = derive(sums[:, s][:, :, region].sum(axis=-1))
        for weights in (region, region.astype(np.float64), region.astype(np.uint8)):
            got = sm.pooled(name, weights=weights)
            for k in want:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f'{name} {k}')
    assert sm.pooled(weights=region)['n'].tolist() == [8, 8]
    # a region without a counted pixel: NaN ratios, no warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        empty = sm.pooled(weights=np.array([[0, 0, 0], [0, 0, 1]]))
    assert np.isnan(empty['rmse']).all() and (empty['n'] == 0).all()


def test_score_maps_pooled_with_cell_areas_gives_areas():
    from qtmpnn.score import ScoreMaps
    sums = _hand_maps()
    sm = ScoreMaps(sums, ('model', 'persistence'))
    area = np.array([[1.0, 0.5, 0.25], [2.0, 4.0, 8.0]])                     # binary fractions: every product is exact
    got = sm.pooled('model', weights=area)
    over, under, n, sq = (sums[:, 0, k] for k in (5, 6, 0, 3))
    np.testing.assert_array_equal(got['iiee'], (area * (over + under)).sum(axis=(-2, -1)))
    np.testing.assert_array_equal(got['over'], (area * over).sum(axis=(-2, -1)))
    np.testing.assert_array_equal(got['n'], (area * n).sum(axis=(-2, -1)))
    np.testing.assert_array_equal(got['rmse'], np.sqrt((area * sq).sum(axis=(-2, -1)) / (area * n).sum(axis=(-2, -1))))
    assert got['iiee'].tolist() == [1 * 2 + 0.25 * 2 + 2 * 4 + 4 * 1, 1 * 2 + 0.5 * 3 + 0.25 * 3 + 2 * 4]
    # areas times a region
    region = np.array([[1, 1, 0], [0, 0, 0]])
    assert sm.pooled(weights=area * region)['iiee'].tolist() == [2.0, 3.5]


def test_score_maps_refuse_wrong_shapes_by_name():
    from qtmpnn.score import ScoreMaps
    for shape in ((2, 2, 8, 6), (2, 1, 8, 2, 3), (2, 2, 7, 2, 3), (2, 8, 2, 2, 3), (1, 2, 2, 8, 2, 3)):
        with pytest.raises(ValueError, match='ScoreMaps: sums of shape'):
            ScoreMaps(np.zeros(shape), ('model', 'persistence'))
    sm = ScoreMaps(_hand_maps(), ('model', 'persistence'))
    for w in (np.ones((3, 2)), np.ones(6), np.ones((1, 2, 3)), 2.0):
        with pytest.raises(ValueError, match='ScoreMaps.pooled: weights of shape'):
            sm.pooled(weights=w)


def test_scores_carry_maps_only_when_given():
    from qtmpnn.score import ScoreMaps, Scores
    sc = Scores(np.zeros((1, 2, 2, 8)), ('model', 'persistence'))
    assert sc.maps is None
    sm = ScoreMaps(_hand_maps(), ('model', 'persistence'))
    assert Scores(np.zeros((1, 2, 2, 8)), ('model', 'persistence'), maps=sm).maps is sm
    assert list(inspect.signature(Scores.__init__).parameters) == ['self', 'sums', 'sources', 'maps']


def test_score_maps_is_a_method_beside_score():
    """score() keeps its signature (tests/test_score_host.py pins it); the maps come from score_maps(), which takes the same
    arguments, and make_graphed_scores takes the buffer."""
    from model.mpnnlstm import NextFramePredictorS2S
    assert (list(inspect.signature(NextFramePredictorS2S.score_maps).parameters)
            == list(inspect.signature(NextFramePredictorS2S.score).parameters))
    for name, p in inspect.signature(NextFramePredictorS2S.score).parameters.items():
        assert inspect.signature(NextFramePredictorS2S.score_maps).parameters[name].default == p.default, name
    assert inspect.signature(NextFramePredictorS2S.make_graphed_scores).parameters['maps'].default is None
    from qtmpnn import ops
    assert list(inspect.signature(ops.rollout_score_maps).parameters) == ['outputs', 'meshes', 'y', 'maps', 'threshold',
                                                                          'persistence', 'climatology']
