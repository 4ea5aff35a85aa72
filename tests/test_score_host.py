"""CPU-side checks of forecast verification (no GPU): the score() switch, the qt_score_rollout entry and its argument checks,
the restatement on a case worked out by hand, and qtmpnn.score.Scores against the restatement."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np

from score_restated import restated_metrics, restated_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_signature():
    from model.mpnnlstm import NextFramePredictor, NextFramePredictorS2S
    sig = inspect.signature(NextFramePredictorS2S.score)
    assert list(sig.parameters)[1:] == ['loader', 'climatology', 'mask', 'high_interest_region', 'graph_structure', 'use_graph',
                                        'threshold']
    assert sig.parameters['use_graph'].default is False
    assert sig.parameters['threshold'].default == 0.15
    assert callable(NextFramePredictorS2S.make_graphed_scores)
    # the abstract facade is the reference's, unchanged
    assert list(inspect.signature(NextFramePredictor.score).parameters) == ['self', 'x', 'y', 'rollout']
    assert NextFramePredictor.__abstractmethods__ == {'train', 'predict', 'score'}


def test_score_entry_is_declared_exported_and_bound():
    from helpers import HEADER, header_decls
    from qtmpnn import _lib
    decl = header_decls()['qt_score_rollout']
    assert re.match(r'int\s+qt_score_rollout\s*\(', decl.text) and decl.times == 1
    header = open(HEADER).read()
    for slot in ('hits', 'over', 'under', 'correct negatives'):         # the header comment states the slot table
        assert slot in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'qt_score_rollout')
    assert 'qt_score_rollout' in _lib._SIGNATURES and 'qt_score_rollout' in _lib.exported_names()
    assert lib.qt_abi_version() == 1


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_score_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 16)(*([1] * 16))
    ptrs = (ctypes.c_void_p * 16)(*([x] * 16))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.15, B=1, n=8, m=8, partial=x):
        rc = lib.qt_score_rollout(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm, thr,
                                  B, n, m, partial, None)
        return rc, lib.qt_last_error()

    bad = [dict(outs=None), dict(labels=None), dict(y=None), dict(partial=None), dict(strides=None), dict(Ns=None),
           dict(nseg=17), dict(nseg=0), dict(B=0), dict(B=-3), dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1),
           dict(b2=x, b2ss=-1), dict(n=0), dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_score_rollout' in err, (kw, rc, err)
    # all NULL, as every other entry is refused on a machine without a GPU
    assert lib.qt_score_rollout(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.15, 1, 8, 8, None,
                                None) == -1
    assert b'qt_score_rollout' in lib.qt_last_error()


def test_restatement_on_a_case_worked_out_by_hand():
    """4 x 4, threshold 0.5, the last column masked (12 counted pixels); every value is a binary fraction, so the sums are exact.
    d = field - truth per counted pixel:   0  .5   0 |  .25  0  -.5 |  .25  0  -.25 |  0  1  -.25
    field > .5:                            F   F   T |   F   T   F  |   T   T   T   |  F  T   F      (0.5 > 0.5 is False)
    truth > .5:                            F   F   T |   F   T   T  |   F   T   T   |  F  F   F
    -> sum d = 1, sum |d| = 3, sum d^2 = 4 * .0625 + 2 * .25 + 1 = 1.75; hits 4, over 2, under 1, correct negatives 5."""
    nan = np.nan
    truth = np.array([[0, 0, 1, 7], [0, 1, 1, nan], [.5, .75, 1, 0], [0, 0, .25, 1]], np.float32)[None]
    field = np.array([[0, .5, 1, nan], [.25, 1, .5, 9], [.75, .75, .75, 1], [0, 1, 0, 0]], np.float32)[None]
    mask = np.zeros((4, 4), bool)
    mask[:, 3] = True
    sums, absterms = restated_sums(field, truth, mask, 0.5)
    assert sums.shape == (1, 8) and sums[0].tolist() == [12, 1.0, 3.0, 1.75, 4, 2, 1, 5]
    assert absterms[0].tolist() == [3.0, 3.0, 1.75]
    m = restated_metrics(sums)
    assert m['bias'][0] == 1 / 12 and m['mae'][0] == 0.25 and m['rmse'][0] == (1.75 / 12) ** 0.5
    assert m['accuracy'][0] == 0.75 and m['over'][0] == 2 and m['under'][0] == 1 and m['iiee'][0] == 3 and m['n'][0] == 12
    # without the mask the NaNs of the last column propagate, as in numpy
    assert np.isnan(restated_sums(field, truth, None, 0.5)[0][0, 1:4]).all()


def _hand_sums():
    """(3 clips, 2 steps, 2 sources, 8): clip 0 / 1 differ in n by 9x; clip 2, step 1 counts no pixel."""
    s = np.zeros((3, 2, 2, 8))
    s[0, :, 0] = [[10, 2, 6, 10, 3, 1, 2, 4], [10, -5, 5, 2.5, 0, 0, 5, 5]]
    s[1, :, 0] = [[90, 0, 0, 0, 40, 0, 0, 50], [90, 9, 18, 360, 30, 20, 10, 30]]
    s[2, :, 0] = [[4, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0]]
    s[:, :, 1] = s[:, :, 0][:, ::-1]
    return s


def test_scores_derived_metrics_equal_the_restatement():
    from qtmpnn.score import METRICS, Scores
    sums = _hand_sums()
    sc = Scores(sums, ('model', 'persistence'))
    assert sc.sums.dtype == np.float64 and sc.sums.shape == (3, 2, 2, 8) and sc.sources == ('model', 'persistence')
    for s, name in enumerate(sc.sources):
        want = restated_metrics(sums[:, :, s])
        got = sc.metrics(name)
        assert set(got) == set(METRICS) == set(want)
        for k in METRICS:
            assert got[k].shape == (3, 2)
            np.testing.assert_array_equal(got[k], want[k], err_msg=f'{name} {k}')
            np.testing.assert_array_equal(getattr(sc, k)(name), want[k])
    assert sc.rmse()[0, 0] == 1.0 and sc.accuracy()[0, 0] == 0.7 and sc.iiee()[1, 1] == 30


def test_scores_by_lead_pools_the_sums():
    from qtmpnn.score import Scores
    sums = _hand_sums()[:2]
    sc = Scores(sums, ('model', 'persistence'))
    lead = sc.by_lead('model')
    # step 0: rmse 1 over 10 pixels and 0 over 90 -> sqrt(10 / 100), not the mean 0.5 of the two
    assert lead['rmse'][0] == np.sqrt(10 / 100) and np.mean(sc.rmse()[:, 0]) == 0.5
    want = restated_metrics(sums[:, :, 0].sum(axis=0))
    for k, v in lead.items():
        assert v.shape == (2,)
        np.testing.assert_array_equal(v, want[k], err_msg=k)
    assert lead['n'].tolist() == [100, 100] and lead['over'].tolist() == [1, 20]


def test_scores_without_counted_pixels_give_nan_not_an_error():
    from qtmpnn.score import Scores
    sc = Scores(_hand_sums(), ('model', 'persistence'))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = sc.metrics('model')
        empty = Scores(np.zeros((1, 2, 1, 8)), ('model',)).by_lead()
    for k in ('bias', 'mae', 'rmse', 'accuracy'):
        assert np.isnan(m[k][2, 1]) and not np.isnan(m[k][2, 0])
        assert np.isnan(empty[k]).all()
    assert m['n'][2, 1] == 0 and m['iiee'][2, 1] == 0
    try:
        sc.metrics('climatology')
    except KeyError as e:
        assert 'climatology' in str(e)
    else:
        raise AssertionError('an absent source must be refused by name')
