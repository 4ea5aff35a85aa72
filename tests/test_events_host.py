"""CPU-side checks of the event dates (no GPU): the qt_event_scan / qt_event_sums entries and their argument checks, the numpy
restatement on a case worked out by hand, and qtmpnn.events.EventDates (derived numbers, pooling, error map, refusals)."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from events_restated import first_runs, restated_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_event_entries_are_declared_exported_and_bound():
    from helpers import header_decls
    from qtmpnn import _lib
    decls = header_decls()
    scan, sums = decls['qt_event_scan'], decls['qt_event_sums']
    assert re.match(r'int\s+qt_event_scan\s*\(', scan.text) and re.match(r'int\s+qt_event_sums\s*\(', sums.text)
    assert scan.times == sums.times == 1
    assert re.search(r'int32_t\s*\*\s*dates\s*,\s*int32_t\s*\*\s*runs', scan.text)
    assert re.search(r'int64_t\s*\*\s*sums', sums.text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('qt_event_scan', 'qt_event_sums'):
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names(), name
    # the head of qt_event_scan is qt_score_rollout's with one dense base: (nseg .. y, strides), (base, strides), mask, thr, B, n, m
    score = _lib._SIGNATURES['qt_score_rollout']
    assert _lib._SIGNATURES['qt_event_scan'][:17] == score[:12] + score[15:20]
    score_params = [p.replace('base1', 'base') for p in decls['qt_score_rollout'].params]
    assert scan.params[:17] == score_params[:12] + score_params[15:20]
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_event_scan_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, base=None, bcs=0, bss=0,
             pm=None, thr=0.15, B=1, n=8, m=8, launch=x, lcs=64, target=0, k=1, z0=0, dates=x, runs=x):
        rc = lib.qt_event_scan(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, base, bcs, bss, pm, thr, B, n, m, launch,
                               lcs, target, k, z0, dates, runs, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(outs=None), dict(strides=None), dict(labels=None), dict(Ns=None),
           dict(n_devs=None), dict(y=None), dict(launch=None), dict(dates=None), dict(runs=None),
           dict(B=0), dict(B=-3), dict(n=0), dict(m=0), dict(m=-8),
           dict(ycs=-1), dict(yss=-64), dict(base=x, bcs=-1), dict(base=x, bss=-1), dict(lcs=-1),
           dict(k=0), dict(k=-2), dict(z0=-1), dict(z0=-16), dict(target=2), dict(target=-1),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_event_scan' in err, (kw, rc, err)
    assert b'nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(lcs=-1)[1]
    assert b'k (persist)' in call(k=0)[1]
    assert b'z0' in call(z0=-1)[1]
    assert b'target' in call(target=2)[1]
    assert b'dates' in call(dates=None)[1] and b'runs' in call(runs=None)[1]
    # all NULL, as every other entry is refused on a machine without a GPU
    assert lib.qt_event_scan(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0.15, 1, 8, 8, None, 0, 0, 1, 0,
                             None, None, None) == -1
    assert b'qt_event_scan' in lib.qt_last_error()


def test_event_sums_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()

    def call(dates=x, S1=2, B=1, n=8, m=8, sums=x):
        rc = lib.qt_event_sums(dates, S1, B, n, m, sums, None)
        return rc, lib.qt_last_error()

    for kw in (dict(dates=None), dict(sums=None), dict(S1=1), dict(S1=4), dict(S1=0), dict(S1=-2), dict(B=0), dict(B=-1),
               dict(n=0), dict(m=0), dict(n=-8)):
        rc, err = call(**kw)
        assert rc == -1 and b'qt_event_sums' in err, (kw, rc, err)
    assert b'S1' in call(S1=4)[1]
    assert b'sums' in call(sums=None)[1]
    assert b'bad sizes' in call(B=0)[1]


def test_first_runs_follow_the_definition():
    s = np.array([1, 0, 0, 1, 0, 0, 0, 1, 0], bool).reshape(9, 1, 1)
    assert first_runs(s, False, 1)[0, 0] == 1 and first_runs(s, False, 2)[0, 0] == 1 and first_runs(s, False, 3)[0, 0] == 4
    assert first_runs(s, False, 4)[0, 0] == -1
    assert first_runs(s, True, 1)[0, 0] == 0 and first_runs(s, True, 2)[0, 0] == -1
    # a run that reaches the end of the window: complete with k = 1, cut off with k = 2
    e = np.array([1, 1, 1, 0], bool).reshape(4, 1, 1)
    assert first_runs(e, False, 1)[0, 0] == 3 and first_runs(e, False, 2)[0, 0] == -1
    assert first_runs(e, True, 3)[0, 0] == 0 and first_runs(e, True, 4)[0, 0] == -1


def _hand_case():
    nan = np.nan
    #              (0,0) (0,1) (0,2) (1,0) (1,1) (1,2)
    model = np.array([[.9, .9, .1, .1, .1, .5],
                      [.1, .9, .1, .1, .1, .5],
                      [.9, .9, .1, .1, .9, .9],
                      [.1, .9, .1, .1, nan, .9],
                      [.1, .1, .1, .1, .9, .9]], np.float32).reshape(5, 2, 3)
    obs = np.array([[.9, .1, .1, .1, .1, .9],
                    [.9, .1, .9, .1, .1, .9],
                    [.1, .9, .9, .1, .9, .9],
                    [.1, .9, .1, .1, .9, .9],
                    [.9, .9, .1, .1, .9, .9]], np.float32).reshape(5, 2, 3)
    launch = np.array([[.9, .9, .5], [.9, .9, .9]], np.float32)
    mask = np.array([[False, False, False], [True, False, False]])
    return model, obs, launch, mask


def test_restated_events_on_a_case_worked_out_by_hand():
    """2 x 3, T = 5, threshold 0.5, break-up (target: not ice), k = 2.  Ice states per step (1 = ice), launch first:
      (0, 0)  launch 1 | model 1 0 1 0 0: one open step (a run of k - 1) broken by ice, then open at 3, 4 -> 3
                       | observed 1 1 0 0 1 -> 2: a hit with e = +1
      (0, 1)  launch 1 | model 1 1 1 1 0: the run that starts at 4 would complete past the window -> -1
                       | observed 0 0 1 1 1 -> 0: a miss
      (0, 2)  launch 0.5 == thr: not ice, already open at launch -> -1 for both whatever follows: neither
      (1, 0)  masked -> -2 for both, not counted
      (1, 1)  model 0 0 1 nan 1: the event at 0 was found before the step without a node -> -2 for both, not counted
      (1, 2)  launch 1 | model .5 .5 1 1 1: a value equal to the threshold is not ice -> 0
                       | observed 1 1 1 1 1 -> -1: a false alarm
    sums of the model: n 4, sum e 1, sum |e| 1, sum e^2 1, hits 1, false alarms 1, misses 1, neither 1."""
    model, obs, launch, mask = _hand_case()
    dates, sums = restated_events([{'observed': obs, 'model': model}], [launch], mask, 0.5, 'breakup', 2)
    assert dates.shape == (1, 2, 2, 3) and dates.dtype == np.int32 and sums.shape == (1, 1, 8) and sums.dtype == np.int64
    assert dates[0, 1].tolist() == [[3, -1, -1], [-2, -2, 0]]
    assert dates[0, 0].tolist() == [[2, 0, -1], [-2, -2, -1]]
    assert sums[0, 0].tolist() == [4, 1, 1, 1, 1, 1, 1, 1]
    # k = 1: the single open step counts, and so does the last one
    d1, s1 = restated_events([{'observed': obs, 'model': model}], [launch], mask, 0.5, 'breakup', 1)
    assert d1[0, 1].tolist() == [[1, 4, -1], [-2, -2, 0]] and d1[0, 0].tolist() == [[2, 0, -1], [-2, -2, -1]]
    assert s1[0, 0].tolist() == [4, 3, 5, 17, 2, 1, 0, 1]
    # freeze-up of the same frames: every pixel but (0, 2) is ice at launch already; (0, 2) closes for two steps in the
    # observed frames only (1, 2): a miss
    d2, s2 = restated_events([{'observed': obs, 'model': model}], [launch], mask, 0.5, 'freezeup', 2)
    assert d2[0, 1].tolist() == [[-1, -1, -1], [-2, -2, -1]] and d2[0, 0].tolist() == [[-1, -1, 1], [-2, -2, -1]]
    assert s2[0, 0].tolist() == [4, 0, 0, 0, 0, 0, 1, 3]
    # a third source and a second clip: the rows are per clip and per forecast source
    d3, s3 = restated_events([{'observed': obs, 'model': model, 'climatology': obs}] * 2, [launch] * 2, None, 0.5, 'breakup', 2)
    assert d3.shape == (2, 3, 2, 3) and s3.shape == (2, 2, 8)
    # without the mask (1, 0) is counted: open from step 0 in both -> 0, a hit with e = 0
    assert d3[1, 1].tolist() == [[3, -1, -1], [0, -2, 0]] and np.array_equal(d3[1, 2], d3[1, 0])
    assert s3[1, 1].tolist() == [5, 0, 0, 0, 3, 0, 0, 2] and s3[0, 0].tolist() == [5, 1, 1, 1, 2, 1, 1, 1]


def _hand_events():
    """Two clips, sources observed / model / climatology, 2 x 3 frames; sums consistent with the dates."""
    dates = np.array([[[[2, 0, -1], [-2, 5, -1]], [[3, -1, -1], [-2, 1, 0]], [[2, 0, 4], [-2, -1, -1]]],
                      [[[1, -1, -1], [-2, -2, -1]], [[4, 2, -1], [-2, -2, -1]], [[-1, -1, -1], [-2, -2, -1]]]], np.int32)
    sums = np.array([[[5, -3, 5, 17, 2, 1, 1, 1], [5, 0, 0, 0, 2, 1, 1, 1]],
                     [[4, 3, 3, 9, 1, 1, 0, 2], [4, 0, 0, 0, 0, 0, 1, 3]]], np.int64)
    return dates, sums


def test_hand_events_are_what_the_restatement_counts():
    """The sums of _hand_events() recomputed from its dates by the definition's slot rules."""
    dates, sums = _hand_events()
    for c in range(2):
        o = dates[c, 0].astype(np.int64)
        for s in (1, 2):
            f = dates[c, s].astype(np.int64)
            cnt, both = o != -2, (o >= 0) & (f >= 0)
            e = (f - o)[both]
            want = [cnt.sum(), e.sum(), np.abs(e).sum(), (e * e).sum(), both.sum(), (cnt & (o < 0) & (f >= 0)).sum(),
                    (cnt & (o >= 0) & (f < 0)).sum(), (cnt & (o < 0) & (f < 0)).sum()]
            assert sums[c, s - 1].tolist() == want, (c, s)


def test_derive_on_hand_sums():
    from qtmpnn.events import METRICS, SLOTS, derive
    assert SLOTS == ('n', 'sum_e', 'sum_abs_e', 'sum_sq_e', 'hits', 'false_alarms', 'misses', 'neither')
    d = derive(np.array([10, -6, 10, 36, 4, 1, 3, 2], np.int64))
    assert set(d) == set(METRICS)
    assert d['n'] == 10 and d['bias'] == -1.5 and d['mae'] == 2.5 and d['rmse'] == 3.0
    assert d['hit_rate'] == 4 / 7 and d['false_alarm_ratio'] == 0.2
    assert d['hits'] == 4 and d['false_alarms'] == 1 and d['misses'] == 3
    # zero denominators: NaN, no warning; counts stay
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        z = derive(np.array([[7, 0, 0, 0, 0, 0, 0, 7], [7, 0, 0, 0, 0, 2, 0, 5], [7, 0, 0, 0, 0, 0, 3, 4]]))
    assert np.isnan(z['bias']).all() and np.isnan(z['mae']).all() and np.isnan(z['rmse']).all()
    assert np.isnan(z['hit_rate'][:2]).all() and z['hit_rate'][2] == 0
    assert np.isnan(z['false_alarm_ratio'][[0, 2]]).all() and z['false_alarm_ratio'][1] == 1
    assert z['n'].tolist() == [7, 7, 7] and z['misses'].tolist() == [0, 0, 3]
    with pytest.raises(ValueError, match='derive: sums of shape'):
        derive(np.zeros((3, 7)))


def test_event_dates_metrics_pooled_and_date():
    from qtmpnn.events import METRICS, EventDates, derive
    dates, sums = _hand_events()
    ev = EventDates(dates, sums, ('observed', 'model', 'climatology'), 'breakup', 2, 0.15)
    assert ev.dates.dtype == np.int32 and ev.sums.dtype == np.int64 and ev.dates.shape == (2, 3, 2, 3)
    assert (ev.kind, ev.persist, ev.threshold) == ('breakup', 2, 0.15)
    for s, name in enumerate(ev.sources):
        np.testing.assert_array_equal(ev.date(name), dates[:, s])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for s, name in ((0, 'model'), (1, 'climatology')):
            per_clip, pooled = ev.metrics(name), ev.pooled(name)
            want, want_pooled = derive(sums[:, s]), derive(sums[:, s].sum(axis=0))
            for k in METRICS:
                assert per_clip[k].shape == (2,) and pooled[k].shape == ()
                np.testing.assert_array_equal(per_clip[k], want[k], err_msg=f'{name} {k}')
                np.testing.assert_array_equal(pooled[k], want_pooled[k], err_msg=f'{name} {k}')
                np.testing.assert_array_equal(getattr(ev, k)(name), want[k])
    m = ev.metrics()
    assert m['bias'].tolist() == [-1.5, 3.0] and m['rmse'][1] == 3.0 and m['hit_rate'].tolist() == [2 / 3, 1.0]
    p = ev.pooled()
    assert p['n'] == 9 and p['hits'] == 3 and p['bias'] == 0.0 and p['mae'] == 8 / 3 and p['rmse'] == np.sqrt(26 / 3)
    assert p['hit_rate'] == 0.75 and p['false_alarm_ratio'] == 0.4
    # pooling is of sums, not a mean of the clips' ratios
    assert p['mae'] != m['mae'].mean()
    c = ev.metrics('climatology')
    assert np.isnan(c['bias'][1]) and c['hit_rate'][1] == 0 and np.isnan(c['false_alarm_ratio'][1])


def test_event_dates_error_map():
    from qtmpnn.events import EventDates
    dates, sums = _hand_events()
    ev = EventDates(dates, sums, ('observed', 'model', 'climatology'), 'breakup', 2, 0.15)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        em, ec = ev.error_map('model'), ev.error_map('climatology')
    assert em.shape == ec.shape == (2, 3) and em.dtype == np.float64
    # (0, 0): e = +1 and +3 -> 2; (1, 1): -4 in clip 0 only; elsewhere no clip has both
    assert em[0, 0] == 2.0 and em[1, 1] == -4.0 and np.isnan(em[[0, 0, 1, 1], [1, 2, 0, 2]]).all()
    assert ec[0, 0] == 0.0 and ec[0, 1] == 0.0 and np.isnan(ec[[0, 1, 1, 1], [2, 0, 1, 2]]).all()


def test_event_dates_refuse_by_name():
    from qtmpnn.events import EventDates
    dates, sums = _hand_events()
    src = ('observed', 'model', 'climatology')
    for bad in (dates[:, :2], dates[0], dates.astype(np.float32), dates.reshape(2, 3, 6)):
        with pytest.raises(ValueError, match='EventDates: dates of shape'):
            EventDates(bad, sums, src, 'breakup', 2, 0.15)
    for bad in (sums[:1], sums[:, :1], sums[..., :7], sums.astype(np.float64)):
        with pytest.raises(ValueError, match='EventDates: sums of shape'):
            EventDates(dates, bad, src, 'breakup', 2, 0.15)
    with pytest.raises(ValueError, match='EventDates: sources'):
        EventDates(dates, sums, ('model', 'observed', 'climatology'), 'breakup', 2, 0.15)
    with pytest.raises(ValueError, match='EventDates: kind must be one of'):
        EventDates(dates, sums, src, 'melt', 2, 0.15)
    with pytest.raises(ValueError, match='EventDates: persist must be'):
        EventDates(dates, sums, src, 'breakup', 0, 0.15)
    ev = EventDates(dates[:, :2], sums[:, :1], src[:2], 'freezeup', 1, 0.5)
    with pytest.raises(KeyError, match='climatology'):
        ev.metrics('climatology')
    with pytest.raises(KeyError, match='climatology'):
        ev.date('climatology')
    for fn in (ev.metrics, ev.pooled, ev.error_map):
        with pytest.raises(KeyError, match='observed'):
            fn('observed')
    assert ev.date('observed').shape == (2, 2, 3)


def test_event_dates_is_a_method_beside_score():
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    from qtmpnn.events import EventDates
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    events = inspect.signature(NextFramePredictorS2S.event_dates).parameters
    assert list(events) == list(score) + ['kind', 'persist']
    for name, p in score.items():
        assert events[name].default == p.default, name
    assert events['kind'].default == 'breakup' and events['persist'].default == 5
    graphed = inspect.signature(NextFramePredictorS2S.make_graphed_events).parameters
    assert list(graphed)[:4] == ['self', 'x', 'y', 'concat_layers'] and list(graphed)[-3:] == ['threshold', 'kind', 'persist']
    assert list(inspect.signature(ops.rollout_event_dates).parameters) == ['outputs', 'meshes', 'y', 'launch', 'threshold', 'kind',
                                                                           'persist', 'climatology']
    assert list(inspect.signature(EventDates.__init__).parameters) == ['self', 'dates', 'sums', 'sources', 'kind', 'persist',
                                                                       'threshold']
