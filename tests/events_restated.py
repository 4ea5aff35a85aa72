"""Break-up / freeze-up dates restated in numpy from dense frames, written from the definition: the checker of qt_event_scan,
qt_event_sums, ops.rollout_event_dates, NextFramePredictorS2S.event_dates() and qtmpnn.events.EventDates (tests only).

Per source every candidate step is tested for a full run of the target state, over all pixels at once.  Comparisons are strict >
on the fp32 values with the threshold rounded to fp32 once: that is what decides a state.  Everything else is integer, so a
device that follows the definition gives the same numbers exactly."""
import numpy as np

KINDS = {'breakup': False, 'freezeup': True}           # the target state g: no ice / ice


def first_runs(states, g, k):
    """states (T, W, H) bool -> (W, H) int32: per pixel the smallest z with states[z] == ... == states[z + k - 1] == g, all
    inside the sequence (z <= T - k: a run cut off by the end does not count); -1 where there is none."""
    T = len(states)
    date = np.full(states.shape[1:], -1, dtype=np.int32)
    for z in range(T - k, -1, -1):                     # downwards, so that the smallest z is the one that stays
        date[(states[z:z + k] == g).all(axis=0)] = z
    return date


def restated_events(fields, launches, mask, thr, kind, k):
    """fields: per clip {source: (T, W, H) float32} with 'observed' first, then 'model' (NaN where a pixel has no node) and any
    further forecast source; launches: per clip (W, H) float32, the launch frame; mask (W, H) bool, True = not counted, or None.
    -> (dates (n_clips, S1, W, H) int32, sums (n_clips, S1 - 1, 8) int64).  Dates: >= 0 the event's step, -1 no event, -2 not
    counted (masked, or the model's frame is NaN at any step).  sums per forecast source over the counted pixels: [n, sum e,
    sum |e|, sum e^2, both have an event, forecast only, observed only, neither], e = date - observed date."""
    g = KINDS[kind]
    names = list(fields[0])
    assert names[:2] == ['observed', 'model'] and k >= 1
    T, W, H = fields[0]['observed'].shape
    t32 = np.float32(thr)
    keep = np.ones((W, H), dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    dates = np.zeros((len(fields), len(names), W, H), dtype=np.int32)
    sums = np.zeros((len(fields), len(names) - 1, 8), dtype=np.int64)
    for c, (f_clip, launch) in enumerate(zip(fields, launches)):
        launch = np.asarray(launch)
        assert list(f_clip) == names and launch.dtype == np.float32 and launch.shape == (W, H)
        for name in names:
            assert f_clip[name].dtype == np.float32 and f_clip[name].shape == (T, W, H), name
        counted = keep & ~np.isnan(f_clip['model']).any(axis=0)
        with np.errstate(invalid='ignore'):
            ice = {name: f_clip[name] > t32 for name in names}
            a0 = launch > t32
        for s, name in enumerate(names):
            d = first_runs(ice[name], g, k)
            d[a0 == g] = -1                            # already in the target state at launch: no event
            d[~counted] = -2
            dates[c, s] = d
        obs = dates[c, 0].astype(np.int64)
        for s in range(1, len(names)):
            fc = dates[c, s].astype(np.int64)
            both, e = counted & (obs >= 0) & (fc >= 0), fc - obs
            sums[c, s - 1] = [counted.sum(), e[both].sum(), np.abs(e[both]).sum(), (e[both] ** 2).sum(), both.sum(),
                              (counted & (obs < 0) & (fc >= 0)).sum(), (counted & (obs >= 0) & (fc < 0)).sum(),
                              (counted & (obs < 0) & (fc < 0)).sum()]
    return dates, sums
