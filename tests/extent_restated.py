"""Regional ice extent, ice area and over- / under-forecast areas restated in numpy from dense frames, written from the slot
table of qt_extent_rollout in include/qtmpnn.h.  The checker of qt_extent_rollout, ops.rollout_extent and NextFramePredictorS2S.extent()
(tests only; no code shared with qtmpnn).

What decides an integer or an indicator is done as the device does it: ice on the fp32 value with the threshold rounded to fp32
once (strict >, so a NaN is not ice).  The float sums are float64 sums of terms formed in float64 from the fp32 values and the
fp32 areas."""
import numpy as np


def restated_extent(fields, truth, counted, regions, areas, thr, R):
    """fields: S arrays (T, W, H) float32; truth (T, W, H) float32; counted (W, H) or (T, W, H) bool, True = the pixel counts;
    regions (W, H) integers (0 <= r < R: region r, anything else: none) or None (all in region 0); areas (W, H) or None (1)
    -> (sums (T, R, 1 + S, 4), absterms (T, R, 1 + S, 4)): per lead time and region
        row 0      [n, A = sum a, E_o = sum a I_o, SIA_o = sum a y]
        row 1 + s  [E_s = sum a I_s, SIA_s = sum a f_s, O_s = sum a I_s (1 - I_o), U_s = sum a (1 - I_s) I_o]
    and the sum of |term| of every slot (what a rounding-error bound scales with; n itself for the count)."""
    truth = np.asarray(truth)
    fields = [np.asarray(f) for f in fields]
    assert truth.dtype == np.float32 and truth.ndim == 3 and all(f.dtype == np.float32 and f.shape == truth.shape for f in fields)
    T, shape, S = len(truth), truth.shape[1:], len(fields)
    counted = np.broadcast_to(np.asarray(counted, dtype=bool), truth.shape)
    reg = np.zeros(shape, dtype=np.int64) if regions is None else np.asarray(regions).astype(np.int64)
    a = np.ones(shape) if areas is None else np.asarray(areas).astype(np.float32).astype(np.float64)
    assert reg.shape == shape and a.shape == shape
    t32 = np.float32(thr)
    sums, absterms = np.zeros((T, R, 1 + S, 4)), np.zeros((T, R, 1 + S, 4))
    for t in range(T):
        for r in range(R):
            sel = counted[t] & (reg == r)
            w, y = a[sel], truth[t][sel]
            with np.errstate(invalid='ignore'):
                io = y > t32
            rows = [[float(sel.sum()), w.sum(), w[io].sum(), (w * y.astype(np.float64)).sum()]]
            mags = [[float(sel.sum()), np.abs(w).sum(), np.abs(w[io]).sum(), np.abs(w * y.astype(np.float64)).sum()]]
            for f in fields:
                v = f[t][sel]
                with np.errstate(invalid='ignore'):
                    i_s = v > t32
                terms = [w[i_s], w * v.astype(np.float64), w[i_s & ~io], w[~i_s & io]]
                rows.append([x.sum() for x in terms])
                mags.append([np.abs(x).sum() for x in terms])
            sums[t, r], absterms[t, r] = rows, mags
    return sums, absterms
