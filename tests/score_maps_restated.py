"""Per-pixel verification sums restated in numpy, written from the definitions: the checker of qt_score_maps,
ops.rollout_score_maps and the `.maps` of NextFramePredictorS2S.score_maps() (tests only).

The clips are taken one by one in loader order and every pixel's eight float64 sums get `sums += term`, so each sum is the
left-to-right float64 sum over the clips.  d = field - truth is formed in fp32 (the d that score() sees) and then widened, so
|d| and d * d are exact in float64 and the only roundings are those of the sequential adds: a device that adds the same terms
in the same order gives the same bits.  Comparisons are strict > on the fp32 values with the threshold rounded to fp32 once."""
import numpy as np


def restated_maps(fields, truths, mask, thr):
    """fields: per clip {source: (T, W, H) float32}, the model's frames first (NaN where a pixel has no node); truths: per clip
    (T, W, H) float32; mask (W, H) bool, True = not counted, or None.  -> (T, S, 8, W, H) float64 in qtmpnn.score.SLOTS order.
    A pixel of a clip and step is counted iff the model's frame is not NaN there and the pixel is not masked (the counting rule
    of score_restated.restated_sums fed predict()'s frames)."""
    names = list(fields[0])
    T, W, H = truths[0].shape
    keep = np.ones((W, H), dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    t32 = np.float32(thr)
    sums = np.zeros((T, len(names), 8, W, H), dtype=np.float64)
    for f_clip, truth in zip(fields, truths):
        truth = np.asarray(truth)
        assert list(f_clip) == names and truth.dtype == np.float32 and truth.shape == (T, W, H)
        counted = keep[None] & ~np.isnan(np.asarray(f_clip[names[0]]))          # (T, W, H)
        yi = truth > t32
        for s, name in enumerate(names):
            f = np.asarray(f_clip[name])
            assert f.dtype == np.float32 and f.shape == (T, W, H)
            with np.errstate(invalid='ignore'):
                d32 = f - truth
                fi = f > t32
            assert d32.dtype == np.float32
            d = np.where(counted, d32.astype(np.float64), 0.0)
            terms = [counted, d, np.abs(d), d * d, counted & fi & yi, counted & fi & ~yi, counted & ~fi & yi,
                     counted & ~fi & ~yi]
            for k, term in enumerate(terms):
                sums[:, s, k] += np.where(counted, term.astype(np.float64), 0.0)
    return sums
