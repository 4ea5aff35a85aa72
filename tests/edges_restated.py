"""Ice-edge distance sums restated in numpy and Python integers from dense frames, written from the definition: indicator,
counted and edge sets from shifted arrays, squared distances by brute force over all pairs of edge pixels, the scaled distance by
math.isqrt.  The checker of qt_edge_rollout, ops.rollout_edges and NextFramePredictorS2S.edge_distance() (tests only; imports
nothing of the package).

counted(p): not under the mask and, where `counted` is given, true there (a pixel with a node).  ice(x) = counted & (x > thr) on
the fp32 values with the threshold rounded to fp32 once, strict: NaN and -inf are not ice, +inf is.  The edge set E(x) holds the
ice pixels with at least one 4-neighbour that is inside the frame, counted and not ice.  d2(p, E) = min over e in E of
dr^2 + dc^2, q = isqrt(65536 d2).  Per step: [n_f, n_o, sum_q_fo, sum_q_of, sum_d2_fo, sum_d2_of, max_d2_fo, max_d2_of], `fo`
over p in E(field) against E(truth), `of` the reverse; a direction whose target set is empty has sum and max 0."""
import math

import numpy as np


def ice(values, counted, thr):
    """(W, H) bool: counted & (values > fp32(thr)) on fp32 values."""
    values = np.asarray(values)
    assert values.dtype == np.float32
    with np.errstate(invalid='ignore'):
        return counted & (values > np.float32(thr))


def edge_set(is_ice, counted):
    """(W, H) bool: ice pixels with a 4-neighbour inside the frame that is counted and not ice."""
    open_water = counted & ~is_ice
    near = np.zeros_like(open_water)
    near[1:, :] |= open_water[:-1, :]               # the neighbour above
    near[:-1, :] |= open_water[1:, :]               # below
    near[:, 1:] |= open_water[:, :-1]               # to the left
    near[:, :-1] |= open_water[:, 1:]               # to the right
    return is_ice & near


def nearest_d2(a, b):
    """Edge sets a, b (W, H) bool, b non-empty -> int64 d2(p, b) for every p of a, in raster order: all pairs."""
    pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
    out = np.empty(len(pa), dtype=np.int64)
    for i in range(0, len(pa), 256):
        d = pa[i:i + 256, None, :] - pb[None, :, :]
        out[i:i + 256] = (d * d).sum(axis=2).min(axis=1)
    return out


def directed(a, b):
    """[sum q, sum d2, max d2] over p in a against b; zeros if either set is empty."""
    if not a.any() or not b.any():
        return [0, 0, 0]
    d2 = [int(v) for v in nearest_d2(a, b)]
    return [sum(math.isqrt(65536 * v) for v in d2), sum(d2), max(d2)]


def restated_edges(field, truth, mask, thr, counted=None):
    """field, truth (T, W, H) float32; mask (W, H) bool, True = not counted, or None; counted (T, W, H) bool or None (all);
    -> sums (T, 8) int64."""
    field, truth = np.asarray(field), np.asarray(truth)
    assert field.dtype == np.float32 and truth.dtype == np.float32 and field.shape == truth.shape and field.ndim == 3
    keep = np.ones(field.shape, dtype=bool) if counted is None else np.asarray(counted, dtype=bool).copy()
    assert keep.shape == field.shape
    if mask is not None:
        keep &= ~np.asarray(mask, dtype=bool)[None]
    sums = np.zeros((len(field), 8), dtype=np.int64)
    for t in range(len(field)):
        ef, eo = edge_set(ice(field[t], keep[t], thr), keep[t]), edge_set(ice(truth[t], keep[t], thr), keep[t])
        fo, of = directed(ef, eo), directed(eo, ef)
        sums[t] = [ef.sum(), eo.sum(), fo[0], of[0], fo[1], of[1], fo[2], of[2]]
    return sums
