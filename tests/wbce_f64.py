"""Pixel-space model of the weighted binary cross-entropy training loss, in numpy float64, beside tests/bce_f64.py and
tests/wloss_f64.py and in their terms: a mesh is known by its label map alone, (B, P) integers with < 0 where a pixel has no node,
and a node is the set of pixels that carry its label.  Nothing of qtmpnn is imported."""
import numpy as np

from bce_f64 import CLAMP, EPS, U, logs  # noqa: F401  (one clamp, one epsilon, one unit roundoff for both models)


def wbce(out_col0, labels, y, w, lam, pw, keep=None, g=1.0, W=1):
    """Weighted binary cross-entropy of one step: total = - lam * sum over clips b and pixels p with a node (and keep[p], when given)
    of w[p] (pw y L1 + (1 - y) L0) with o = out[labels[b, p]], L1 = max(log o, -100), L0 = max(log(1 - o), -100), and its gradient
    g lam (o_i sw_i - swy_i (pw + o_i (1 - pw))) / max(o_i (1 - o_i), 1e-12), sw_i = sum of w and swy_i = sum of w y over the node's
    counted pixels (the per-pixel (o - y (pw + o (1 - pw))) / (o (1 - o)) summed over them with their weights), as full rows of
    width W with exact zeros outside column 0.
    Returns (total, mag_total, grad (N, W), mag_grad (N, W)).  mag holds the sum of the absolute values of the terms actually added:
    mag_total = lam * sum of w (|pw y L1| + |L0| + |y L0|) (the terms pw y L1, L0, -y L0 of every pixel), and
    mag_grad[:, 0] = |g| lam (|o| sw + (pw + o (1 - pw)) sum of w |y|) / max(o (1 - o), 1e-12); an entry whose terms all vanish
    (lam = 0, a node whose pixels all have w = 0) has mag = 0."""
    o = np.asarray(out_col0, np.float64).reshape(-1)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 2, 'labels: (B, P)'
    y = np.asarray(y, np.float64).reshape(lab.shape)
    w = np.broadcast_to(np.asarray(w, np.float64).reshape(1, -1), lab.shape)
    lam, pw = float(lam), float(pw)
    assert (w >= 0).all() and lam >= 0 and pw > 0
    ok = lab >= 0
    if keep is not None:
        ok = ok & (np.asarray(keep).reshape(1, -1) != 0)
    N = o.shape[0]
    l1, l0 = logs(o)
    idx, yk, wk = lab[ok], y[ok], w[ok]
    total = -lam * float((wk * (pw * yk * l1[idx] + (1.0 - yk) * l0[idx])).sum())
    mag_total = lam * float((wk * (np.abs(pw * yk * l1[idx]) + np.abs(l0[idx]) + np.abs(yk * l0[idx]))).sum())
    sw, swy, sway = np.zeros(N), np.zeros(N), np.zeros(N)
    np.add.at(sw, idx, wk)
    np.add.at(swy, idx, wk * yk)
    np.add.at(sway, idx, wk * np.abs(yk))
    den = np.maximum(o * (1.0 - o), EPS)
    c = pw + o * (1.0 - pw)             # > 0 for o in [0, 1] and pw > 0
    grad, mag = np.zeros((N, W)), np.zeros((N, W))
    grad[:, 0] = g * lam * (o * sw - swy * c) / den
    mag[:, 0] = abs(g) * lam * (np.abs(o) * sw + sway * np.abs(c)) / den
    return total, mag_total, grad, mag
