"""Pixel-space model of the weighted training loss, in numpy float64, beside tests/transfer_f64.py and in its terms: a mesh is
known by its label map alone, (B, P) integers with < 0 where a pixel has no node, and a node is the set of pixels that carry its
label.  Nothing of qtmpnn is imported."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def wsse(out_col0, labels, y, w, lam, keep=None, g=1.0, W=1):
    """Weighted squared error of one step: total = lam * sum over clips b and pixels p with a node (and keep[p], when given) of
    w[p] (out[labels[b, p]] - y[b, p])^2, and its gradient 2 g lam (sw_i out_i - swy_i), sw_i = sum of w and swy_i = sum of w y
    over the node's counted pixels, as full rows of width W with exact zeros outside column 0.
    Returns (total, mag_total, grad (N, W), mag_grad (N, W)); mag holds the sum of the absolute values of an entry's terms:
    every term of the total is >= 0, so mag_total == total, and mag_grad[:, 0] = 2 |g| lam (sw |out| + sum of w |y|)."""
    o = np.asarray(out_col0, np.float64).reshape(-1)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 2, 'labels: (B, P)'
    y = np.asarray(y, np.float64).reshape(lab.shape)
    w = np.broadcast_to(np.asarray(w, np.float64).reshape(1, -1), lab.shape)
    lam = float(lam)
    assert (w >= 0).all() and lam >= 0
    ok = lab >= 0
    if keep is not None:
        ok = ok & (np.asarray(keep).reshape(1, -1) != 0)
    N = o.shape[0]
    d = o[np.where(ok, lab, 0)] - y
    total = lam * float((w[ok] * d[ok] ** 2).sum())
    sw, swy, sway = np.zeros(N), np.zeros(N), np.zeros(N)
    np.add.at(sw, lab[ok], w[ok])
    np.add.at(swy, lab[ok], w[ok] * y[ok])
    np.add.at(sway, lab[ok], w[ok] * np.abs(y[ok]))
    grad, mag = np.zeros((N, W)), np.zeros((N, W))
    grad[:, 0] = 2.0 * g * lam * (sw * o - swy)
    mag[:, 0] = 2.0 * abs(g) * lam * (sw * np.abs(o) + sway)
    return total, total, grad, mag
