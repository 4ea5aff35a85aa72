"""Pixel-space model of the binary cross-entropy training loss, in numpy float64, beside tests/wloss_f64.py and in its terms: a mesh
is known by its label map alone, (B, P) integers with < 0 where a pixel has no node, and a node is the set of pixels that carry its
label.  Nothing of qtmpnn is imported."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
CLAMP = -100.0          # torch's BCELoss clamps both logarithms here
EPS = float(np.float32(1e-12))      # and the denominator of its gradient here: torch's constant is a float, in every precision


def logs(o):
    """(max(log o, -100), max(log(1 - o), -100)) of float64 probabilities."""
    o = np.asarray(o, np.float64)
    with np.errstate(divide='ignore'):
        return np.maximum(np.log(o), CLAMP), np.maximum(np.log1p(-o), CLAMP)


def bce(out_col0, labels, y, keep=None, g=1.0, W=1):
    """Binary cross-entropy of one step: total = - sum over clips b and pixels p with a node (and keep[p], when given) of
    y L1 + (1 - y) L0 with o = out[labels[b, p]], L1 = max(log o, -100), L0 = max(log(1 - o), -100), and its gradient
    g (npix_i o_i - sy_i) / max(o_i (1 - o_i), 1e-12), npix_i and sy_i the count and the sum of y over the node's counted pixels
    (torch's (o - y) / max(o (1 - o), 1e-12) summed over them), as full rows of width W with exact zeros outside column 0.
    Returns (total, mag_total, grad (N, W), mag_grad (N, W)).  mag_total is the sum over the pixels of |y L1| + |L0| + |y L0|, the
    absolute values of the terms y L1, L0, -y L0; mag_grad[:, 0] = |g| (npix |o| + sum |y|) / max(o (1 - o), 1e-12): a per-pixel and
    a per-node evaluation of the gradient both lie within a rounding bound times it."""
    o = np.asarray(out_col0, np.float64).reshape(-1)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 2, 'labels: (B, P)'
    y = np.asarray(y, np.float64).reshape(lab.shape)
    ok = lab >= 0
    if keep is not None:
        ok = ok & (np.asarray(keep).reshape(1, -1) != 0)
    N = o.shape[0]
    l1, l0 = logs(o)
    idx, yk = lab[ok], y[ok]
    total = -float((yk * l1[idx] + (1.0 - yk) * l0[idx]).sum())
    mag_total = float((np.abs(yk * l1[idx]) + np.abs(l0[idx]) + np.abs(yk * l0[idx])).sum())
    cnt, sy, say = np.zeros(N), np.zeros(N), np.zeros(N)
    np.add.at(cnt, idx, 1.0)
    np.add.at(sy, idx, yk)
    np.add.at(say, idx, np.abs(yk))
    den = np.maximum(o * (1.0 - o), EPS)
    grad, mag = np.zeros((N, W)), np.zeros((N, W))
    grad[:, 0] = g * (cnt * o - sy) / den
    mag[:, 0] = abs(g) * (cnt * np.abs(o) + say) / den
    return total, mag_total, grad, mag
