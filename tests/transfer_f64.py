"""Pixel-space model of the mesh <-> image transfers and of the training loss, in numpy float64.

Everything here works from a mesh's `labels` array alone: (B, P) integers, the clip-global node row of every pixel, < 0 where a
pixel has no node.  No level, no cell record, no pixel count, no tile: a node IS the set of pixels that carry its label.  Plain
loops over clips and np.add.at; nothing of qtmpnn is imported.

Every function returns (value, mag): `mag` has the shape of `value` and holds, per entry, the sum of the absolute values of the
terms that the entry is the sum of (after any scaling).  The GPU tests bound |kernel - value| by a multiple of 2^-24 * mag.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def _lab(labels):
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 2, 'labels: (B, P)'
    return lab


def npix(labels, N):
    """(N,) number of pixels that carry each label: what the kernels divide by."""
    lab = _lab(labels).reshape(-1)
    return np.bincount(lab[lab >= 0], minlength=N).astype(np.float64)[:N]


def _scale(cnt):
    return 1.0 / np.maximum(cnt, 1.0)


def pool(img, labels, N, mean):
    """img (B, S, P, C) -> node sums or means (S, N, C): node i of step s = sum over the pixels p of clip b with labels[b, p] == i of
    img[b, s, p] (divided by the node's pixel count when `mean`).  Pixels without a node take no part."""
    img = np.asarray(img, np.float64)
    lab = _lab(labels)
    B, S, P, C = img.shape
    out, mag = np.zeros((S, N, C)), np.zeros((S, N, C))
    for b in range(B):
        ok = lab[b] >= 0
        for s in range(S):
            np.add.at(out[s], lab[b][ok], img[b, s][ok])
            np.add.at(mag[s], lab[b][ok], np.abs(img[b, s][ok]))
    if mean:
        sc = _scale(npix(lab, N))[None, :, None]
        out, mag = out * sc, mag * sc
    return out, mag


def gather(val, labels, inv_npix=None):
    """The transpose of pool: val (N, C) -> pixels (B, P, C), pixel p = val[labels[p]] (times inv_npix[labels[p]] when given: the
    transpose of the mean); pixels without a node are 0."""
    val = np.asarray(val, np.float64)
    lab = _lab(labels)
    if inv_npix is not None:
        val = val * np.asarray(inv_npix, np.float64)[:, None]
    ok = lab >= 0
    img = val[np.where(ok, lab, 0)] * ok[..., None]
    return img, np.abs(img)


def remesh(val_old, labels_old, labels_new, N_new):
    """State transfer old mesh -> new mesh: new node i = (1 / npix_new[i]) * sum over its pixels p of val_old[labels_old[p]].

    A pixel that has a node in the new mesh but none in the old one contributes ZERO to the sum and still counts in npix_new:
    that is what the kernels do (csrc/transfer.hip tile_body / k_pool_nodes load a source row only where the source label is >= 0
    and scale by the destination's full pixel count; csrc/remeshclip.hip likewise) and what un-flattening on the old mesh -- 0
    where it has no node -- followed by flattening on the new one gives."""
    val_old = np.asarray(val_old, np.float64)
    lo, ln = _lab(labels_old), _lab(labels_new)
    C = val_old.shape[1]
    out, mag = np.zeros((N_new, C)), np.zeros((N_new, C))
    ok = (ln >= 0) & (lo >= 0)
    np.add.at(out, ln[ok], val_old[lo[ok]])
    np.add.at(mag, ln[ok], np.abs(val_old[lo[ok]]))
    sc = _scale(npix(ln, N_new))[:, None]
    return out * sc, mag * sc


def remesh_t(g_new, labels_old, labels_new, N_old):
    """The transpose of remesh: old node j = sum over its pixels p (that have a new node) of g_new[l_new[p]] / npix_new[l_new[p]]."""
    g_new = np.asarray(g_new, np.float64)
    lo, ln = _lab(labels_old), _lab(labels_new)
    C = g_new.shape[1]
    gs = g_new * _scale(npix(ln, g_new.shape[0]))[:, None]
    out, mag = np.zeros((N_old, C)), np.zeros((N_old, C))
    ok = (ln >= 0) & (lo >= 0)
    np.add.at(out, lo[ok], gs[ln[ok]])
    np.add.at(mag, lo[ok], np.abs(gs[ln[ok]]))
    return out, mag


def decoder_input(val4, posfeat):
    """[val4[:, 0] | posfeat] (N, 4): a copy, entry by entry."""
    val4, posfeat = np.asarray(val4, np.float64), np.asarray(posfeat, np.float64)
    out = np.concatenate([val4[:, :1], posfeat], axis=1)
    return out, np.abs(out)


def decoder_input_t(g):
    """Its backward: column 0 passes, columns 1..3 are exact zeros."""
    g = np.asarray(g, np.float64)
    out = np.zeros_like(g)
    out[:, 0] = g[:, 0]
    return out, np.abs(out)


def sse(out_col0, labels, y, keep=None, g=1.0, W=1):
    """Squared error of one step: total = sum over clips b and pixels p with a node (and keep[p], when given) of
    (out[labels[b, p]] - y[b, p])^2, and its gradient 2 g (npix_i out_i - sum_p y_p) over the same pixels, as full rows of
    width W with exact zeros outside column 0.  Returns (total, mag_total, grad (N, W), mag_grad (N, W)); every term of the
    total is a square, so mag_total == total."""
    o = np.asarray(out_col0, np.float64).reshape(-1)
    lab = _lab(labels)
    y = np.asarray(y, np.float64).reshape(lab.shape)
    ok = lab >= 0
    if keep is not None:
        ok = ok & (np.asarray(keep).reshape(1, -1) != 0)
    N = o.shape[0]
    d = o[np.where(ok, lab, 0)] - y
    total = float((d[ok] ** 2).sum())
    cnt = np.zeros(N)
    sy, say = np.zeros(N), np.zeros(N)
    np.add.at(cnt, lab[ok], 1.0)
    np.add.at(sy, lab[ok], y[ok])
    np.add.at(say, lab[ok], np.abs(y[ok]))
    grad, mag = np.zeros((N, W)), np.zeros((N, W))
    grad[:, 0] = 2.0 * g * (cnt * o - sy)
    mag[:, 0] = 2.0 * abs(g) * (cnt * np.abs(o) + say)
    return total, total, grad, mag


def frame(val, labels, n_rows, fill):
    """One output frame: pixel p = val[labels[p]] where 0 <= labels[p] < n_rows, else `fill`.  (B, P, C); a copy, no arithmetic."""
    val = np.asarray(val, np.float64)
    lab = _lab(labels)
    ok = (lab >= 0) & (lab < n_rows)
    out = np.where(ok[..., None], val[np.where(ok, lab, 0)], fill)
    return out, np.abs(out)
