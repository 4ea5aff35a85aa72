"""Host checks of the float64 pixel model (tests/transfer_f64.py) on its own: it reproduces the reference's recorded flatten /
unflatten results, equals the CPU oracle on a hand-built masked label map, and every gradient function is the exact transpose of its
forward.  No GPU, nothing of qtmpnn."""
import numpy as np
import torch

import transfer_f64 as M
from helpers import golden


def _hand_map():
    """16 x 24 label map, two clips' worth of structure in one: an 8 x 8 cell with three masked pixels INSIDE it, a node-less 8 x 8
    region, 4 x 4, 2 x 2 and 1 x 1 cells, a masked single pixel.  Returns labels (16, 24) and the node count."""
    lab = -np.ones((16, 24), np.int64)
    nxt = [0]

    def cell(r, c, z):
        lab[r:r + z, c:c + z] = nxt[0]
        nxt[0] += 1
    cell(0, 0, 8)                                   # 64 pixels ...
    lab[2, 3] = lab[2, 4] = lab[7, 7] = -1          # ... three of them masked: 61 left
    for r in (0, 4):
        for c in (8, 12):
            cell(r, c, 4)                           # 16 pixels each
    # columns 16 .. 23 of rows 0 .. 7: no node at all
    for r in range(8, 16, 2):
        for c in range(0, 8, 2):
            cell(r, c, 2)                           # 4 pixels each
    for r in range(8, 16):
        for c in range(8, 16):
            cell(r, c, 1)
    lab[9, 9] = -1                                  # a masked single pixel (its label stays unused: an empty node)
    cell(8, 16, 8)
    return lab, nxt[0]


def test_hand_map_has_the_intended_cells():
    lab, N = _hand_map()
    cnt = M.npix(lab.reshape(1, -1), N)
    assert set(np.unique(cnt).astype(int)) >= {1, 4, 16, 64} and 61 in cnt and 0 in cnt
    assert (lab[0:8, 0:8] < 0).sum() == 3 and (lab[0:8, 0:8] == 0).sum() == 61        # masked pixels inside a cell
    assert (lab[0:8, 16:24] < 0).all()                                                  # a node-less region


def test_model_reproduces_the_recorded_flatten_and_unflatten():
    """tests/golden/transfer.npz was written by the reference in float32 with dense (N, P) products: a node's entry is a sum of npix
    non-zero terms, so it lies within (npix + 2) * 2^-24 * sum |terms| of the float64 model (the standard bound of a float32 sum
    of n terms, plus the rounding of the division and of the stored result)."""
    t = golden('transfer.npz')
    lab = t['labels'].reshape(1, -1).astype(np.int64)
    N = t['npix'].shape[0]
    cnt = M.npix(lab, N)
    assert np.array_equal(cnt, t['npix'].astype(np.float64))
    img = t['img'].astype(np.float64)                               # (ns, 64, 64, c)
    ns, _, _, c = img.shape
    flat, mag = M.pool(img.reshape(1, ns, -1, c), lab, N, True)
    assert (np.abs(flat - t['flat']) <= (cnt[None, :, None] + 2) * M.U * mag).all()
    for s in range(ns):
        gx, gmag = M.gather(t['flat_gy'][s], lab, 1.0 / cnt)
        assert (np.abs(gx[0] - t['flat_gx'][s].reshape(-1, c)) <= 3 * M.U * gmag[0]).all()
    data = t['data'].astype(np.float64)                             # (2, N, 5)
    for s in range(data.shape[0]):
        im, _ = M.gather(data[s], lab)
        assert np.array_equal(im[0].astype(np.float32), t['unflat'][s].reshape(-1, data.shape[2]))
    gi = t['unflat_gi'].astype(np.float64)
    gd, dmag = M.pool(gi.reshape(1, gi.shape[0], -1, gi.shape[-1]), lab, N, False)
    assert (np.abs(gd - t['unflat_gd']) <= (cnt[None, :, None] + 2) * M.U * dmag).all()


def test_model_equals_the_oracle_on_a_masked_non_square_map():
    from oracle import qt_oracle as O
    lab, N = _hand_map()
    rng = np.random.default_rng(0)
    cnt = M.npix(lab.reshape(1, -1), N)
    img = rng.standard_normal((3, 16, 24, 5))
    ref = O.flatten(torch.from_numpy(img), lab, np.maximum(cnt, 1.0)).numpy()
    got, _ = M.pool(img.reshape(1, 3, -1, 5), lab.reshape(1, -1), N, True)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-15)
    val = rng.standard_normal((N, 5))
    ref = O.unflatten(torch.from_numpy(val), lab, (16, 24)).numpy()
    got, _ = M.gather(val, lab.reshape(1, -1))
    assert np.array_equal(got[0].reshape(16, 24, 5), ref)
    # the state transfer = unflatten on the old map, flatten on the new one; the new map: the old one shifted by (3, 5), so that
    # some pixels have a new node but no old one and the other way round
    new = -np.ones_like(lab)
    new[3:, 5:] = lab[:-3, :-5]
    assert ((new >= 0) & (lab < 0)).any() and ((new < 0) & (lab >= 0)).any()
    cn = M.npix(new.reshape(1, -1), N)
    ref = O.flatten(O.unflatten(torch.from_numpy(val), lab, (16, 24))[None], new, np.maximum(cn, 1.0))[0].numpy()
    got, _ = M.remesh(val, lab.reshape(1, -1), new.reshape(1, -1), N)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-15)


def _dot(a, b):
    return float((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum())


def test_every_gradient_function_is_the_transpose_of_its_forward():
    lab0, N = _hand_map()
    lab = np.stack([lab0.reshape(-1), np.where(lab0.reshape(-1)[::-1] >= 0, lab0.reshape(-1)[::-1] + N, -1)])     # two clips
    N2 = 2 * N
    new = np.roll(lab, 29, axis=1)
    new[:, :40] = -1
    rng = np.random.default_rng(1)
    cnt = M.npix(lab, N2)
    inv = 1.0 / np.maximum(cnt, 1.0)

    def same(a, b):
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), (a, b)
    x, g = rng.standard_normal((2, 3, lab.shape[1], 4)), rng.standard_normal((3, N2, 4))
    for mean in (True, False):
        Ax = M.pool(x, lab, N2, mean)[0]
        Atg = np.stack([M.gather(g[s], lab, inv if mean else None)[0] for s in range(3)], axis=1)
        same(_dot(Ax, g), _dot(x, Atg))
    v, gn = rng.standard_normal((N2, 4)), rng.standard_normal((N2, 4))
    same(_dot(M.remesh(v, lab, new, N2)[0], gn), _dot(v, M.remesh_t(gn, lab, new, N2)[0]))
    v4, pf, g4 = rng.standard_normal((N2, 4)), rng.standard_normal((N2, 3)), rng.standard_normal((N2, 4))
    lin = M.decoder_input(v4, pf)[0] - M.decoder_input(np.zeros_like(v4), pf)[0]
    same(_dot(lin, g4), _dot(v4, M.decoder_input_t(g4)[0]))
    assert (M.decoder_input_t(g4)[0][:, 1:] == 0).all()
    # the squared error is quadratic in `out`, so a central difference is its directional derivative exactly
    o, y, d = rng.standard_normal(N2), rng.standard_normal(lab.shape), rng.standard_normal(N2)
    keep = rng.random(lab.shape[1]) < 0.7
    for kp in (None, keep):
        _, _, grad, _ = M.sse(o, lab, y, kp, g=0.37, W=4)
        fd = 0.37 * (M.sse(o + 0.5 * d, lab, y, kp)[0] - M.sse(o - 0.5 * d, lab, y, kp)[0])
        same(fd, _dot(grad[:, 0], d))
        assert (grad[:, 1:] == 0).all()


def test_frame_fills_pixels_without_a_row():
    lab0, N = _hand_map()
    lab = lab0.reshape(1, -1)
    val = np.arange(N, dtype=np.float64)[:, None] + 1.0
    full, _ = M.frame(val, lab, N, np.nan)
    assert np.isnan(full[lab < 0]).all() and np.array_equal(full[lab >= 0][:, 0], lab[lab >= 0] + 1.0)
    cut, _ = M.frame(val, lab, N - 10, 0.0)
    assert (cut[lab >= N - 10] == 0).all() and (cut[lab < 0] == 0).all() and np.array_equal(cut[(lab >= 0) & (lab < N - 10)], full[(lab >= 0) & (lab < N - 10)])
