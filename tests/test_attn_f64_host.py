"""Host checks of the float64 attention restatement (tests/attn_f64.py) on its own: against the restatement of PyG's TransformerConv
(tests/mh_restated.py) without dropout, and the statistics of the counter-hash dropout mask.  No GPU, nothing of qtmpnn."""
import itertools

import numpy as np
import pytest
import torch

from attn_f64 import attention_f64, dropout_mask, gradients


def _random_symmetric_graph(N, seed):
    """CSR of a random symmetric graph (row = target, col = source), attributes with attr(j -> i) = [angle + 1/2 mod 1, dist] of
    attr(i -> j), self pairs on about half of the nodes (never stored as edges)."""
    rng = np.random.default_rng(seed)
    und = set()
    for i in range(N):
        for j in rng.choice(N, size=3, replace=False):
            if i != j:
                und.add((min(i, int(j)), max(i, int(j))))
    attr = {}
    for i, j in und:
        ang, dist = float(rng.random()), float(0.25 + 3 * rng.random())
        attr[(i, j)] = (ang, dist)
        attr[(j, i)] = ((ang + 0.5) % 1.0, dist)
    keys = sorted(attr)                                       # (target, source), row major
    rowptr = np.zeros(N + 1, dtype=np.int32)
    for i, _ in keys:
        rowptr[i + 1] += 1
    rowptr = np.cumsum(rowptr).astype(np.int32)
    col = np.array([j for _, j in keys], dtype=np.int32)
    eattr = np.array([attr[k] for k in keys], dtype=np.float64)
    selfpair = (rng.random(N) < 0.5).astype(np.float32)
    return rowptr, col, eattr, selfpair


@pytest.mark.parametrize('heads', [1, 3])
def test_restatement_equals_pyg_restatement_without_dropout(heads):
    """keep = 1: output and every gradient of attention_f64 equal mh_restated.TransformerConv in float64 on the same edge list, the
    projections fed as the module's linears (identity input), to 1e-12 relative."""
    import mh_restated
    N, C, G = 37, 5, heads
    rowptr, col, eattr, selfpair = _random_symmetric_graph(N, 11 + heads)
    assert (selfpair > 0).any() and (selfpair == 0).any() and (np.diff(rowptr) > 0).all()
    rng = np.random.default_rng(3)
    proj = rng.standard_normal((N, G * 4 * C))
    We = rng.standard_normal((G, C, 2))
    g = rng.standard_normal((N, G * C))
    ref = attention_f64(rowptr, col, selfpair, eattr, proj, We, C, G, 1.0, 0, 0)
    gp, gw = gradients(ref, g)

    # the PyG module on x = proj: its linears select the q / k / v / skip blocks (weights = selection matrices, no bias)
    conv = mh_restated.TransformerConv(G * 4 * C, C, heads=G, concat=True, edge_dim=2).double()
    P = np.arange(G * 4 * C).reshape(G, 4, C)
    with torch.no_grad():
        for lin, blk in ((conv.lin_query, 0), (conv.lin_key, 1), (conv.lin_value, 2), (conv.lin_skip, 3)):
            lin.weight.zero_()
            lin.bias.zero_()
            lin.weight[torch.arange(G * C), torch.from_numpy(P[:, blk].reshape(-1))] = 1.0
        conv.lin_edge.weight.copy_(torch.from_numpy(We.reshape(G * C, 2)))
    own = np.nonzero(selfpair > 0)[0]
    tgt = np.concatenate([np.repeat(np.arange(N), np.diff(rowptr)), own])
    src = np.concatenate([col, own])
    ea = np.concatenate([eattr, np.zeros((len(own), 2))])
    perm = np.random.default_rng(5).permutation(len(tgt))                      # PyG's result does not depend on the edge order
    x = torch.from_numpy(proj).requires_grad_(True)
    out = conv(x, torch.from_numpy(np.stack([src, tgt])[:, perm]), torch.from_numpy(ea[perm]))
    gx, gwe = torch.autograd.grad(out, [x, conv.lin_edge.weight], torch.from_numpy(g))

    def same(a, b, what):
        a, b = a.detach().numpy(), b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (what, np.abs(a - b).max(), np.abs(b).max())
    same(ref.out, out, 'out')
    same(gp, gx, 'd proj')
    same(gw.reshape(G * C, 2), gwe, 'd We')
    assert all(float(gp.view(N, G, 4, C)[:, :, b].abs().max()) > 0 for b in range(4))


def _grid_pairs(n=40):
    """(target, source) of a n x n 4-neighbour grid plus one self pair per node."""
    idx = np.arange(n * n).reshape(n, n)
    a = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel()])
    b = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel()])
    return np.concatenate([a, b, idx.ravel()]), np.concatenate([b, a, idx.ravel()])


@pytest.mark.parametrize('keep', [0.9, 0.5])
@pytest.mark.parametrize('seed', [1234, 0, 0xDEADBEEF, 2654435768])
def test_mask_statistics(keep, seed):
    """8 heads x epochs {0, 1, 2} on the 7840 pairs of a 40 x 40 grid: every mask's keep rate within 5 binomial standard deviations of
    keep; every two masks (across heads and across epochs) and each mask against its transpose (i, j) <-> (j, i) agree on a fraction
    within 5 sigma of keep^2 + (1 - keep)^2, the agreement of independent draws."""
    i, j = _grid_pairs()
    n = len(i)
    assert n == 7840
    masks = {(h, ep): dropout_mask(seed, ep, h, i, j, keep) for h in range(8) for ep in (0, 1, 2)}
    s_rate = np.sqrt(keep * (1 - keep) / n)
    p = keep * keep + (1 - keep) * (1 - keep)
    s_agree = np.sqrt(p * (1 - p) / n)
    for key, m in masks.items():
        assert abs(m.mean() - keep) <= 5 * s_rate, (key, m.mean())
    for (ka, ma), (kb, mb) in itertools.combinations(masks.items(), 2):
        assert abs((ma == mb).mean() - p) <= 5 * s_agree, (ka, kb, (ma == mb).mean())
    off = i != j                                             # (a self pair is its own transpose)
    s_off = np.sqrt(p * (1 - p) / off.sum())
    for (h, ep), m in masks.items():
        t = dropout_mask(seed, ep, h, j, i, keep)
        assert abs((m[off] == t[off]).mean() - p) <= 5 * s_off, (h, ep, (m[off] == t[off]).mean())


def test_mask_scalar_definition():
    """The vectorised mask equals the definition evaluated one pair at a time in Python integers; keep = 1 keeps everything."""
    def one(seed, epoch, head, i, j, keep):
        m = 0xFFFFFFFF
        eff = ((seed + head * 0x632BE5AB) & m) ^ ((epoch * 0x9E3779B9) & m)
        h = eff ^ ((i * 0x9E3779B1) & m) ^ ((j * 0x85EBCA77) & m)
        h ^= h >> 16
        h = (h * 0x7FEB352D) & m
        h ^= h >> 15
        h = (h * 0x846CA68B) & m
        h ^= h >> 16
        return np.float32(h >> 8) * np.float32(2.0 ** -24) < np.float32(keep)
    rng = np.random.default_rng(0)
    i, j = rng.integers(0, 1 << 20, 500), rng.integers(0, 1 << 20, 500)
    for seed, epoch, head, keep in ((0xDEADBEEF, 7, 5, 0.5), (0, 0, 0, 0.9), (0xFFFFFFFF, 3, 63, 0.1)):
        want = np.array([one(seed, epoch, head, int(a), int(b), keep) for a, b in zip(i, j)])
        assert np.array_equal(dropout_mask(seed, epoch, head, i, j, keep), want)
    assert dropout_mask(1, 2, 3, i, j, 1.0).all()
