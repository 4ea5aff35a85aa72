"""Edge-softmax attention with counter-hash dropout restated in float64, written from the definitions: the checker of qt_attn_fwd /
qt_attn_bwd (csrc/attn.hip) and of ops._Attention (tests only; plain torch / numpy on the CPU, nothing of qtmpnn is imported).

Operands as the kernels take them: proj (N, G 4C) = per head [q | k | v | skip], We (G, C, 2); the message col[e] -> row(e) carries
the attributes eattr[e], every node with selfpair > 0 one more pair (i, i) with attributes 0 (selfpair None: no self pairs).

    s_p   = q_i . (k_j + We a_p) / sqrt(c_real)                 over all C columns (the columns above c_real are the caller's padding)
    alpha = softmax of s over the pairs of target i
    out_i = sum_p alpha_p d_p (v_j + We a_p) + skip_i           d_p = 0 or 1 / keep, a constant of the differentiation

tests/test_attn_f64_host.py pins this to the restatement of PyG's TransformerConv (tests/mh_restated.py) and the mask's statistics."""
import math
from types import SimpleNamespace

import numpy as np
import torch

_M32 = 0xFFFFFFFF


def dropout_mask(seed, epoch, head, i, j, keep):
    """True where the pair (target i, source j) of `head` is kept at step `epoch` ("Attention dropout mask")."""
    i, j = np.asarray(i).astype(np.uint64), np.asarray(j).astype(np.uint64)
    head_seed = (int(seed) + int(head) * 0x632BE5AB) & _M32
    eff = head_seed ^ ((int(epoch) * 0x9E3779B9) & _M32)
    h = np.uint64(eff) ^ ((i * np.uint64(0x9E3779B1)) & np.uint64(_M32)) ^ ((j * np.uint64(0x85EBCA77)) & np.uint64(_M32))
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & np.uint64(_M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & np.uint64(_M32)
    h ^= h >> np.uint64(16)
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(keep)


def pairs_of(rowptr, col, selfpair):
    """(tgt, src, edge) int64 arrays of all pairs: the E stored edges in CSR order (edge = e), then the self pairs (edge = -1)."""
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
    N = len(rowptr) - 1
    E = int(rowptr[N])
    tgt = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    src = col[:E]
    if selfpair is not None:
        own = np.nonzero(np.asarray(selfpair)[:N] > 0)[0].astype(np.int64)
        tgt, src = np.concatenate([tgt, own]), np.concatenate([src, own])
    edge = np.concatenate([np.arange(E, dtype=np.int64), np.full(len(tgt) - E, -1, dtype=np.int64)])
    return tgt, src, edge


def attention_f64(rowptr, col, selfpair, eattr, proj, We, c_real, heads, keep, seed, epoch, gmod=0, dtype=torch.float64):
    """-> namespace: out (N, gmod C) attached to the leaves proj / We (requires_grad, `dtype`); tgt, src, edge (pairs,);
    alpha, mult (pairs, G): softmax coefficient before dropout and the dropout multiplier; absum (N, gmod C): per output entry
    sum_p alpha d |v_j + We a| + |skip| (what a rounding-error bound scales with); spread (N, G): max - min score per target.
    `dtype` = float32 runs the same statements in single precision (the yardstick of an accumulation-order bound)."""
    G = int(heads)
    gmod = int(gmod) or G
    tgt_np, src_np, edge_np = pairs_of(rowptr, col, selfpair)
    N = len(np.asarray(rowptr)) - 1
    E = int((edge_np >= 0).sum())
    proj = torch.as_tensor(np.asarray(proj)).to(dtype)[:N].clone().requires_grad_(True)
    We = torch.as_tensor(np.asarray(We)).to(dtype).reshape(G, -1, 2).clone().requires_grad_(True)
    C = We.shape[1]
    assert proj.shape == (N, G * 4 * C), (proj.shape, N, G, C)
    attr = torch.zeros(len(tgt_np), 2, dtype=dtype)
    attr[:E] = torch.as_tensor(np.asarray(eattr)).to(dtype)[:E]
    tgt, src = torch.from_numpy(tgt_np), torch.from_numpy(src_np)

    mult = np.ones((len(tgt_np), G))
    if keep < 1.0:
        inv_keep = 1.0 / float(np.float32(keep))
        for g in range(G):
            mult[:, g] = np.where(dropout_mask(seed, epoch, g, tgt_np, src_np, keep), inv_keep, 0.0)
    mult = torch.from_numpy(mult).to(dtype)

    P = proj.view(N, G, 4, C)
    q, k, v, skip = P[:, :, 0], P[:, :, 1], P[:, :, 2], P[:, :, 3]
    e = torch.einsum('gck,pk->pgc', We, attr)                              # (pairs, G, C)
    s = (q[tgt] * (k[src] + e)).sum(-1) / math.sqrt(c_real)                # (pairs, G)
    idx = tgt.unsqueeze(1).expand(-1, G)
    smax = torch.full((N, G), -math.inf, dtype=dtype).scatter_reduce(0, idx, s.detach(), 'amax', include_self=True)
    smin = torch.full((N, G), math.inf, dtype=dtype).scatter_reduce(0, idx, s.detach(), 'amin', include_self=True)
    has = torch.zeros(N, dtype=torch.bool).index_fill(0, tgt, True)
    ex = torch.exp(s - smax[tgt])
    alpha = ex / torch.zeros(N, G, dtype=dtype).index_add(0, tgt, ex)[tgt]
    msg = v[src] + e
    w = (alpha * mult).unsqueeze(-1)
    out = torch.zeros(N, G, C, dtype=dtype).index_add(0, tgt, w * msg) + skip          # no pair: out_i = skip_i
    absum = torch.zeros(N, G, C, dtype=dtype).index_add(0, tgt, (w * msg.abs()).detach()) + skip.detach().abs()
    spread = torch.where(has.unsqueeze(1), smax - smin, torch.zeros(N, G, dtype=dtype))

    def groups(t):
        return t.reshape(N, G // gmod, gmod * C).sum(dim=1)
    return SimpleNamespace(out=groups(out), absum=groups(absum), proj=proj, We=We, tgt=tgt_np, src=src_np, edge=edge_np,
                           alpha=alpha.detach(), mult=mult, spread=spread, N=N, E=E, G=G, C=C, gmod=gmod)


def gradients(ref, g):
    """(d proj (N, G 4C), d We (G, C, 2)) of sum(out * g) by autograd, the mask held constant; g (N, gmod C)."""
    g = torch.as_tensor(np.asarray(g)).to(ref.out.dtype)[:ref.N]
    gp, gw = torch.autograd.grad(ref.out, [ref.proj, ref.We], g, retain_graph=True)
    return gp, gw
