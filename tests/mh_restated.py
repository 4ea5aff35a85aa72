"""torch_geometric 2.2.0 TransformerConv with any `heads` / `concat`, restated in plain torch from the library's published
definition (beta=False, edge_dim=2, root_weight=True: what the reference's convolutions use).  tests/golden/make_golden_mh.py installs
it as torch_geometric.nn.TransformerConv, so that the reference's MHTransformerConv (a subclass that adds the head merge `lin`) runs on
it; tests/test_mh_host.py pins it to oracle/qt_oracle.py:transformer_conv at heads=1, concat=False.  PARITY WITH PyG ITSELF UNPINNED.

Per head g (C = out_channels):  q = Wq x_i + bq, k = Wk x_j + bk, v = Wv x_j + bv, e = We edge_attr (no bias), all (heads C) wide;
alpha^g = softmax_j(q_i^g . (k_j^g + e^g) / sqrt(C)) over the incoming edges of i (exp(a - max) / (sum + 1e-16)), dropout on alpha;
out_i = concat_g (or mean_g) sum_j alpha^g (v_j^g + e^g), + Wskip x_i + bskip (lin_skip: in -> heads C, or C without concat).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class TransformerConv(nn.Module):
    """Parameters in PyG's creation order: lin_key, lin_query, lin_value (.weight, .bias), lin_edge.weight, lin_skip (.weight, .bias).
    Positional order of the arguments as in PyG: (in, out, heads, concat, beta, dropout, edge_dim, bias, root_weight)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True,
                 root_weight=True, **kwargs):
        super().__init__()
        assert not beta and edge_dim == 2 and root_weight, 'restated for beta=False, edge_dim=2, root_weight=True'
        self.in_channels, self.out_channels, self.heads, self.concat, self.dropout = in_channels, out_channels, heads, concat, dropout
        self.lin_key = nn.Linear(in_channels, heads * out_channels)
        self.lin_query = nn.Linear(in_channels, heads * out_channels)
        self.lin_value = nn.Linear(in_channels, heads * out_channels)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        self.lin_skip = nn.Linear(in_channels, heads * out_channels if concat else out_channels, bias=bias)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        src, dst = edge_index
        n, H, C = x.shape[0], self.heads, self.out_channels
        q = self.lin_query(x).view(n, H, C)
        k = self.lin_key(x).view(n, H, C)
        v = self.lin_value(x).view(n, H, C)
        e = self.lin_edge(edge_attr).view(-1, H, C)
        a = (q[dst] * (k[src] + e)).sum(-1) / math.sqrt(C)                                          # (E, H)
        idx = dst.unsqueeze(1).expand(-1, H)
        amax = torch.full((n, H), -float('inf'), dtype=a.dtype).scatter_reduce(0, idx, a.detach(), 'amax', include_self=True)
        ex = torch.exp(a - amax[dst])
        alpha = ex / (torch.zeros(n, H, dtype=a.dtype).index_add(0, dst, ex)[dst] + 1e-16)
        alpha = F.dropout(alpha, self.dropout, self.training)
        out = torch.zeros(n, H, C, dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * (v[src] + e))
        out = out.reshape(n, H * C) if self.concat else out.mean(dim=1)
        return out + self.lin_skip(x)
