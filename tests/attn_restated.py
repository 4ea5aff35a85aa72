"""The attention coefficients of tests/mh_restated.py's TransformerConv (PyG 2.2.0 restated), and a subclass that records them.

coefficients() is the alpha of mh_restated.TransformerConv.forward before dropout: per head g,
alpha^g_e = exp(a_e - max) / (sum + 1e-16) over the incoming edges of dst(e), a_e = q_dst . (k_src + e) / sqrt(C).
RecordingTransformerConv runs the restatement unchanged and, while `RecordingTransformerConv.log` is a list, appends one entry per
call: the module, the edge_index it received and alpha (E, heads) in that edge order.  tests/golden/make_golden_attn.py installs it
as torch_geometric.nn.TransformerConv under the reference's modules.
"""
import math

import torch

from mh_restated import TransformerConv


def coefficients(conv, x, edge_index, edge_attr):
    """alpha (E, heads) of `conv` (an mh_restated.TransformerConv) for the messages edge_index[0] -> edge_index[1]."""
    src, dst = edge_index
    n, H, C = x.shape[0], conv.heads, conv.out_channels
    q = conv.lin_query(x).view(n, H, C)
    k = conv.lin_key(x).view(n, H, C)
    e = conv.lin_edge(edge_attr).view(-1, H, C)
    a = (q[dst] * (k[src] + e)).sum(-1) / math.sqrt(C)
    idx = dst.unsqueeze(1).expand(-1, H)
    amax = torch.full((n, H), -float('inf'), dtype=a.dtype).scatter_reduce(0, idx, a, 'amax', include_self=True)
    ex = torch.exp(a - amax[dst])
    return ex / (torch.zeros(n, H, dtype=a.dtype).index_add(0, dst, ex)[dst] + 1e-16)


class RecordingTransformerConv(TransformerConv):
    log = None          # a list while recording

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        out = super().forward(x, edge_index, edge_attr)
        if RecordingTransformerConv.log is not None:
            with torch.no_grad():
                alpha = coefficients(self, x, edge_index, edge_attr)
            RecordingTransformerConv.log.append(dict(module=self, edge_index=edge_index.detach().clone(), alpha=alpha))
        return out
