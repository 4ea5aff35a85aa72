"""Graph-recurrent cells of the hot path: the reference's model/model.py names (GraphConv,
GConvLSTM, CONVOLUTIONS, CONVOLUTION_KWARGS ...) with the same parameters / state-dict keys, computed
by fused HIP kernels (qtmpnn.ops) on a `Mesh` instead of per-module PyG calls.

Where the reference passes (edge_index, edge_weight) these modules take the Mesh in the edge_index
slot; the Mesh already holds the ChebConv normalisation, which PyG recomputes in every call.
"""

import torch
import torch.nn as nn

from qtmpnn import ops, recompute
from qtmpnn.mesh import Mesh

_MULTI_CONV = True     # comparator: tests/test_gpu_ops.py sets it False (one projection + attention launch pair per convolution)


class ChebConv(nn.Module):
    """Parameter layout of torch_geometric ChebConv (lins.{k}.weight (out, in) glorot, bias zeros);
    reference kwargs K=3, normalization='sym', bias=True (model/model.py:53)."""

    def __init__(self, in_channels, out_channels, K=3, normalization='sym', bias=True):
        super().__init__()
        assert normalization == 'sym', 'only the symmetric normalisation is used by the reference'
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        for lin in self.lins:
            nn.init.xavier_uniform_(lin.weight)

    def plan_params(self):
        return [lin.weight for lin in self.lins] + [self.bias]

    def cheb_coeffs(self, T):
        """Coefficient matrices (K, in, out) of the Chebyshev series this layer applies, from its plan_params() or index stand-ins of
        them: the hook every layout takes a layer's weights through (GCNConv overrides it)."""
        return torch.stack(T[:self.K]).transpose(1, 2)

    def plan_layout(self, T, fill, in_pad=None, out_pad=None):
        """[W_0^T; ...; W_{K-1}^T; bias; 0 0 0] as one ((K*in_pad)+4, out_pad) matrix padded with `fill`, from plan_params() or
        stand-ins of them (data movement only, see ops.PackPlan)."""
        cin, cout = in_pad or self.in_channels, out_pad or self.out_channels
        w = nn.functional.pad(self.cheb_coeffs(T), (0, cout - self.out_channels, 0, cin - self.in_channels), value=fill)
        tail = nn.functional.pad(T[-1].unsqueeze(0), (0, cout - self.out_channels, 0, 3), value=fill)    # bias row + 3 padding rows
        return torch.cat([w.reshape(self.K * cin, cout), tail], dim=0)

    def packed(self, in_pad=None, out_pad=None):
        """plan_layout of the parameters themselves, zero padded; a zero row stands in for the bias of a bias=False layer."""
        T = self.plan_params()
        if self.bias is None:
            T[-1] = T[0].new_zeros(self.out_channels)
        return self.plan_layout(T, 0.0, in_pad, out_pad)

    def plan_layout_projected(self, T, fill):
        """A K = 3 layer with ONE output channel as the (in + 4, 4) matrix [w_0 w_1 w_2 0 ; b 0 0 0 ; 0 ...]: the operand of
        `project first, then propagate` (ops.scalar_cheb3) -- U = z @ this gives the three coefficient products and the bias."""
        assert self.K == 3 and self.out_channels == 1 and self.in_channels % 4 == 0
        w = nn.functional.pad(torch.stack(T[:3])[:, 0, :].t(), (0, 1), value=fill)             # (in, 4)
        tail = nn.functional.pad(T[3].view(1, 1), (0, 3, 0, 3), value=fill)                      # (4, 4): [b 0 0 0] + 3 zero rows
        return torch.cat([w, tail], dim=0)

    def forward(self, x, edge_index, edge_weight=None):
        mesh = _need_mesh(edge_index, x)
        pad = (-x.shape[1]) % 4
        xin = nn.functional.pad(x, (0, pad)) if pad else x
        opad = (-self.out_channels) % 4
        y = ops.cheb_poly(xin, self.packed(xin.shape[1], self.out_channels + opad), mesh, self.K, 1)
        return y[:, :self.out_channels] if opad else y


class GCNConv(ChebConv):
    """torch_geometric GCNConv(add_self_loops=False) (model/model.py:50; parameters lin.weight (out, in), bias):
    out = A^ (x W^T) + b with A^_ij = d_i^-1/2 w_ij d_j^-1/2.  The mesh weights are symmetric and its self pairs have
    weight 0, so A^ = -L^ off the diagonal: a GCNConv IS the Chebyshev series [0, -W^T] and reuses the ChebConv
    kernels, including the weight-space composition of stacked layers."""

    def __init__(self, in_channels, out_channels, add_self_loops=False):
        nn.Module.__init__(self)
        assert not add_self_loops, 'the reference uses add_self_loops=False'
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, 2
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.lin.weight)

    def plan_params(self):
        return [self.lin.weight, self.bias]

    def cheb_coeffs(self, T):       # (the negation is arithmetic, not data movement: GCNConv layouts are evaluated directly, never planned)
        wt = T[0].t()
        return torch.stack([torch.zeros_like(wt), -wt])


class TransformerConv(nn.Module):
    """torch_geometric TransformerConv(heads=1, edge_dim=2, dropout=0.1, concat=False) (model/model.py:51): parameters
    lin_key / lin_query / lin_value (.weight (out, in), .bias), lin_edge.weight (out, 2), lin_skip (.weight, .bias).
    One projection GEMM produces [q | k | v | skip]; the edge softmax runs in the fused attention kernel, which
    recomputes the [angle, dist] edge attributes from the node centroids."""

    def __init__(self, in_channels, out_channels, heads=1, edge_dim=2, dropout=0.0, concat=False):
        super().__init__()
        assert heads == 1 and not concat and edge_dim == 2, 'the reference uses heads=1, concat=False, edge_dim=2'
        self.in_channels, self.out_channels, self.dropout = in_channels, out_channels, dropout
        self.lin_key = nn.Linear(in_channels, out_channels)
        self.lin_query = nn.Linear(in_channels, out_channels)
        self.lin_value = nn.Linear(in_channels, out_channels)
        self.lin_edge = nn.Linear(edge_dim, out_channels, bias=False)
        self.lin_skip = nn.Linear(in_channels, out_channels)
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge, self.lin_skip):
            nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)

    def pack(self):
        """(W, We, accumulators) for one forward pass: the fused projection [q | k | v | skip] with its bias row, the padded edge
        weight, and the gradient accumulators all uses of this convolution in the pass share (a recurrent cell calls it once per
        time step: packing per call cost ~40 tiny kernels each time, forward + backward)."""
        return TransformerConv.pack_many([self])[0]

    def plan_params(self):
        """The parameters in module order (= the stand-ins proj_layout receives)."""
        return [self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias, self.lin_value.weight,
                self.lin_value.bias, self.lin_edge.weight, self.lin_skip.weight, self.lin_skip.bias]

    @staticmethod
    def proj_layout(Ts, cin, cout, fill):
        """(W (n, cin_p + 4, 4 cp), We (n, cp, 2)) of n convolutions of one (in, out) shape from their plan_params() lists (or index
        stand-ins of them: data movement only, padding = `fill`, see ops.PackPlan): W[i] = [q | k | v | skip] of convolution i
        with its bias row + 3 padding rows."""
        n = len(Ts)
        cin_p, cp = cin + (-cin) % 4, cout + (-cout) % 4
        w = torch.stack([t for T in Ts for t in (T[2], T[0], T[4], T[7])]).view(n, 4, cout, cin)           # (n, 4, cout, cin)
        w = nn.functional.pad(w.permute(0, 3, 1, 2), (0, cp - cout, 0, 0, 0, cin_p - cin), value=fill)     # (n, cin_p, 4, cp)
        b = torch.stack([t for T in Ts for t in (T[3], T[1], T[5], T[8])]).view(n, 1, 4, cout)
        b = nn.functional.pad(b, (0, cp - cout, 0, 0, 0, 3), value=fill)                                    # bias row + 3 padding rows
        W = torch.cat([w, b], dim=1).reshape(n, cin_p + 4, 4 * cp)
        We = nn.functional.pad(torch.stack([T[6] for T in Ts]), (0, 0, 0, cp - cout), value=fill)          # (n, cp, 2)
        return W, We

    @staticmethod
    def pack_many(convs):
        """[PackedConv] for a list of convolutions: proj_layout of the parameters themselves, one batched evaluation per shape."""
        return _pack_by_shape(convs, lambda c: (c.in_channels, c.out_channels), TransformerConv.proj_layout, PackedConv)

    def forward(self, x, edge_index, edge_weight=None, packed=None, return_attention_weights=None):
        """return_attention_weights=True (or PyG's positional flag in the `packed` slot): (out, (edge_index, alpha)) as PyG returns
        them, alpha (E', 1) over mesh.edge_index(self_loops=True), before dropout and DETACHED (PyG's alpha carries autograd).
        `out` is the same as without the flag."""
        packed, want = _attention_flag(packed, return_attention_weights)
        mesh = _need_mesh(edge_index, x)
        cin, cout = self.in_channels, self.out_channels
        cin_p, cp = cin + (-cin) % 4, cout + (-cout) % 4
        x = x[:, :cin] if x.shape[1] > cin_p else x
        if x.shape[1] < cin_p:
            x = nn.functional.pad(x, (0, cin_p - x.shape[1]))
        pc = packed if packed is not None else self.pack()
        proj = ops.cheb_poly(x, pc.W, mesh, 1, 1, acc=pc.acc if packed is not None else None)     # one GEMM: [q | k | v | skip]
        out = ops.attention(proj, pc.We, mesh, cout, self.dropout, self.training, pc.acc_e if packed is not None else None)
        out = out[:, :cout] if cp != cout else out
        return _attention_result(self, out, want, mesh, lambda: ops.attention_weights(proj, pc.We, mesh, cout))


@recompute.register_record
class PackedConv:
    """Packed weights of one attention convolution for one forward pass (+ the gradient accumulators of that pass)."""
    __slots__ = ('W', 'We', 'acc', 'acc_e')

    def __init__(self, W, We):
        self.W, self.We, self.acc, self.acc_e = W, We, ops.GradAcc(), ops.GradAcc()


def _pack_by_shape(convs, shape, layout, packed):
    """[packed(*matrices)] for a list of attention convolutions: `layout` (proj_layout and its like) evaluated on the parameters
    themselves with zero padding, once per shape(conv) for all convolutions of that shape; each convolution gets its views of the
    batched matrices (unbind: one stack in the backward, not a dozen launches per convolution -- 24+ convolutions per cell)."""
    out, groups = [None] * len(convs), {}
    for i, c in enumerate(convs):
        groups.setdefault(shape(c), []).append(i)
    for key, idxs in groups.items():
        mats = layout([convs[i].plan_params() for i in idxs], *key, 0.0)
        for i, *views in zip(idxs, *[m.unbind(0) for m in mats]):
            out[i] = packed(*views)
    return out


class MHTransformerConv(nn.Module):
    """The reference's MHTransformerConv (model/model.py:26-37): torch_geometric TransformerConv(in, out, heads, concat=True,
    beta=False, dropout, edge_dim=2, bias=True, root_weight=True) followed by lin = Linear(heads * out, out).  Parameters, in the
    reference's creation order: lin_key / lin_query / lin_value (.weight (heads out, in), .bias), lin_edge.weight (heads out, 2),
    lin_skip (.weight, .bias), lin (.weight (out, heads out), .bias).  One projection GEMM produces [q | k | v | skip] per head;
    the attention of all heads and the head merge run in one launch (ops.mh_attention)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True,
                 root_weight=True):
        super().__init__()
        assert concat and not beta and edge_dim == 2 and bias and root_weight, \
            'the reference uses concat=True, beta=False, edge_dim=2, bias=True, root_weight=True'
        if not (1 <= heads <= 4 and 1 <= out_channels <= 32):
            raise ValueError(f'MHTransformerConv(heads={heads}, out_channels={out_channels}): the HIP kernels take 1 .. 4 heads of '
                             'at most 32 channels')
        self.in_channels, self.out_channels, self.heads, self.dropout = in_channels, out_channels, heads, dropout
        hc = heads * out_channels
        self.lin_key = nn.Linear(in_channels, hc)
        self.lin_query = nn.Linear(in_channels, hc)
        self.lin_value = nn.Linear(in_channels, hc)
        self.lin_edge = nn.Linear(edge_dim, hc, bias=False)
        self.lin_skip = nn.Linear(in_channels, hc)
        self.lin = nn.Linear(hc, out_channels)
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_edge, self.lin_skip, self.lin):
            nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)

    def plan_params(self):
        """The parameters in module order (= the stand-ins _layout receives)."""
        return [self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias, self.lin_value.weight,
                self.lin_value.bias, self.lin_edge.weight, self.lin_skip.weight, self.lin_skip.bias, self.lin.weight, self.lin.bias]

    @staticmethod
    def _layout(Ts, cin, cout, H, fill):
        """(W (n, cin_p + 4, H 4 cp), We (n, H, cp, 2), Wt (n, H cp, cp), blin (n, cp)) of n convolutions of one shape from their
        plan_params() lists (data movement only, padding = `fill`, like TransformerConv.proj_layout): W[i] = [q | k | v | skip] of
        every head, head-major, with the bias row + 3 padding rows; Wt = lin.weight^T split by head.  Channels above out_channels
        (cp = out rounded up to 4) are padding everywhere, so the padding columns of cat and y stay zero."""
        n = len(Ts)
        cin_p, cp = cin + (-cin) % 4, cout + (-cout) % 4
        w = torch.stack([t for T in Ts for t in (T[2], T[0], T[4], T[7])]).view(n, 4, H, cout, cin)
        w = nn.functional.pad(w.permute(0, 4, 2, 1, 3), (0, cp - cout, 0, 0, 0, 0, 0, cin_p - cin), value=fill)  # (n, cin_p, H, 4, cp)
        b = torch.stack([t for T in Ts for t in (T[3], T[1], T[5], T[8])]).view(n, 4, H, cout).transpose(1, 2)
        b = nn.functional.pad(b, (0, cp - cout), value=fill).reshape(n, 1, H * 4 * cp)
        W = torch.cat([w.reshape(n, cin_p, H * 4 * cp), nn.functional.pad(b, (0, 0, 0, 3), value=fill)], dim=1)
        We = nn.functional.pad(torch.stack([T[6] for T in Ts]).view(n, H, cout, 2), (0, 0, 0, cp - cout), value=fill)
        Wt = torch.stack([T[9] for T in Ts]).view(n, cout, H, cout).permute(0, 2, 3, 1)                         # (n, H, c, o)
        Wt = nn.functional.pad(Wt, (0, cp - cout, 0, cp - cout), value=fill).reshape(n, H * cp, cp)
        bl = nn.functional.pad(torch.stack([T[10] for T in Ts]), (0, cp - cout), value=fill)
        return W, We, Wt, bl

    def pack(self):
        """The packed weights of one forward pass (see _layout) with the gradient accumulators all uses in the pass share."""
        return MHTransformerConv.pack_many([self])[0]

    @staticmethod
    def pack_many(convs):
        """[PackedMHConv] for a list of convolutions: _layout of the parameters themselves, one batched evaluation per shape."""
        return _pack_by_shape(convs, lambda c: (c.in_channels, c.out_channels, c.heads), MHTransformerConv._layout, PackedMHConv)

    def forward(self, x, edge_index, edge_weight=None, packed=None, return_attention_weights=None):
        """return_attention_weights=True (or PyG's positional flag in the `packed` slot): (y, (edge_index, alpha)), alpha (E', heads)
        over mesh.edge_index(self_loops=True), before dropout and detached (see TransformerConv.forward)."""
        packed, want = _attention_flag(packed, return_attention_weights)
        mesh = _need_mesh(edge_index, x)
        cin, cout = self.in_channels, self.out_channels
        cin_p, cp = cin + (-cin) % 4, cout + (-cout) % 4
        x = x[:, :cin] if x.shape[1] > cin_p else x
        if x.shape[1] < cin_p:
            x = nn.functional.pad(x, (0, cin_p - x.shape[1]))
        pc = packed if packed is not None else self.pack()
        proj = ops.cheb_poly(x, pc.W, mesh, 1, 1, acc=pc.acc if packed is not None else None)      # one GEMM: [q | k | v | skip] x H
        y = ops.mh_attention(proj, pc.We, pc.Wt, pc.bl, mesh, cout, self.heads, self.dropout, self.training,
                             pc.acc_e if packed is not None else None, pc.acc_l if packed is not None else None)
        y = y[:, :cout] if cp != cout else y
        # the H heads' rows side by side (head-major [q | k | v | skip]): groups 4 cp apart, blocks cp apart
        return _attention_result(self, y, want, mesh,
                                 lambda: ops.attention_weights(proj, pc.We, mesh, cout, self.heads, ps=cp, hs=4 * cp))


@recompute.register_record
class PackedMHConv:
    """Packed weights of one MHTransformerConv for one forward pass (+ the gradient accumulators of that pass)."""
    __slots__ = ('W', 'We', 'Wt', 'bl', 'acc', 'acc_e', 'acc_l')

    def __init__(self, W, We, Wt, bl):
        self.W, self.We, self.Wt, self.bl = W, We, Wt, bl
        self.acc, self.acc_e, self.acc_l = ops.GradAcc(), ops.GradAcc(), ops.GradAcc()


def _attention_flag(packed, flag):
    """(packed, return_attention_weights) of an attention convolution's call: a bool in the `packed` slot is PyG's positional
    return_attention_weights flag (conv(x, edge_index, edge_attr, True)), never packed weights."""
    if isinstance(packed, bool):
        if flag is not None:
            raise TypeError('return_attention_weights given twice: positionally (in the `packed` slot) and by keyword')
        return None, packed
    if flag is not None and not isinstance(flag, bool):
        raise TypeError(f'return_attention_weights must be a bool or None, not {type(flag).__name__}')
    return packed, bool(flag)


def _attention_result(conv, out, want, mesh, weights):
    """The return value of an attention convolution: `out`, or with the flag (out, (edge_index, alpha)).  weights() launches
    qt_attn_weights on the operands the forward just used; it also runs when a recording (Seq2Seq.record_attention) selects `conv`."""
    rec = _recorder()
    name = rec.name_of(conv) if rec is not None else None
    if not (want or name is not None):
        return out
    if name is not None:
        rec.check()
    pairs = ops.pyg_attention(mesh, *weights())
    if name is not None:
        rec.add(name, mesh, pairs)
    return (out, pairs) if want else out


class AttentionRecorder:
    """The state of one Seq2Seq.record_attention block: which convolutions to record (qualified module names, a predicate or all),
    and the records so far -- dicts with name, phase ('encoder' | 'decoder'), t (the step within the phase: the convolution's
    call count so far), mesh, edge_index (2, E') int64 and alpha (E', heads) float32, detached, in PyG's layout."""

    def __init__(self, model, select=None):
        self.model, self.records, self._calls = model, [], {}
        if select is None:
            pred = lambda n: True
        elif callable(select):
            pred = select
        else:
            names = set([select] if isinstance(select, str) else select)
            pred = names.__contains__
        self._names = {id(m): n for n, m in model.named_modules() if isinstance(m, (TransformerConv, MHTransformerConv)) and pred(n)}

    def name_of(self, conv):
        return self._names.get(id(conv))

    def names_of(self, convs):
        return [self._names.get(id(c)) for c in convs]

    def check(self):
        if getattr(self.model, 'static_shapes', False) or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError('attention weights cannot be recorded in static mode or inside a graph capture (make_graphed_step, '
                               'make_graphed_rollout, predict(use_graph=True)): the edge list needs a host read')

    def add(self, name, mesh, pairs):
        self.check()
        t = self._calls.get(name, 0)
        self._calls[name] = t + 1
        self.records.append(dict(name=name, phase=name.split('.')[0], t=t, mesh=mesh, edge_index=pairs[0], alpha=pairs[1]))


_RECORDER = [None]      # the open AttentionRecorder, or None: then no convolution launches anything for it


def _recorder():
    """The open AttentionRecorder for this call, or None; a recomputed step's replay is no call of its own (it records nothing)."""
    return None if recompute.replaying() else _RECORDER[0]


def _need_mesh(edge_index, *node_tensors):
    """The Mesh a module received in the reference's edge_index slot; node_tensors: (N, c) operands whose rows must be the mesh's
    nodes -- the kernels walk the mesh's rows and read these buffers unchecked."""
    if not isinstance(edge_index, Mesh):
        raise TypeError('pass the Mesh (graph_structure["mapping"]) where the reference passes edge_index: '
                        'the HIP path keeps adjacency and normalisation in the Mesh')
    for t in node_tensors:
        if t is not None and t.shape[0] != edge_index.N:
            raise ValueError(f'a node tensor of {t.shape[0]} rows for a mesh of {edge_index.N} nodes')
    return edge_index


CONVOLUTIONS = {
    'ChebConv': ChebConv,
    'GCNConv': GCNConv,
    'TransformerConv': TransformerConv,
    'MHTransformerConv': MHTransformerConv,
    'GATConv': None,
    'GATv2Conv': None,
    'Dummy': None,
}

CONVOLUTION_KWARGS = {
    'GCNConv': dict(add_self_loops=False),
    'TransformerConv': dict(heads=1, edge_dim=2, dropout=0.1, concat=False),
    'MHTransformerConv': dict(heads=3, edge_dim=2, dropout=0.1),
    'ChebConv': dict(K=3, normalization='sym', bias=True),
    'GATConv': dict(heads=1, edge_dim=2),
    'GATv2Conv': dict(heads=1, edge_dim=2),
    'Dummy': dict(),
}


def _conv_class(convolution_type):
    assert convolution_type in CONVOLUTIONS, f'unknown convolution {convolution_type}'
    cls = CONVOLUTIONS[convolution_type]
    if cls is None:
        raise NotImplementedError(f'{convolution_type} is not built yet on the HIP path (ChebConv is; SURVEY.md 8(f))')
    return cls


class GraphConv(nn.Module):
    """n stacked convolutions with no nonlinearity in between (model/model.py:59-97)."""

    def __init__(self, convolution_type, in_channels, out_channels, n_layers):
        super().__init__()
        self.convolution_type, self.n_layers = convolution_type, n_layers
        cls, kw = _conv_class(convolution_type), CONVOLUTION_KWARGS[convolution_type]
        chans = [in_channels] + [out_channels] * n_layers
        self.convolutions = nn.ModuleList([cls(a, b, **kw) for a, b in zip(chans[:-1], chans[1:])])

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=False):
        for conv in self.convolutions:
            x = conv(x, edge_index, edge_attr)
        return x


class GConvLSTM(nn.Module):
    """Peephole graph-LSTM (model/model.py:263-463); forward returns (O, H', C') like the reference (:463).

    All eight GraphConv stacks of the reference are evaluated by ONE Chebyshev pass over Z = [X | H]:
    the stacked convolutions are pre-composed in weight space (ops.compose_chebconvs) and the four
    gates share the recurrence T_k(L^) Z.
    """

    GATES = 'ifco'

    def __init__(self, in_channels, out_channels, n_conv_layers=1, convolution_type='GCNConv', name='GConvLSTM'):
        super().__init__()
        assert convolution_type in CONVOLUTIONS
        self.convolution_type, self.n_conv_layers, self.name = convolution_type, n_conv_layers, name
        self.in_channels, self.out_channels = in_channels, out_channels
        for g in self.GATES:        # creation order = the reference's state-dict order
            setattr(self, f'conv_x_{g}', GraphConv(convolution_type, in_channels, out_channels, n_conv_layers))
            setattr(self, f'conv_h_{g}', GraphConv(convolution_type, out_channels, out_channels, n_conv_layers))
            if g != 'c':
                setattr(self, f'w_c_{g}', nn.Parameter(torch.zeros(1, out_channels)))
            setattr(self, f'b_{g}', nn.Parameter(torch.zeros(1, out_channels)))

    # -- weight packing (once per forward pass): ONE set of layout functions, written with data-movement ops only, serves both the
    # gather of a whole model's parameters (ops.PackPlan over stand-ins) and direct evaluation on the parameters (ops.pack_direct)
    @property
    def is_series(self):
        """True when every convolution is a Chebyshev series (ChebConv, GCNConv): the stacks compose in weight space."""
        return hasattr(self.conv_x_i.convolutions[0], 'cheb_coeffs')

    @property
    def _layer_by_layer(self):
        """True when the eight TransformerConv stacks run layer by layer (ops.multi_conv); else attention stacks (MHTransformerConv
        ones always) run one convolution after another."""
        return _MULTI_CONV and self.out_channels % 4 == 0 and type(self.conv_x_i.convolutions[0]) is TransformerConv

    @property
    def plannable(self):
        return self._layer_by_layer or all(type(c) is ChebConv and c.bias is not None for c in self._convs())

    def _convs(self):
        """The convolutions in module order: branch (conv_x, conv_h), gate, layer."""
        return [c for br in ('conv_x', 'conv_h') for g in self.GATES for c in getattr(self, f'{br}_{g}').convolutions]

    def plan_params(self):
        """The parameters plan_layout reads, in module order (none of the convolutions that pack_from packs one by one)."""
        convs = self._convs() if self.is_series or self._layer_by_layer else []
        return [p for c in convs for p in c.plan_params()] + [self.w_c_i, self.w_c_f, self.w_c_o, self.b_i, self.b_f, self.b_c, self.b_o]

    def pack(self, in_pad=None, ln=None, variants=(True,)):
        """One PackedCell per requested variant (with_h True / False); the variants share the peephole / bias tensors and their
        gradient accumulator.  W: ((K*C + Ks_padded), 4h) for Z = [X (padded to in_pad) | H].  plan_layout evaluated on the
        parameters themselves; stacked series compose with torch ops, on the GPU as well."""
        outs = ops.pack_direct(self.plan_params(), lambda T, fill: self.plan_layout(T, fill, '', in_pad, variants))
        return self.pack_from(outs, '', in_pad, ln, variants, device_compose=False)

    def plan_layout(self, T, fill, prefix, in_pad=None, variants=(True,)):
        """Outputs (named with `prefix`) from plan_params() or stand-ins of them: wc (3, h), b (4, h) and
        - layer-by-layer attention stacks: M0x / M0h (1, cin_p + 4, 4 x 4C) and E0 (8, C, 2) for layer 0, M<l> (8, C + 4, 4C) and
          E<l> for the deeper layers -- stack g = head g in the order conv_x_{i,f,c,o}, conv_h_{i,f,c,o}.  Layer 0 has two input
          segments (X and H: the four stacks of a branch share their input, so their projections are ONE matrix with 4 x 4C
          columns), deeper layers one (head g reads column block g of the previous layer's output);
        - series, one conv layer per stack: the gate matrix W of every requested variant as (x-bias member, h-bias member) sums;
        - deeper series: the per-layer weight / bias stacks of both branches, which pack_from composes;
        - other attention stacks: nothing more (pack_from packs them per convolution)."""
        L, h = self.n_conv_layers, self.out_channels
        per = (len(T) - 7) // (8 * L)
        conv = lambda bi, gi, l: T[((bi * 4 + gi) * L + l) * per:((bi * 4 + gi) * L + l + 1) * per]
        out = {prefix + 'wc': torch.cat(T[-7:-4], dim=0), prefix + 'b': torch.cat(T[-4:], dim=0)}
        if self._layer_by_layer:
            for l in range(L):
                if l == 0:
                    Wes = []
                    for bi, br in enumerate('xh'):
                        W, We = TransformerConv.proj_layout([conv(bi, gi, 0) for gi in range(4)], self.in_channels if bi == 0 else h, h, fill)
                        out[f'{prefix}M0{br}'] = W.permute(1, 0, 2).reshape(1, W.shape[1], 4 * W.shape[2])
                        Wes.append(We)
                    out[prefix + 'E0'] = torch.cat(Wes, dim=0)
                else:
                    W, We = TransformerConv.proj_layout([conv(bi, gi, l) for bi in range(2) for gi in range(4)], h, h, fill)
                    out[f'{prefix}M{l}'], out[f'{prefix}E{l}'] = W, We
            return out
        if not self.is_series:
            return out
        cs = self._convs()

        def Wt(bi, l):       # (4, K, in, h)
            return torch.stack([cs[(bi * 4 + gi) * L + l].cheb_coeffs(conv(bi, gi, l)) for gi in range(4)])

        def Bs(bi, l):       # (4, h)
            return torch.stack([conv(bi, gi, l)[-1] for gi in range(4)])

        if L > 1:
            for bi, br in enumerate('xh'):
                for l in range(L):
                    out[f'{prefix}P{br}{l}'] = Wt(bi, l)
                    out[f'{prefix}B{br}{l}'] = Bs(bi, l)
            return out
        Px, Ph = Wt(0, 0), Wt(1, 0)
        cin = in_pad or self.in_channels
        if cin > self.in_channels:
            Px = nn.functional.pad(Px, (0, 0, 0, cin - self.in_channels), value=fill)
        rows = lambda bs: nn.functional.pad(bs.unsqueeze(1).permute(1, 0, 2).reshape(1, 4 * h), (0, 0, 0, 3), value=fill)
        for with_h in variants:
            M = torch.cat([Px, Ph], dim=2) if with_h else Px
            Wm = M.permute(1, 2, 0, 3).reshape(Px.shape[1] * M.shape[2], 4 * h)
            out[f'{prefix}W{int(with_h)}'] = (torch.cat([Wm, rows(Bs(0, 0))], dim=0),
                                              torch.cat([torch.full_like(Wm, fill), rows(Bs(1, 0))], dim=0))
        return out

    def pack_from(self, outs, prefix, in_pad=None, ln=None, variants=(True,), device_compose=True):
        """PackedCells from the outputs of plan_layout (same arguments), gathered by a plan or evaluated directly.  device_compose:
        stacked series whose matrices are on the GPU compose there, one launch per product (ops.compose_pack); False: with torch
        ops everywhere (ops.compose_chebconvs + _assemble, the reference implementation of that composition)."""
        L, h = self.n_conv_layers, self.out_channels
        wc, b = outs[prefix + 'wc'], outs[prefix + 'b']
        acc_p = ops.GradAcc()
        if not self.is_series:
            multi = convs = None
            if self._layer_by_layer:
                multi = [([outs[prefix + 'M0x'], outs[prefix + 'M0h']] if l == 0 else [outs[f'{prefix}M{l}']], outs[f'{prefix}E{l}'],
                          ops.GradAcc()) for l in range(L)]
            else:       # all convolutions of the cell packed together (pack_many), handed out per stack and layer
                packed = iter(type(self.conv_x_i.convolutions[0]).pack_many(self._convs()))
                convs = {f'{br}_{g}': [next(packed) for _ in range(L)] for br in ('conv_x', 'conv_h') for g in self.GATES}
            cells = [PackedCell(None, 0, 0, wc, b, ln, None, acc_p) for _ in variants]
            for c in cells:             # the variants share the packed convolutions (and their accumulators)
                c.multi, c.convs = multi, convs
            return cells
        if L == 1:
            K = self.conv_x_i.convolutions[0].K
            return [PackedCell(outs[f'{prefix}W{int(v)}'], K, 1, wc, b, ln, ops.GradAcc(), acc_p) for v in variants]
        if device_compose and wc.is_cuda:
            stacks = [[outs[f'{prefix}{n}{br}{l}'] for l in range(L)] for n, br in (('P', 'x'), ('B', 'x'), ('P', 'h'), ('B', 'h'))]
            Ws, WTs, Kc, Ksc = ops.compose_pack(*stacks, in_pad or self.in_channels, variants)
            cells = []
            for W, WT in zip(Ws, WTs):
                acc_w = ops.GradAcc()
                acc_w.wt['T'] = WT                   # the gate GEMM stages its weight chunk from the transpose
                cells.append(PackedCell(W, Kc, Ksc, wc, b, ln, acc_w, acc_p))
            return cells
        Px, bx = ops.compose_chebconvs([outs[f'{prefix}Px{l}'] for l in range(L)], [outs[f'{prefix}Bx{l}'] for l in range(L)])
        Ph, bh = ops.compose_chebconvs([outs[f'{prefix}Ph{l}'] for l in range(L)], [outs[f'{prefix}Bh{l}'] for l in range(L)])
        return self._assemble(Px, bx, Ph, bh, wc, b, in_pad, ln, variants, acc_p)

    def _assemble(self, Px, bx, Ph, bh, wc, b, in_pad, ln, variants, acc_p):
        h = self.out_channels
        cin = in_pad or self.in_channels
        if cin > self.in_channels:
            Px = nn.functional.pad(Px, (0, 0, 0, cin - self.in_channels))
        K, Ks = Px.shape[1], bx.shape[1]
        bias_rows = nn.functional.pad((bx + ops.unalias(bh)).permute(1, 0, 2).reshape(Ks, 4 * h), (0, 0, 0, (-Ks) % 4))
        out = []
        for with_h in variants:
            M = torch.cat([Px, Ph], dim=2) if with_h else Px           # (4, K, C, h)
            W = torch.cat([M.permute(1, 2, 0, 3).reshape(K * M.shape[2], 4 * h), bias_rows], dim=0)
            out.append(PackedCell(W, K, Ks, wc, b, ln, ops.GradAcc(), acc_p))
        return out

    def step(self, X, mesh, H, C, pk, alias_h=False, pass_x=False):
        """One cell update with packed weights `pk`; pk.ln = (4, h) LayerNorm parameters fused onto H', C' or None.
        alias_h / pass_x: return H' / X once more after (O, H', C') -- see ops.gate_cell."""
        if pk.W is None and (alias_h or pass_x):
            out = tuple(self.step(X, mesh, H, C, pk))
            return out + ((out[1],) if alias_h else ()) + ((X,) if pass_x else ())
        if pk.W is None and pk.multi is not None:
            Hz = H if H is not None else X.new_zeros(X.shape[0], self.out_channels)     # conv_h(0) is not 0 (biases)
            c0 = self.conv_x_i.convolutions[0]
            cin_p = c0.in_channels + (-c0.in_channels) % 4
            if X.shape[1] != cin_p:
                X = X[:, :c0.in_channels] if X.shape[1] > cin_p else X
                X = nn.functional.pad(X, (0, cin_p - X.shape[1])) if X.shape[1] < cin_p else X
            y, L = None, len(pk.multi)
            for l, (Ws, We, acc) in enumerate(pk.multi):
                segs = [(X, Ws[0]), (Hz, Ws[1])] if l == 0 else [(y, Ws[0])]
                y = ops.multi_conv(segs, We, mesh, self.out_channels, c0.dropout, self.training, acc, gmod=4 if l == L - 1 else 0,
                                   record=self._multi_record(l, mesh))
            return ops.lstm_cell(y, C, pk.wc, pk.b, pk.ln, mesh, pk.acc_p)
        if pk.W is None:
            Hz = H if H is not None else X.new_zeros(X.shape[0], self.out_channels)     # conv_h(0) is not 0 (biases)

            def stack(name, x):
                for conv, pc in zip(getattr(self, name).convolutions, pk.convs[name] if pk.convs else [None] * self.n_conv_layers):
                    x = conv(x, mesh, packed=pc) if pc is not None else conv(x, mesh)
                return x
            G = torch.cat([stack(f'conv_x_{g}', X) + stack(f'conv_h_{g}', Hz) for g in self.GATES], dim=1)
            return ops.lstm_cell(G, C, pk.wc, pk.b, pk.ln, mesh, pk.acc_p)
        return ops.gate_cell(X, H, pk.W, C, pk.wc, pk.b, pk.ln, mesh, pk.K, pk.Ks, pk.acc_w, pk.acc_p, alias_h, pass_x)

    def _multi_record(self, l, mesh):
        """The record(P, We) hook of ops.multi_conv for layer l while a recording selects any of its eight convolutions, else None:
        the weights launch reads the layer's projections P (G, 4, N, C) in place -- one launch for all eight stacks, or one per
        selected stack."""
        rec = _recorder()
        if rec is None:
            return None
        convs = [getattr(self, f'{br}_{g}').convolutions[l] for br in ('conv_x', 'conv_h') for g in self.GATES]
        names = rec.names_of(convs)
        if not any(names):
            return None
        h = self.out_channels

        def record(P, We):
            rec.check()
            G, _, N, C = P.shape
            if all(names):
                ae, as_ = ops.attention_weights(P, We, mesh, h, G, ld=C, ps=N * C, hs=4 * N * C)
                parts = [(n, ae[g:g + 1], as_[g:g + 1]) for g, n in enumerate(names)]
            else:
                parts = [(n, *ops.attention_weights(P[g], We[g], mesh, h, 1, ld=C, ps=N * C, hs=4 * N * C)) for g, n in enumerate(names) if n]
            for n, ae, as_ in parts:
                rec.add(n, mesh, ops.pyg_attention(mesh, ae, as_))
        return record

    def forward(self, X, edge_index, edge_weight=None, H=None, C=None):
        pad = (-X.shape[1]) % 4
        if pad:
            X = nn.functional.pad(X, (0, pad))
        return self.step(X, _need_mesh(edge_index, X, H, C), H, C, self.pack(X.shape[1], None, (H is not None,))[0])


@recompute.register_record
class PackedCell:
    """Packed weights of one GConvLSTM for one forward pass (+ the gradient accumulators of that pass)."""
    __slots__ = ('W', 'K', 'Ks', 'wc', 'b', 'ln', 'acc_w', 'acc_p', 'convs', 'multi')

    def __init__(self, W, K, Ks, wc, b, ln, acc_w, acc_p):
        self.W, self.K, self.Ks, self.wc, self.b, self.ln, self.acc_w, self.acc_p = W, K, Ks, wc, b, ln, acc_w, acc_p
        self.convs = None
        self.multi = None


def _not_built(name):
    class _Missing(nn.Module):
        def __init__(self, *a, **k):
            raise NotImplementedError(f'{name} is a non-default variant of the reference and is outside the '
                                      'hot path built here (SURVEY.md section 2)')
    _Missing.__name__ = name
    return _Missing


GConvGRU = _not_built('GConvGRU')
GConvLSTM_Simple = _not_built('GConvLSTM_Simple')
SplitGConvLSTM = _not_built('SplitGConvLSTM')
DummyLSTM = _not_built('DummyLSTM')
MPNNLSTM = _not_built('MPNNLSTM')
MPNNLSTMI = _not_built('MPNNLSTMI')
