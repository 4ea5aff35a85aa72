"""One update of the TransformerConv GConvLSTM cell restated in float64, written from the definitions: the checker of the composite
GConvLSTM.step -> ops.multi_conv -> ops.lstm_cell (tests only; plain torch / numpy on the CPU, it imports attn_f64 and nothing of
qtmpnn or model).

The eight convolution stacks run layer by layer.  Per layer the projections [q | k | v | skip] = x W^T + b of the eight stacks are
assembled as attention_f64's proj (N, 8 4C) in the head order conv_x_{i,f,c,o}, conv_h_{i,f,c,o} and ONE attention_f64 call with
heads = 8 and the layer's seed evaluates them, so head g draws dropout_mask(seed_l, epoch, g, i, j, keep).  Stack g of layer 0 reads
X (g < 4) or H; stack g of a deeper layer reads stack g's output of the layer below.  After the last layer conv_x + conv_h per
gate, then the peephole cell:

    I = sigmoid(g_i + w_c_i C + b_i)     F = sigmoid(g_f + w_c_f C + b_f)     T = tanh(g_c + b_c)
    C' = F C + I T                       O = sigmoid(g_o + w_c_o C' + b_o)    H' = O tanh(C')

and, where LayerNorm parameters ln (4, h) = (weight_h, bias_h, weight_c, bias_c) are given, layer_norm(H') and layer_norm(C') with
eps 1e-5.  Parameters by PyG's names, as oracle.qt_oracle.GConvLSTM's state dict lays them out; geometry as attention_f64 takes it
(rowptr, col, selfpair, eattr of the valid nodes).  tests/test_tcell_f64_host.py pins this to the oracle's cell."""
import re
from types import SimpleNamespace

import torch

from attn_f64 import attention_f64, gradients

GATES = 'ifco'
STACKS = [f'{br}_{g}' for br in ('conv_x', 'conv_h') for g in GATES]          # head order of every layer's launch


def leaves(state, dtype=torch.float64):
    """{name: leaf of `dtype` that requires a gradient} from a state dict."""
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}


def leaf(t, dtype=torch.float64, grad=True):
    return None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_(grad)


def n_layers(params):
    return 1 + max(int(m.group(1)) for m in (re.match(r'conv_x_i\.convolutions\.(\d+)\.', k) for k in params) if m)


class _Attention(torch.autograd.Function):
    """attention_f64 makes leaves of its operands; this carries its output and gradients into the surrounding graph."""

    @staticmethod
    def forward(ctx, proj, We, call):
        with torch.enable_grad():           # (autograd is off inside forward; the namespace keeps its own graph for backward)
            ctx.ref = call(proj.detach().numpy(), We.detach().numpy())
        return ctx.ref.out.detach().clone()

    @staticmethod
    def backward(ctx, g):
        gp, gw = gradients(ctx.ref, g.numpy())
        return gp, gw, None


def cell(params, geo, X, H, C, c_real, ln=None, keep=1.0, epoch=0, seeds=None, dtype=torch.float64):
    """One update.  params: leaves(); X (N, cin), H, C (N, h) or None (zero state), ln (4, h) or None: tensors of `dtype`, leaves or
    not; seeds: one per layer (needed when keep < 1).  -> namespace O, H, C (the new state, after LayerNorm where given), pre: the four
    gate pre-activations (i, f, c, o), detached; attn: attention_f64's namespace per layer (mult: the masks it drew).
    `dtype` = float32 runs the same statements in single precision."""
    L = n_layers(params)
    h = params['b_i'].shape[1]
    N = len(geo.rowptr) - 1
    assert X.shape[0] == N and X.dtype == dtype, (X.shape, N, X.dtype)
    seeds = [0] * L if seeds is None else list(seeds)
    assert len(seeds) == L
    Hz = torch.zeros(N, h, dtype=dtype) if H is None else H
    Cz = torch.zeros(N, h, dtype=dtype) if C is None else C
    y, attn = None, []
    for l in range(L):
        blocks = []
        for g, name in enumerate(STACKS):
            x = (X if g < 4 else Hz) if l == 0 else y[:, g]
            for lin in ('lin_query', 'lin_key', 'lin_value', 'lin_skip'):
                pre = f'{name}.convolutions.{l}.{lin}.'
                blocks.append(x @ params[pre + 'weight'].T + params[pre + 'bias'])
        proj = torch.cat(blocks, dim=1)                                                  # (N, 8 4C)
        We = torch.stack([params[f'{name}.convolutions.{l}.lin_edge.weight'] for name in STACKS])       # (8, C, 2)

        def call(p, w, seed=seeds[l]):
            attn.append(attention_f64(geo.rowptr, geo.col, geo.selfpair, geo.eattr, p, w, c_real, 8, keep, seed, epoch, dtype=dtype))
            return attn[-1]
        out = _Attention.apply(proj, We, call)
        y = out.view(N, 8, h)
    gate = y.view(N, 2, 4, h).sum(dim=1)                                                 # conv_x + conv_h per gate
    p = params
    pi = gate[:, 0] + p['w_c_i'] * Cz + p['b_i']
    pf = gate[:, 1] + p['w_c_f'] * Cz + p['b_f']
    pc = gate[:, 2] + p['b_c']
    Cn = torch.sigmoid(pf) * Cz + torch.sigmoid(pi) * torch.tanh(pc)
    po = gate[:, 3] + p['w_c_o'] * Cn + p['b_o']
    O = torch.sigmoid(po)
    Hn = O * torch.tanh(Cn)
    if ln is not None:
        Hn, Cn = layer_norms(Hn, Cn, ln)
    return SimpleNamespace(O=O, H=Hn, C=Cn, pre=tuple(t.detach() for t in (pi, pf, pc, po)), attn=attn)


def layer_norms(Hn, Cn, ln):
    """(layer_norm(H'), layer_norm(C')) with ln (4, h) = (weight_h, bias_h, weight_c, bias_c), eps 1e-5."""
    lnf, h = torch.nn.functional.layer_norm, Hn.shape[1]
    return lnf(Hn, (h,), ln[0], ln[1], 1e-5), lnf(Cn, (h,), ln[2], ln[3], 1e-5)


def steps(params, geo, Xs, H, C, c_real, ln=None, keep=1.0, epoch=0, seeds=None, dtype=torch.float64):
    """T chained updates: H', C' of update t (after LayerNorm where given) are the state of update t + 1, Xs[t] its input; seeds: one
    list (a seed per layer) per step.  -> the T namespaces of cell()."""
    out = []
    for t, X in enumerate(Xs):
        r = cell(params, geo, X, H, C, c_real, ln, keep, epoch, None if seeds is None else seeds[t], dtype)
        H, C = r.H, r.C
        out.append(r)
    return out
