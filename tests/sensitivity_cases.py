"""The cases of tests/test_gpu_sensitivity.py and their yardstick: the float64 oracle (oracle.qt_oracle.Seq2Seq on the CPU, the
same weights, the same meshes) with J_t formed on its outputs and the maps taken by torch.autograd.grad with respect to its
input.  The oracle's flatten is an index_add and its unflatten an index_select, so the maps pass through the pooling of the
frames and, on data-driven meshes, through the state transfer between meshes, with the label maps held fixed.

Shapes (the smallest with several quadtree levels, a mask and two clips): 32 x 32 frames, T_in = 3, T_out = 2, hidden 8,
dropout 0, eval mode, B = 2 different clips.  Run with dtype=torch.float32 the same code is the honest float32 evaluation whose
distance to float64 the GPU's distance is measured beside (profiles/sensitivity.txt)."""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SHAPE, T_IN, T_OUT, HIDDEN, B = (32, 32), 3, 2, 8, 2
RTOL, REL_ATOL = 1e-4, 5e-5          # tests/helpers.py::grad_close, floor 0: per (clip, lead) map


def land_mask():
    mask = np.zeros(SHAPE, dtype=bool)
    mask[22:, :10] = True
    return mask


def high_interest():
    hir = np.zeros(SHAPE, dtype=bool)
    hir[4:7, 20:25] = True
    return hir


def region_target():
    w = np.zeros(SHAPE, np.float32)
    w[8:20, 12:28] = 1.0
    return w


CASES = {
    # name: convolution, input channels, layers, conv layers, mesh ('preset' | 'pixel' | 'data'), thresh
    'cheb_preset': dict(conv='ChebConv', cin=1, nl=2, nc=2, mesh='preset', thresh=-np.inf),
    'gcn_pixel': dict(conv='GCNConv', cin=4, nl=2, nc=2, mesh='pixel', thresh=-np.inf),
    'transformer_preset': dict(conv='TransformerConv', cin=1, nl=1, nc=2, mesh='preset', thresh=-np.inf),
    'mh_preset': dict(conv='MHTransformerConv', cin=1, nl=1, nc=2, mesh='preset', thresh=-np.inf, heads=2),
    'cheb_data': dict(conv='ChebConv', cin=1, nl=2, nc=2, mesh='data', thresh=0.1),
}


def inputs(case):
    """x (B, T_in, W, H, cin), concat (B, T_out, W, H, 1) float32: two different clips; further channels are noise."""
    from qtmpnn import synthetic
    c = CASES[case]
    noise = 0.0 if c['mesh'] == 'data' else 0.02        # (data-driven meshes: flat background, so no cell sits at the threshold)
    clips = [synthetic.make_clip(900 + 7 * b, canvas=SHAPE, digit=(12, 12), n_digits=1, n_frames=T_IN, pixel_noise=noise)
             for b in range(B)]
    rng = np.random.default_rng(12)
    x = np.stack(clips).astype(np.float32)
    if c['cin'] > 1:
        x = np.concatenate([x, rng.random((B, T_IN, *SHAPE, c['cin'] - 1)).astype(np.float32)], axis=-1)
    concat = (0.2 * rng.random((B, T_OUT, *SHAPE, 1))).astype(np.float32)
    return x, concat


class OracleMHTransformerConv(nn.Module):
    """The reference's MHTransformerConv (model/model.py:26-37) on the oracle's restated PyG TransformerConv: heads H, concat,
    root weight, then lin.  Head g reads rows [g C, (g + 1) C) of every projection, as PyG's view(-1, H, C) does."""

    def __init__(self, in_channels, out_channels, heads=1, edge_dim=2, dropout=0.0):
        super().__init__()
        hc = heads * out_channels
        self.heads, self.out_channels = heads, out_channels
        self.lin_key, self.lin_query, self.lin_value = (nn.Linear(in_channels, hc) for _ in range(3))
        self.lin_edge = nn.Linear(edge_dim, hc, bias=False)
        self.lin_skip = nn.Linear(in_channels, hc)
        self.lin = nn.Linear(hc, out_channels)

    def forward(self, x, edge_index, edge_attr=None):
        from oracle import qt_oracle as O
        C, outs = self.out_channels, []
        full = dict(self.named_parameters())
        for g in range(self.heads):
            p = {k: v[g * C:(g + 1) * C] for k, v in full.items() if not k.startswith('lin.')}
            outs.append(O.transformer_conv(x, edge_index, edge_attr, p, 0.0, False))
        return F.linear(torch.cat(outs, dim=-1), self.lin.weight, self.lin.bias)


def oracle_model(case, monkeypatch=None):
    """The float64-to-be oracle with perturbed weights (still float32: the product loads exactly these values)."""
    from oracle import qt_oracle as O
    c = CASES[case]
    if c['conv'] == 'MHTransformerConv':
        monkeypatch.setitem(O.CONVS, 'MHTransformerConv', (OracleMHTransformerConv, dict(heads=c['heads'], edge_dim=2, dropout=0.1)))
    torch.manual_seed(5)
    ref = O.Seq2Seq(HIDDEN, 0.0, c['thresh'], input_timesteps=T_IN, input_features=c['cin'] + 3, output_timesteps=T_OUT,
                    n_layers=c['nl'], n_conv_layers=c['nc'], convolution_type=c['conv'])
    ref.use_edge_attrs = c['conv'] in ('TransformerConv', 'MHTransformerConv')
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return ref.eval()


def functional(out, labels, w, dtype):
    """J_t of one clip on the oracle's side: the output un-flattened through the step's labels, weighted mean over w."""
    from oracle import qt_oracle as O
    frame = O.unflatten(out, labels, SHAPE)[..., 0]
    wt = torch.as_tensor(w, dtype=dtype)
    return (frame * wt).sum() / wt.sum()


def weights_of(target, mask):
    w = np.ones(SHAPE, np.float32) if target is None else np.array(target, np.float32)
    if mask is not None:
        w[mask] = 0.0
    return w


def oracle_run(ref, clip, concat, w, leads, dtype, mask, hir, gsr):
    """One clip through the oracle in `dtype` -> (J (L,), maps (L, T_in, W, H, C), label maps of every step)."""
    model = copy.deepcopy(ref).to(dtype).eval()
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)               # (the oracle's zero states and constants follow the default dtype)
    try:
        x = torch.from_numpy(np.ascontiguousarray(clip)).to(dtype).requires_grad_(True)
        g = None if gsr is None else {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in gsr.items()}
        outs, maps, _ = model(x, torch.from_numpy(concat).to(dtype), mask=mask, high_interest_region=hir, graph_structure=g)
        Js = [functional(outs[t], maps[t], w, dtype) for t in leads]
        grads = [torch.autograd.grad(J, x, retain_graph=True)[0] for J in Js]
    finally:
        torch.set_default_dtype(old)
    return (np.array([float(J.detach()) for J in Js]), np.stack([g.detach().double().numpy() for g in grads]),
            [np.asarray(m) for m in maps])


def oracle_gradient(ref, x, concat, w, leads, dtype, mask, hir, gsr):
    """All clips -> (J (B, L), maps (B, L, T_in, W, H, C) float64, labels [clip][step])."""
    runs = [oracle_run(ref, x[b], concat[b], w, leads, dtype, mask, hir, gsr) for b in range(x.shape[0])]
    return np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), [r[2] for r in runs]


def path_points(x, base, steps):
    """The clips of the integrated-gradients path in float32, as the product forms them: base + alpha_k (x - base) with
    alpha_k = (k + 1/2) / steps; (B, steps, T_in, W, H, C)."""
    alphas = ((np.arange(steps, dtype=np.float32) + np.float32(0.5)) / np.float32(steps)).astype(np.float32)
    delta = (x - base).astype(np.float32)
    return (base[:, None] + alphas[None, :, None, None, None, None] * delta[:, None]).astype(np.float32)


def oracle_integrated(ref, x, base, concat, w, leads, steps, dtype, mask, hir, gsr):
    """Integrated gradients at the product's midpoints -> (J, J_baseline (B, L), maps (B, L, ...) float64, residual (B, L)):
    the mean of the oracle's gradients over the path points times (x - base); the residual is the oracle's own
    sum(maps) - (J - J_baseline), the midpoint rule's error at `steps` points."""
    pts = path_points(x, base, steps)
    Bn = x.shape[0]
    J = oracle_gradient(ref, x, concat, w, leads, dtype, mask, hir, gsr)[0]
    Jb = oracle_gradient(ref, base, concat, w, leads, dtype, mask, hir, gsr)[0]
    grads = np.stack([oracle_gradient(ref, pts[:, k], concat, w, leads, dtype, mask, hir, gsr)[1] for k in range(steps)])
    maps = grads.mean(axis=0) * (x.astype(np.float64) - base.astype(np.float64))[:, None]
    return J, Jb, maps, maps.reshape(Bn, len(leads), -1).sum(axis=2) - (J - Jb)


def distance(got, ref):
    """The two figures of a comparison of maps (B, L, ...): the worst |got - ref| over a (clip, lead) map relative to that map's
    largest entry, and the worst ratio of |got - ref| to grad_close's bound (RTOL |ref| + REL_ATOL max|ref|; <= 1 passes)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rel = ratio = 0.0
    for b in range(ref.shape[0]):
        for l in range(ref.shape[1]):
            d, r = np.abs(got[b, l] - ref[b, l]), np.abs(ref[b, l])
            rel = max(rel, float(d.max() / r.max()))
            ratio = max(ratio, float((d / (RTOL * r + REL_ATOL * r.max())).max()))
    return rel, ratio
