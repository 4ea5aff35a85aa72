#!/usr/bin/env python3
"""Generate the MHTransformerConv fixtures tests/golden/mh_{conv,cell,rollout}.npz by EXECUTING the reference's own modules.

Needs the reference project, found the way make_golden.py finds it (the GPU tests read only the arrays written here):

    python tests/golden/make_golden_mh.py

make_golden.py provides the stand-ins of the third-party modules and imports the reference's model/ package.  Its
torch_geometric.nn.TransformerConv stand-in (oracle/qt_oracle.py) is built for heads=1 only; here it is replaced by
tests/mh_restated.py (any heads / concat, PyG 2.2.0 restated: parity with PyG itself unpinned) and the reference's
model.model / model.seq2seq are reloaded, so that their MHTransformerConv subclasses the restatement.  Everything around the
convolution arithmetic -- MHTransformerConv's head merge, GConvLSTM, Encoder / Decoder, Seq2Seq, the re-meshing -- is the
reference's own code.  eval(): attention dropout off (it cannot be RNG matched).  Only arrays are written.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                   # noqa: E402  (stand-ins + the reference's modules)
import mh_restated                         # noqa: E402

sys.modules['torch_geometric.nn'].TransformerConv = mh_restated.TransformerConv
RM = importlib.reload(MG.RM)
RS = importlib.reload(MG.RS)
RG, RU, synthetic = MG.RG, MG.RU, MG.synthetic
assert issubclass(RM.MHTransformerConv, mh_restated.TransformerConv)

KW = RM.CONVOLUTION_KWARGS['MHTransformerConv']


def mesh_64():
    """The quadtree of transformer_cell.npz's frame: labels, sorted edges / [angle, dist] and the reference's own edge arrays."""
    c = synthetic.make_clip(33, canvas=(64, 64), n_digits=1, n_frames=1, pixel_noise=0.0)
    g = RG.image_to_graph(RU.add_positional_encoding(torch.from_numpy(c)), thresh=0.1, use_edge_attrs=True)
    ei, ea = g['edge_index'], g['edge_attrs']
    labels = g['mapping'].numpy().argmax(0).reshape(64, 64).astype(np.int32)
    sei, sea = MG.sort_edges(ei, ea)
    return ei, ea, g['data'].shape[1], dict(labels=labels, edges=sei, attrs=sea)


def conv_case():
    """One MHTransformerConv(6, 8) and one (8, 1) (the decoder's fc_out2 shape): inputs, outputs, input and parameter gradients."""
    ei, ea, n, out = mesh_64()
    gen = torch.Generator().manual_seed(11)
    for name, cin, cout, seed in (('a', 6, 8, 120), ('b', 8, 1, 121)):
        conv = RM.MHTransformerConv(cin, cout, **KW)
        MG.randomize(conv, seed, scale=0.4, bscale=0.2)
        conv.eval()
        x = torch.randn(n, cin, generator=gen).requires_grad_(True)
        y = conv(x, ei, ea)
        gy = torch.randn(n, cout, generator=gen)
        grads = torch.autograd.grad(y, [x] + list(conv.parameters()), gy)
        out.update({f'{name}/x': x.detach().numpy(), f'{name}/y': y.detach().numpy(), f'{name}/gy': gy.numpy(),
                    f'{name}/gx': grads[0].numpy()})
        out.update(MG.state_arrays(conv, f'{name}/w/'))
        for (k, _), gr in zip(conv.named_parameters(), grads[1:]):
            out[f'{name}/g/{k}'] = gr.numpy()
    np.savez_compressed(os.path.join(HERE, 'mh_conv.npz'), **out)
    print('mh conv N =', n, 'E =', out['edges'].shape[1])


def cell_case():
    """GConvLSTM(4, 8, n_conv_layers=2, 'MHTransformerConv'), laid out like transformer_cell.npz."""
    ei, ea, n, out = mesh_64()
    gen = torch.Generator().manual_seed(6)
    cell = RM.GConvLSTM(4, 8, n_conv_layers=2, convolution_type='MHTransformerConv')
    MG.randomize(cell, 90)
    cell.eval()
    X = torch.randn(n, 4, generator=gen).requires_grad_(True)
    H = torch.randn(n, 8, generator=gen).requires_grad_(True)
    C = torch.randn(n, 8, generator=gen).requires_grad_(True)
    Oo, Hn, Cn = cell(X, ei, ea, H, C)
    gO, gH, gC = (torch.randn(n, 8, generator=gen) for _ in range(3))
    grads = torch.autograd.grad([Oo, Hn, Cn], [X, H, C] + list(cell.parameters()), [gO, gH, gC])
    out.update(X=X.detach().numpy(), H=H.detach().numpy(), C=C.detach().numpy(), O=Oo.detach().numpy(),
               Hn=Hn.detach().numpy(), Cn=Cn.detach().numpy(), gO=gO.numpy(), gH=gH.numpy(), gC=gC.numpy(),
               gX=grads[0].numpy(), gHin=grads[1].numpy(), gCin=grads[2].numpy())
    out.update(MG.state_arrays(cell, 'w/'))
    for (k, _), gr in zip(cell.named_parameters(), grads[3:]):
        out['g/' + k] = gr.numpy()
    np.savez_compressed(os.path.join(HERE, 'mh_cell.npz'), **out)
    print('mh cell N =', n)


def rollout_case():
    """Masked ice-like Seq2Seq (hidden 8, one layer, two conv layers, 2 -> 3 steps): outputs, loss, every gradient, the mesh
    labels of every step and the reference's state-dict keys."""
    f, m = synthetic.make_ice_like(23, shape=(64, 64), channels=3, n_frames=5)
    x, y = f[:2], f[2:5, ..., :1].copy()
    concat = y * 0.5
    model = RS.Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.15, input_timesteps=2, input_features=6, output_timesteps=3,
                       n_layers=1, n_conv_layers=2, transform_func=MG.dist_from_05, convolution_type='MHTransformerConv')
    MG.randomize(model, 93, scale=0.1, bscale=0.05)
    model.eval()
    xt, yt, ct, mk = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(concat), torch.from_numpy(m)
    labels = []
    orig = RS.image_to_graph

    def spy(img, *a, **k):
        g = orig(img, *a, **k)
        mp = g['mapping'].numpy()
        labels.append(np.where(mp.sum(0) > 0, mp.argmax(0), -1).reshape(img.shape[1:3]).astype(np.int32))
        return g
    RS.image_to_graph = spy
    try:
        outs, maps = model(xt, yt, ct, teacher_forcing_ratio=0, mask=m)
    finally:
        RS.image_to_graph = orig
    y_hat = torch.stack([RG.unflatten(outs[i], maps[i], (64, 64), m) for i in range(3)])
    loss = torch.nn.MSELoss()(y_hat[:, ~mk], yt[:, ~mk])
    loss.backward()
    sd = model.state_dict()
    out = dict(x=x, y=y, concat=concat, mask=m, loss=np.float64(loss.item()), keys=np.array(list(sd.keys())),
               shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64))
    for i, lab in enumerate(labels):
        out[f'labels_{i}'] = lab
    for i, o in enumerate(outs):
        out[f'out_{i}'] = o.detach().numpy()
    out.update(MG.state_arrays(model, 'w/'))
    for k, p in model.named_parameters():
        out['g/' + k] = p.grad.numpy() if p.grad is not None else np.zeros(p.shape, np.float32)
    np.savez_compressed(os.path.join(HERE, 'mh_rollout.npz'), **out)
    print('mh rollout loss', loss.item(), 'N', [len(o) for o in outs], 'meshes', len(labels))


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(4)
    conv_case()
    cell_case()
    rollout_case()
    print('golden vectors written to', HERE)
