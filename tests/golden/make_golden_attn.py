#!/usr/bin/env python3
"""Generate tests/golden/attn_rollout.npz: the attention coefficients of every TransformerConv call of a rollout of the
reference's own Seq2Seq.

Needs the reference project, found the way make_golden.py finds it (the GPU tests read only the arrays written here):

    python tests/golden/make_golden_attn.py

As make_golden_mh.py: make_golden.py provides the stand-ins and the reference's model/ package; torch_geometric.nn.TransformerConv
is replaced -- here by tests/attn_restated.py's RecordingTransformerConv (the mh_restated.py restatement, recording alpha before
dropout in every call) -- and model.model / model.seq2seq are reloaded.  The Seq2Seq, its GConvLSTM cells, the decoder head and the
re-meshing are the reference's own code; eval() (no attention dropout).

The case: a 64 x 64 one-digit clip, convolution_type='TransformerConv', hidden 8, n_layers=1, n_conv_layers=2, 2 input and 2 output
steps (the second output step runs on a re-meshed frame).  Written: the rollout inputs (x, y, concat, mask) and the weights ('w/'),
and per record r: name_r (qualified module name), t_r (the index of that module's call), edges_r (2, E') int32 sorted like
Mesh.edge_index(self_loops=True)) and alpha_r (E', heads) in that order.  Only arrays are written.
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
import attn_restated                       # noqa: E402

sys.modules['torch_geometric.nn'].TransformerConv = attn_restated.RecordingTransformerConv
RM = importlib.reload(MG.RM)
RS = importlib.reload(MG.RS)
synthetic = MG.synthetic
assert RM.CONVOLUTIONS['TransformerConv'] is attn_restated.RecordingTransformerConv


def rollout_records():
    """(arrays of the fixture, records [(name, t, edges, alpha)])."""
    c = synthetic.make_clip(33, canvas=(64, 64), n_digits=1, n_frames=4, pixel_noise=0.0)
    x, y = c[:2], c[2:4].copy()
    concat = (y * 0.5).astype(np.float32)
    mask = np.zeros((64, 64), dtype=bool)
    model = RS.Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.1, input_timesteps=2, input_features=4, output_timesteps=2,
                       n_layers=1, n_conv_layers=2, convolution_type='TransformerConv')
    MG.randomize(model, 97, scale=0.4, bscale=0.0)
    model.eval()
    names = {id(m): n for n, m in model.named_modules()}
    log = attn_restated.RecordingTransformerConv.log = []
    try:
        with torch.no_grad():
            outs, maps = model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(concat), teacher_forcing_ratio=0, mask=mask)
    finally:
        attn_restated.RecordingTransformerConv.log = None
    calls, records = {}, []
    for r in log:
        name = names[id(r['module'])]
        t = calls.get(name, 0)
        calls[name] = t + 1
        ei = r['edge_index'].numpy()
        order = np.lexsort((ei[1], ei[0]))
        records.append((name, t, ei[:, order].astype(np.int32), r['alpha'].numpy()[order].astype(np.float32)))
    out = dict(x=x, y=y, concat=concat, mask=mask)
    for i, o in enumerate(outs):
        out[f'out_{i}'] = o.detach().numpy()
    out.update(MG.state_arrays(model, 'w/'))
    return out, records, [len(o) for o in outs]


def main():
    out, records, sizes = rollout_records()
    out['n_records'] = np.int64(len(records))
    for i, (name, t, edges, alpha) in enumerate(records):
        out[f'name_{i}'], out[f't_{i}'], out[f'edges_{i}'], out[f'alpha_{i}'] = np.array(name), np.int64(t), edges, alpha
    path = os.path.join(HERE, 'attn_rollout.npz')
    np.savez_compressed(path, **out)
    print('attn rollout: N per output step', sizes, 'records', len(records), 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(4)
    main()
