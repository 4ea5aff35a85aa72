"""Time qt_attn_weights against qt_attn_fwd at the cfg4t shape (diagnostics; profiles/attn_weights.txt).

    python tools/bench_attn_weights.py [C] [G] [reps]
Mesh: 16 ice-like 128x128 clips, land mask, transform_func, thresh 0.15 (tools/bench_configs.py cfg4t); G = 8 groups in the (G, 4, N, C)
planes of a cell layer's projections (ops.multi_conv), as the recording path reads them.  Each launch runs `reps` times, eagerly, one
after the other: run it under `rocprofv3 --kernel-trace --stats` for per-kernel times; the event times printed here include the gaps.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np, torch
from qtmpnn import _lib, synthetic
from qtmpnn._lib import ptr
from qtmpnn.mesh import build_mesh
dev = torch.device('cuda', 0)
C = int(sys.argv[1]) if len(sys.argv) > 1 else 32
G = int(sys.argv[2]) if len(sys.argv) > 2 else 8
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
shape, B = (128, 128), 16
clips = [synthetic.make_ice_like(1000 + k, shape=shape, channels=5, n_frames=12)[0] for k in range(B)]
mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]
x = torch.from_numpy(np.stack(clips)).to(dev)
src = abs(abs(x[..., 0] - 0.5) - 0.5).amax(dim=1)
mesh = build_mesh(src=src, thresh=0.15, mask=mask)
N, E = mesh.N, mesh.E
xy, selfpair, eattr, rev = mesh.attn_geometry()
print('N', N, 'E', E, 'self pairs', int((selfpair > 0).sum()) if selfpair is not None else 0, 'C', C, 'G', G)
P = torch.randn(G, 4, N, C, device=dev)
We = torch.randn(G, C, 2, device=dev) * 0.1
out = torch.empty(G, N, C, device=dev)
stats = torch.empty(G, N, 2, device=dev)
ae, as_ = torch.empty(G, rev.numel(), device=dev), torch.empty(G, N, device=dev)
fwd = lambda: _lib.call('qt_attn_fwd', ptr(mesh.rowptr), ptr(mesh.col), ptr(xy), ptr(eattr), ptr(selfpair), ptr(P), C, ptr(We), C, C, N,
                        ptr(mesh.n_dev), 1.0, 7, None, ptr(out), ptr(stats), G, C, N * C, 4 * N * C, N * C)
wts = lambda: _lib.call('qt_attn_weights', ptr(mesh.rowptr), ptr(mesh.col), ptr(eattr), ptr(selfpair), ptr(P), C, N * C, 4 * N * C, ptr(We),
                        C, C, G, N, ptr(mesh.n_dev), ptr(rev), rev.numel(), ptr(ae), ptr(as_))


def timeit(fn):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


tf, tw = timeit(fwd), timeit(wts)
# bytes: forward reads q, skip per node and k, v per edge, writes out + stats; weights reads q per node and k per edge twice (two passes)
# and writes E + N floats
print(f'qt_attn_fwd     {tf:8.1f} us per launch (event time, {reps} eager launches)')
print(f'qt_attn_weights {tw:8.1f} us per launch  ratio {tw / tf:.2f}')
s = ae.view(G, -1)[:, :E].sum() + as_.sum()
print('check: sum of all coefficients', float(s), 'expected', G * int(mesh.n_valid))
