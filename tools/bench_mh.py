"""Fused multi-head attention + head merge (qt_mhattn_fwd / qt_mhattn_bwd_merge) against the unfused composition (qt_attn_fwd /
qt_attn_bwd with G = 3 heads + a GEMM for the merge) at the cfg4 shapes: forward + backward, HIP events around graph replays of
`reps` calls each, the two variants alternated in one process after a warm-up.

    python tools/bench_mh.py [C ...]          (default: 32 = fc_out1 and the cells at hidden 32, 4 = fc_out2 with c_real 1)
Mesh: 16 ice-like 128x128 clips, land mask, transform_func, thresh 0.15 (BASELINE configs[3]).  Prints one JSON line per C.
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np, torch
from qtmpnn import ops, synthetic
from qtmpnn.mesh import build_mesh
dev = torch.device('cuda', 0)
shape, B, H = (128, 128), 16, 3
clips = [synthetic.make_ice_like(1000 + k, shape=shape, channels=5, n_frames=12)[0] for k in range(B)]
mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]
x = torch.from_numpy(np.stack(clips)).to(dev)
src = abs(abs(x[..., 0] - 0.5) - 0.5).amax(dim=1)
mesh = build_mesh(src=src, thresh=0.15, mask=mask)
N = mesh.N


def graphed(fn, reps):
    fn(); torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        for _ in range(reps):
            fn()
    gr.replay(); torch.cuda.synchronize()
    return gr


def timed(gr, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); gr.replay(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


for C in [int(a) for a in sys.argv[1:]] or [32, 4]:
    c_real = 1 if C == 4 else C
    torch.manual_seed(C)
    live = torch.zeros(C, device=dev); live[:c_real] = 1.0
    proj = ((torch.randn(N, H, 4, C, device=dev) * live).view(N, H * 4 * C)).requires_grad_(True)
    We = (torch.randn(H, C, 2, device=dev) * live.view(1, C, 1)).requires_grad_(True)
    Wt = (torch.randn(H, C, C, device=dev) * 0.2 * live.view(1, C, 1) * live.view(1, 1, C)).view(H * C, C).requires_grad_(True)
    bl = (torch.randn(C, device=dev) * live).requires_grad_(True)
    gy = torch.randn(N, C, device=dev) * live
    ins = [proj, We, Wt, bl]
    out = {}
    for keep in (1.0, 0.9):
        def fused():
            y = ops._MHAttention.apply(proj, We, Wt, bl, mesh, c_real, keep, 7, None, None, H)
            torch.autograd.grad(y, ins, gy)

        def unfused():
            y = ops._Attention.apply(proj, We, mesh, c_real, keep, 7, None, H, 0) @ Wt + bl
            torch.autograd.grad(y, ins, gy)

        def fused_fwd():
            with torch.no_grad():
                ops._MHAttention.apply(proj, We, Wt, bl, mesh, c_real, keep, 7, None, None, H)

        def unfused_fwd():
            with torch.no_grad():
                ops._Attention.apply(proj, We, mesh, c_real, keep, 7, None, H, 0) @ Wt + bl
        reps = 20
        gs = {k: graphed(f, reps) for k, f in (('fused', fused), ('unfused', unfused), ('fused_fwd', fused_fwd), ('unfused_fwd', unfused_fwd))}
        for k in gs:                       # warm-up replays
            timed(gs[k], reps)
        ts = {k: [] for k in gs}
        for _ in range(5):                 # alternated
            for k in gs:
                ts[k].append(timed(gs[k], reps))
        out[f'keep{keep}'] = {k + '_us': round(float(np.median(v)), 1) for k, v in ts.items()}
        out[f'keep{keep}']['spread_us'] = {k: round(float(max(v) - min(v)), 1) for k, v in ts.items()}
        del gs
    print(json.dumps({'N': N, 'E': mesh.E, 'heads': H, 'C': C, 'c_real': c_real, **out}))
