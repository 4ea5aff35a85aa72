"""Fractions Skill Score of a loader of single clips, ms per clip, four ways (configurations of tools/bench_score.py):
    (a) predict(use_graph=True), then the same five sums per scale in numpy on the host from the returned frames (what a user
        did before fss(): indicator fields, window counts by 2-D cumulative sums)
    (b) fss(use_graph=False)
    (c) fss(use_graph=True)
    (d) reliability(use_graph=True) on the same loader: the same loop with a per-pixel product, so (c) - (d) is what the
        neighbourhood launch adds over a per-pixel one
    python tools/bench_fss.py mnist|ice [--repeats R] [--commit TEXT]
Every repeat times all four over the whole loader (a graphed call includes its captures); the order a b c d / d c b a alternates
between repeats.  One untimed call of each comes first.  Prints the median and the spread of the repeats, and how much of (a) is
the numpy pass.  The default scales (1, 3, 5, 9, 17, 33).
    python tools/bench_fss.py kernel
times the launch alone: ops.rollout_fss on 16 steps of a 128 x 128 pixelwise frame, one clip, three sources, per set of scales
-- (1,) is the patch load (halo gathers, ballots) with next to no window work, the others add their window sums -- beside
ops.rollout_reliability and ops.rollout_scores on the same operands.  Each call is captured 20 times into one hipGraph, so that
the host side of the op is not in the figure; device events around 10 replays, 5 rounds of all calls in turn."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from torch.utils.data import DataLoader

from helpers import TinyIceDataset, TinyMovingMNISTDataset
from model.mpnnlstm import NextFramePredictorS2S
from qtmpnn import synthetic

dev = torch.device('cuda', 0)
kind = sys.argv[1] if len(sys.argv) > 1 else 'mnist'
repeats = int(sys.argv[sys.argv.index('--repeats') + 1]) if '--repeats' in sys.argv else 6
commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
THR = 0.15
SCALES = (1, 3, 5, 9, 17, 33)


def kernel_times():
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    n = m = 128
    T = 16
    g = torch.Generator(device='cpu').manual_seed(0)
    mesh = build_pixel_mesh(1, n, m, None, dev)
    outs = [torch.rand(n * m, 4, generator=g).to(dev) for _ in range(T)]
    y, clim, pers = (torch.rand(*shape, generator=g).to(dev) for shape in ((1, T, n * m), (1, T, n * m), (1, n * m)))
    kw = dict(persistence=pers, climatology=clim)
    calls = {f'rollout_fss scales {sc}': (lambda sc=sc: ops.rollout_fss(outs, [mesh] * T, y, 0.5, sc, per_tile=True, **kw))
             for sc in ((1,), (3,), (9,), (33,), SCALES)}
    calls['rollout_reliability 10 bins'] = lambda: ops.rollout_reliability(outs, [mesh] * T, y, 0.5, 10, per_tile=True, **kw)
    calls['rollout_scores'] = lambda: ops.rollout_scores(outs, [mesh] * T, y, 0.5, per_tile=True, **kw)
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for k, f in calls.items():
        f()                                                # untimed: code object, allocator
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k], stream=side):
            keep.append([f() for _ in range(20)])
    us = {k: [] for k in calls}
    for r in range(5):                                     # rounds of all calls, in turn
        for k, graph in graphs.items():
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / 200)
    print(f'kernel: one launch of {T} steps, {n} x {m} pixelwise, 1 clip, 3 sources; us per launch inside a replayed graph, '
          f'median (min-max) of 5 rounds of 200')
    for k, v in us.items():
        print(f'kernel: {k:<44} {np.median(v):7.1f} ({min(v):.1f}-{max(v):.1f})')


def build():
    torch.manual_seed(0)
    if kind == 'mnist':
        ds = TinyMovingMNISTDataset(16, 10, 10, n_digits=1, canvas_size=(64, 64), digit_size=(28, 28))
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=10, output_timesteps=10, device=dev,
                                    model_kwargs=dict(hidden_size=16, dropout=0.1, n_layers=2))
        return ds, nfp, None, None
    ds = TinyIceDataset(4, 10, 90, (128, 128), channels=5)
    mask = synthetic.make_ice_like(40, shape=(128, 128), channels=5, n_frames=2)[1]
    d = np.arange(365, dtype=np.float32)[:, None, None]
    base = ds.y[:, 0, ..., 0].mean(0)
    clim = torch.from_numpy((base[None] * (0.5 + 0.5 * np.cos(2 * np.pi * d / 365.0)))[None].astype(np.float32)).to(dev)
    tf = lambda a: abs(abs(a - 0.5) - 0.5)
    nfp = NextFramePredictorS2S(thresh=-np.inf, decompose=False, input_features=5, input_timesteps=10, output_timesteps=90,
                                device=dev, transform_func=tf,
                                model_kwargs=dict(hidden_size=32, dropout=0.1, n_layers=1, n_conv_layers=3,
                                                  convolution_type='TransformerConv', transform_func=tf))
    return ds, nfp, mask, clim


def box(ind, n):
    """(..., W, H) int64 -> sums over the n x n window around every pixel, zero outside the frame."""
    h = n // 2
    W, H = ind.shape[-2:]
    cs = np.zeros(ind.shape[:-2] + (W + 2 * h + 1, H + 2 * h + 1), dtype=np.int64)
    cs[..., h + 1:h + 1 + W, h + 1:h + 1 + H] = ind
    cs = cs.cumsum(axis=-2).cumsum(axis=-1)
    return cs[..., n:n + W, n:n + H] - cs[..., :W, n:n + H] - cs[..., n:n + W, :H] + cs[..., :W, :H]


def host_sums(field, io, keep):
    """(n, T, K, 5) int64 from (n, T, W, H) fp32 fields: qt_fss_rollout's five sums per scale over the pixels of `keep`."""
    with np.errstate(invalid='ignore'):
        i_s = (keep & (field > np.float32(THR))).astype(np.int64)
    out = np.zeros(field.shape[:2] + (len(SCALES), 5), dtype=np.int64)
    out[..., 0], out[..., 1] = keep.sum(), io.sum(axis=(-2, -1))[..., None]
    for k, n in enumerate(SCALES):
        cs, co = box(i_s, n)[:, :, keep], box(io, n)[:, :, keep]
        out[:, :, k, 2], out[:, :, k, 3], out[:, :, k, 4] = ((cs - co) ** 2).sum(-1), (cs * cs).sum(-1), (co * co).sum(-1)
    return out


if kind == 'kernel':
    kernel_times()
    sys.exit(0)
ds, nfp, mask, clim = build()
nfp.model.eval()
loader = DataLoader(ds, batch_size=1, shuffle=False)
n, T = len(ds), nfp.output_timesteps
keep = np.ones(tuple(ds.image_shape), bool) if mask is None else ~np.asarray(mask, bool)
truth = np.asarray(ds.y)[..., 0].astype(np.float32)
persistence = np.repeat(np.asarray(ds.x)[:, -1:, ..., 0], T, axis=1)
clim_fields = None
if clim is not None:
    clim_fields = np.stack([nfp.get_climatology_array(clim, torch.tensor([d])).cpu().numpy()[..., 0] for d in ds.launch_dates])


host_ms = []          # (a)'s numpy part alone, per clip


def way_a():
    frames = nfp.predict(loader, clim, mask=mask, use_graph=True)[..., 0]
    t0 = time.perf_counter()
    out = a_host(frames)
    host_ms.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def a_host(frames):
    io = (keep & (truth > np.float32(THR))).astype(np.int64)
    srcs = [frames, persistence] + ([clim_fields] if clim_fields is not None else [])
    return np.stack([host_sums(f, io, keep) for f in srcs], axis=2)


ways = {'a': way_a,
        'b': lambda: nfp.fss(loader, clim, mask=mask, threshold=THR, scales=SCALES).sums,
        'c': lambda: nfp.fss(loader, clim, mask=mask, threshold=THR, scales=SCALES, use_graph=True).sums,
        'd': lambda: nfp.reliability(loader, clim, mask=mask, threshold=THR, use_graph=True).sums}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
for k in 'bc':                                     # the three compute the same integers
    assert np.array_equal(first[k], first['a']), k
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('abcd' if r % 2 == 0 else 'dcba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)
names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'fss(use_graph=False)', 'c': 'fss(use_graph=True)',
         'd': 'reliability(use_graph=True)'}
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, {first["a"].shape[2]} sources, scales {SCALES}, '
      f'{repeats} repeats (order a b c d / d c b a alternating), commit {commit}')
for k in 'abcd':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
print(f'{kind}:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, max {max(host_ms):7.2f}')
