"""Ice-edge distances of a loader of single clips, ms per clip, three ways (configurations of tools/bench_score.py):
    (a) predict(use_graph=True), then the same eight integers in numpy on the host from the returned frames (what a user did
        before edge_distance(): threshold, edge sets from shifted arrays, nearest-edge distances per (clip, lead time, source))
    (b) edge_distance(use_graph=False)
    (c) edge_distance(use_graph=True)
    python tools/bench_edges.py mnist|ice [--repeats R] [--commit TEXT]
Every repeat times all three over the whole loader (a graphed call includes its captures); the order a b c / c b a alternates
between repeats.  One untimed call of each comes first, and the three must give the same integers.  Prints the median and the
spread of the repeats, and how much of (a) is the numpy pass.
    python tools/bench_edges.py kernel
times the launches alone: ops.rollout_edges (two launches per call: bit-planes, search) on 16 steps of a 128 x 128 pixelwise
frame, one clip, three sources, beside ops.rollout_fss and ops.rollout_scores on the same operands.  The fields are blobs, so
the edge sets are a few hundred pixels each, as a thresholded concentration field's are.  Each call is captured 20 times into one
hipGraph, so that the host side of the op is not in the figure; device events around 10 replays, 5 rounds of all calls in turn."""
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


def kernel_times():
    from qtmpnn import ops
    from qtmpnn.mesh import build_pixel_mesh
    n = m = 128
    T = 16
    rng = np.random.default_rng(0)

    def blobs(*lead):
        """fp32 in (0, 1): 8 x 8 blocks with pixel noise, ice regions with ragged edges on both sides of 0.5"""
        f = np.kron(rng.random(lead + (n // 8, m // 8)), np.ones((8, 8)))
        return torch.from_numpy((0.75 * f + 0.25 * rng.random(lead + (n, m))).astype(np.float32)).to(dev)
    mesh = build_pixel_mesh(1, n, m, None, dev)
    outs = [torch.cat([blobs().reshape(-1, 1), torch.rand(n * m, 3, device=dev)], 1) for _ in range(T)]
    y, clim, pers = blobs(1, T).reshape(1, T, -1), blobs(1, T).reshape(1, T, -1), blobs(1).reshape(1, -1)
    kw = dict(persistence=pers, climatology=clim)
    sums = ops.rollout_edges(outs, [mesh] * T, y, 0.5, **kw).cpu().numpy()
    print(f'kernel: edge pixels per field: forecast median {int(np.median(sums[..., 0]))}, truth median {int(np.median(sums[..., 1]))}; '
          f'largest d2 {int(sums[..., 6:].max())}')
    calls = {'rollout_edges': lambda: ops.rollout_edges(outs, [mesh] * T, y, 0.5, per_tile=True, **kw),
             'rollout_fss scales (1, 3, 5, 9, 17, 33)': lambda: ops.rollout_fss(outs, [mesh] * T, y, 0.5, per_tile=True, **kw),
             'rollout_scores': lambda: ops.rollout_scores(outs, [mesh] * T, y, 0.5, per_tile=True, **kw)}
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
    print(f'kernel: one call of {T} steps, {n} x {m} pixelwise, 1 clip, 3 sources; us per call inside a replayed graph, '
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


def edge_sets(field, keep):
    """(..., W, H) fp32 -> bool edge sets: ice pixels of `keep` with a 4-neighbour inside the frame, in `keep` and not ice."""
    with np.errstate(invalid='ignore'):
        is_ice = keep & (field > np.float32(THR))
    water = keep & ~is_ice
    near = np.zeros_like(water)
    near[..., 1:, :] |= water[..., :-1, :]
    near[..., :-1, :] |= water[..., 1:, :]
    near[..., :, 1:] |= water[..., :, :-1]
    near[..., :, :-1] |= water[..., :, 1:]
    return is_ice & near


def directed(a, b):
    """[sum q, sum d2, max d2] over the pixels of edge set a against edge set b (both (W, H) bool); zeros if either is empty."""
    pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
    if not len(pa) or not len(pb):
        return [0, 0, 0]
    d2 = np.concatenate([((pa[i:i + 512, None] - pb[None]) ** 2).sum(2).min(1) for i in range(0, len(pa), 512)])
    x = d2 << 16
    q = np.sqrt(x.astype(np.float64)).astype(np.int64)
    q -= q * q > x
    q += (q + 1) * (q + 1) <= x
    return [q.sum(), d2.sum(), d2.max()]


def host_sums(field, eo, keep):
    """(n, T, 8) int64 from (n, T, W, H) fp32 fields: qt_edge_rollout's eight integers."""
    ef = edge_sets(field, keep)
    out = np.zeros(field.shape[:2] + (8,), dtype=np.int64)
    for c in range(field.shape[0]):
        for t in range(field.shape[1]):
            fo, of = directed(ef[c, t], eo[c, t]), directed(eo[c, t], ef[c, t])
            out[c, t] = [ef[c, t].sum(), eo[c, t].sum(), fo[0], of[0], fo[1], of[1], fo[2], of[2]]
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
    eo = edge_sets(truth, keep)
    srcs = [frames, persistence] + ([clim_fields] if clim_fields is not None else [])
    out = np.stack([host_sums(f, eo, keep) for f in srcs], axis=2)
    host_ms.append((time.perf_counter() - t0) * 1e3 / n)
    return out


ways = {'a': way_a,
        'b': lambda: nfp.edge_distance(loader, clim, mask=mask, threshold=THR).sums,
        'c': lambda: nfp.edge_distance(loader, clim, mask=mask, threshold=THR, use_graph=True).sums}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
for k in 'bc':                                     # the three compute the same integers
    assert np.array_equal(first[k], first['a']), k
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('abc' if r % 2 == 0 else 'cba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)
names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'edge_distance(use_graph=False)', 'c': 'edge_distance(use_graph=True)'}
s = first['a']
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, {s.shape[2]} sources, edge pixels per field: '
      f'model median {int(np.median(s[:, :, 0, 0]))}, truth median {int(np.median(s[:, :, 0, 1]))}, '
      f'{repeats} repeats (order a b c / c b a alternating), commit {commit}')
for k in 'abc':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
print(f'{kind}:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, max {max(host_ms):7.2f}')
