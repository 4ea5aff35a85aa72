"""Probability verification of a loader of single clips, ms per clip, three ways (configurations of tools/bench_score.py):
    (a) predict(use_graph=True), then the same per-bin sums in numpy on the host from the returned frames (what a user did
        before reliability())
    (b) reliability(use_graph=False)
    (c) reliability(use_graph=True)
    python tools/bench_reliability.py mnist|ice [--repeats R] [--bins K] [--commit TEXT]
Every repeat times all three over the whole loader (a graphed call includes its captures); the order of (a) and (c) alternates
between repeats.  One untimed call of each comes first.  Prints the median and the spread of the repeats, and how much of (a) is
the numpy pass."""
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
K = int(sys.argv[sys.argv.index('--bins') + 1]) if '--bins' in sys.argv else 10
commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
THR = 0.15


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


def host_sums(field, truth, keep):
    """(n, T, K, 4) float64 from (n, T, W, H) fp32 fields: the four sums per bin of qt_reliability_rollout over the pixels of
    `keep` (the bin from t = f * K in fp32, one bincount per slot over (clip, step, bin))."""
    f, y = field[:, :, keep], truth[:, :, keep]
    o = y > np.float32(THR)
    with np.errstate(invalid='ignore', over='ignore'):
        t = f * np.float32(K)
        k = np.where(t >= np.float32(1), np.minimum(t, np.float32(K - 1)), np.float32(0))
    k = np.nan_to_num(k, nan=0.0).astype(np.int64)
    cell = (np.arange(f.shape[0] * f.shape[1]).reshape(f.shape[0], f.shape[1], 1) * K + k).ravel()
    f64 = f.astype(np.float64)
    d = f64 - o
    size = f.shape[0] * f.shape[1] * K
    slots = [np.bincount(cell, minlength=size), np.bincount(cell, weights=o.ravel(), minlength=size),
             np.bincount(cell, weights=f64.ravel(), minlength=size), np.bincount(cell, weights=(d * d).ravel(), minlength=size)]
    return np.stack(slots, axis=-1).astype(np.float64).reshape(f.shape[0], f.shape[1], K, 4)


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
    srcs = [frames, persistence] + ([clim_fields] if clim_fields is not None else [])
    return np.stack([host_sums(f, truth, keep) for f in srcs], axis=2)


ways = {'a': way_a,
        'b': lambda: nfp.reliability(loader, clim, mask=mask, threshold=THR, bins=K).sums,
        'c': lambda: nfp.reliability(loader, clim, mask=mask, threshold=THR, bins=K, use_graph=True).sums}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
for k in 'bc':                                     # the three compute the same numbers (counts equal; sums to fp32 summation error)
    assert np.array_equal(first[k][..., :2], first['a'][..., :2]), k
    rel = np.abs(first[k][..., 2:] - first['a'][..., 2:]).max() / np.abs(first['a'][..., 2:]).max()
    assert rel < 1e-5, (k, rel)
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('abc' if r % 2 == 0 else 'cba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)
names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'reliability(use_graph=False)', 'c': 'reliability(use_graph=True)'}
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, {first["a"].shape[2]} sources, {K} bins, '
      f'{repeats} repeats (order a b c / c b a alternating), commit {commit}')
for k in 'abc':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
print(f'{kind}:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, max {max(host_ms):7.2f}')
