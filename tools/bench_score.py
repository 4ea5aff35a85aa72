"""Verification of a loader of single clips, ms per clip, three ways (configurations of tools/exp_predict.py):
    (a) predict(use_graph=True), then the same sums in numpy on the host from the returned frames (what a user did before score())
    (b) score(use_graph=False)
    (c) score(use_graph=True)
    python tools/bench_score.py mnist|ice [--repeats R] [--commit TEXT]
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
    """(n, T, 8) float64 from (n, T, W, H) fp32 fields: the eight sums of qt_score_rollout over the pixels of `keep`."""
    f, y = field[:, :, keep], truth[:, :, keep]
    d = f.astype(np.float64) - y
    fi, yi = f > np.float32(THR), y > np.float32(THR)
    return np.stack([np.full(d.shape[:2], d.shape[2], np.float64), d.sum(-1), np.abs(d).sum(-1), (d * d).sum(-1),
                     *(np.count_nonzero(c, axis=-1) for c in (fi & yi, fi & ~yi, ~fi & yi, ~fi & ~yi))], axis=-1)


ds, nfp, mask, clim = build()
nfp.model.eval()
loader = DataLoader(ds, batch_size=1, shuffle=False)
n, T = len(ds), nfp.output_timesteps
keep = np.ones(tuple(ds.image_shape), bool) if mask is None else ~np.asarray(mask, bool)
truth = np.asarray(ds.y)[..., 0]
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
        'b': lambda: nfp.score(loader, clim, mask=mask, threshold=THR).sums,
        'c': lambda: nfp.score(loader, clim, mask=mask, threshold=THR, use_graph=True).sums}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
for k in 'bc':                                     # the three compute the same numbers (counts equal; sums to fp32 summation error)
    assert np.array_equal(first[k][..., [0, 4, 5, 6, 7]], first['a'][..., [0, 4, 5, 6, 7]]), k
    rel = np.abs(first[k][..., 1:4] - first['a'][..., 1:4]).max() / np.abs(first['a'][..., 1:4]).max()
    assert rel < 1e-5, (k, rel)
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('abc' if r % 2 == 0 else 'cba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)
names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'score(use_graph=False)', 'c': 'score(use_graph=True)'}
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, {first["a"].shape[2]} sources, '
      f'{repeats} repeats (order a b c / c b a alternating), commit {commit}')
for k in 'abc':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
print(f'{kind}:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, max {max(host_ms):7.2f}')
