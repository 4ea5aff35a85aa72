"""Per-pixel verification maps of a loader of single clips, ms per clip, three ways (configurations of tools/bench_score.py):
    (a) predict(use_graph=True), then the same per-pixel sums in numpy on the host from the returned frames
    (b) score(use_graph=True)                     -- no maps: what the maps cost is (c) - (b)
    (c) score_maps(use_graph=True)                -- sums and maps from one pass
    python tools/bench_score_maps.py mnist|ice [--repeats R] [--commit TEXT]
Every repeat times all three over the whole loader (a graphed call includes its captures); the order alternates a b c / c b a
between repeats.  One untimed call of each comes first, and (a)'s and (c)'s maps are compared.  Prints the median and the spread of
the repeats, how much of (a) is the numpy pass, and the bytes qt_score_maps moves per batch (for the kernel time of a
`rocprofv3 --kernel-trace --stats` run of this script, taken on its own)."""
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


def host_maps(field, truth, keep):
    """(T, 8, W, H) float64 from (n, T, W, H) fp32 fields: the eight sums of qt_score_maps per pixel over the n clips (fp32 d,
    widened; pixels outside `keep` stay 0)."""
    with np.errstate(invalid='ignore'):
        d = np.where(keep, (field - truth).astype(np.float64), 0.0)
        fi, yi = (field > np.float32(THR)) & keep, (truth > np.float32(THR)) & keep
    nf, ny = ~fi & keep, ~yi & keep
    n = np.broadcast_to(keep, field.shape)
    return np.stack([a.sum(axis=0, dtype=np.float64) for a in (n, d, np.abs(d), d * d, fi & yi, fi & ny, nf & yi, nf & ny)], axis=1)


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
    srcs = [frames, persistence] + ([clim_fields] if clim_fields is not None else [])
    out = np.stack([host_maps(f, truth, keep) for f in srcs], axis=1)         # (T, S, 8, W, H)
    host_ms.append((time.perf_counter() - t0) * 1e3 / n)
    return out


ways = {'a': way_a,
        'b': lambda: nfp.score(loader, clim, mask=mask, threshold=THR, use_graph=True).sums,
        'c': lambda: nfp.score_maps(loader, clim, mask=mask, threshold=THR, use_graph=True).maps.sums}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
counts = [0, 4, 5, 6, 7]                           # (a) and (c) compute the same maps: counts equal, sums to float64 summation order
assert first['c'].shape == first['a'].shape, (first['c'].shape, first['a'].shape)
assert np.array_equal(first['c'][:, :, counts], first['a'][:, :, counts])
rel = np.abs(first['c'][:, :, 1:4] - first['a'][:, :, 1:4]).max() / np.abs(first['a'][:, :, 1:4]).max()
assert rel < 1e-12, rel
assert np.array_equal(first['c'][:, :, 0].sum((-2, -1)), first['b'][..., 0].sum(0))
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('abc' if r % 2 == 0 else 'cba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)
names = {'a': 'predict(use_graph=True) + numpy maps on the host', 'b': 'score(use_graph=True)', 'c': 'score_maps(use_graph=True)'}
S, P = first['a'].shape[1], int(np.prod(ds.image_shape))
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, {S} sources, '
      f'{repeats} repeats (order a b c / c b a alternating), commit {commit}')
for k in 'abc':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<50} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
print(f'{kind}:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, max {max(host_ms):7.2f}')
buf = 8 * S * T * P * 8
print(f'{kind}:     maps buffer {buf / 1e6:.1f} MB ({T} x {S} x 8 x {P} doubles); a batch reads and writes the unmasked share '
      f'{keep.mean():.3f} of it once: {2 * buf * keep.mean() / 1e6:.1f} MB over {-(T // -16)} launches of qt_score_maps')
