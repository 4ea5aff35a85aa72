"""Regional extent sums of a loader of single clips, ms per clip (configuration (b) of tools/exp_predict.py: 128 x 128 pixelwise,
TransformerConv, hidden 32, mask + climatology, I10O90, 4 clips, 3 sources; three regions, cell areas of a 0.25 degree grid):
    (a) predict(use_graph=True), then the same sums in numpy on the host from the returned frames
        (tests/extent_restated.py: what a user did before extent())
    (b) extent(use_graph=True)
    (c) the launches alone on one held rollout (ops.rollout_extent: 6 qt_extent_rollout), device events around 50 calls, beside
        ops.rollout_scores on the same operands
    python tools/bench_extent.py [--repeats R] [--commit TEXT] [--out FILE]
Every repeat times (a) and (b) over the whole loader (a graphed call includes its captures), host clock around work that ends in
a synchronise; their order alternates between repeats.  One untimed call of each comes first: their counts must be equal and
their float sums within 16 * 2^-24 * sum |term|.  Prints the median and the spread of the repeats and how much of (a) is the
numpy pass; --out also writes the lines to a file."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from torch.utils.data import DataLoader

from extent_restated import restated_extent
from helpers import TinyIceDataset
from model.mpnnlstm import NextFramePredictorS2S
from model.utils import cell_area_weights
from qtmpnn import ops, synthetic

dev = torch.device('cuda', 0)
repeats = int(sys.argv[sys.argv.index('--repeats') + 1]) if '--repeats' in sys.argv else 6
commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
THR, NAMES = 0.15, ('hudson', 'foxe', 'strait')

torch.manual_seed(0)
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
nfp.model.eval()
loader = DataLoader(ds, batch_size=1, shuffle=False)
n, T = len(ds), nfp.output_timesteps
truth = np.asarray(ds.y)[..., 0].astype(np.float32)
persistence = [np.repeat(np.ascontiguousarray(c, dtype=np.float32)[None], T, axis=0) for c in np.asarray(ds.x)[:, -1, ..., 0]]
clim_fields = np.stack([nfp.get_climatology_array(clim, torch.tensor([t])).cpu().numpy()[..., 0] for t in ds.launch_dates])
regions = np.digitize(np.arange(128), [40, 90])[None].repeat(128, axis=0)
regions[:4] = -1
areas = cell_area_weights(51.0 + 0.25 * np.arange(128), 128)

host_ms = []          # (a)'s numpy part alone, per clip


def way_a():
    frames = nfp.predict(loader, clim, mask=mask, use_graph=True)[..., 0]
    t0 = time.perf_counter()
    out = [restated_extent([frames[c].astype(np.float32), persistence[c], clim_fields[c]], truth[c], ~mask, regions, areas,
                           THR, 3) for c in range(n)]
    host_ms.append((time.perf_counter() - t0) * 1e3 / n)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def way_b():
    return nfp.extent(loader, clim, mask=mask, use_graph=True, threshold=THR, regions=regions, areas=areas,
                      region_names=NAMES).sums, None


ways = {'a': way_a, 'b': way_b}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
want, absterms = first['a']
got = first['b'][0]
assert np.array_equal(got[..., 0, 0], want[..., 0, 0]) and (np.abs(got - want) <= 16 * 2.0 ** -24 * absterms).all()
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('ab' if r % 2 == 0 else 'ba'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ways[k]()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / n)

# (c): the launches alone, on the outputs and meshes of one eager rollout that stay on the device
x, y, launch_date = next(iter(loader))
x, y = nfp._clip(x), nfp._clip(y)
concat = nfp.get_climatology_array(clim, launch_date)
with torch.no_grad():
    y_hat, meshes = nfp.model(x, concat_layers=concat, teacher_forcing_ratio=0, mask=mask)
region_h, area_h, R = ops.check_regions('bench_extent', regions, areas, (128, 128))
region_d, area_d = torch.from_numpy(region_h).to(dev).view(-1), torch.from_numpy(area_h).to(dev).view(-1)
kw = dict(persistence=x[..., -1, :, :, 0], climatology=concat)
calls_of = {'rollout_extent, 3 regions, areas': lambda: ops.rollout_extent(y_hat, meshes, y, THR, region_d, area_d, R, **kw),
            'rollout_extent, no maps': lambda: ops.rollout_extent(y_hat, meshes, y, THR, **kw),
            'rollout_scores': lambda: ops.rollout_scores(y_hat, meshes, y, THR, **kw)}
calls, launch_ms = 50, {k: [] for k in calls_of}
for k, fn in calls_of.items():
    for _ in range(5):
        fn()
    for r in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        launch_ms[k].append(e0.elapsed_time(e1) / calls)

names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'extent(use_graph=True)'}
lines = [f'python tools/bench_extent.py --repeats {repeats} --commit {commit}',
         f'ice: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, 3 sources, 3 regions with cell areas at '
         f'{THR}, {repeats} repeats (order a b / b a alternating), commit {commit}',
         f'ice: counted pixels per region {got[0, 0, :, 0, 0].astype(int).tolist()}, model IIEE per region at the last lead, mean '
         f'over the clips {np.round((got[:, -1, :, 1, 2] + got[:, -1, :, 1, 3]).mean(axis=0), 2).tolist()}']
for k in 'ab':
    v = np.array(ms[k])
    lines.append(f'ice: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
lines.append(f'ice:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, '
             f'max {max(host_ms):7.2f}')
for k, v in launch_ms.items():
    v = np.array(v)
    lines.append(f'ice: (c) {k:<34} ({-(T // -16)} launches + the float64 tile sum, one clip, device events over {calls} calls, '
                 f'host-paced): median {np.median(v):7.3f} ms per call, min {v.min():7.3f}, max {v.max():7.3f}')
print('\n'.join(lines))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
