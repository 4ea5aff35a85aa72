"""Break-up dates of a loader of single clips, ms per clip (configuration (b) of tools/exp_predict.py: 128 x 128 pixelwise,
TransformerConv, hidden 32, mask + climatology, I10O90, 4 clips, 3 sources):
    (a) predict(use_graph=True), then the same dates and sums in numpy on the host from the returned frames
        (tests/events_restated.py: what a user did before event_dates())
    (b) event_dates(use_graph=True)
    (c) the scan + sums launches alone on one held rollout (ops.rollout_event_dates: 6 qt_event_scan + 1 qt_event_sums), device
        events around 50 calls
    python tools/bench_events.py [--repeats R] [--commit TEXT] [--out FILE]
Every repeat times (a) and (b) over the whole loader (a graphed call includes its captures), host clock around work that ends in
a synchronise; their order alternates between repeats.  One untimed call of each comes first, and the two must agree exactly.
Prints the median and the spread of the repeats and how much of (a) is the numpy pass; --out also writes the lines to a file."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from torch.utils.data import DataLoader

from events_restated import restated_events
from helpers import TinyIceDataset
from model.mpnnlstm import NextFramePredictorS2S
from qtmpnn import ops, synthetic

dev = torch.device('cuda', 0)
repeats = int(sys.argv[sys.argv.index('--repeats') + 1]) if '--repeats' in sys.argv else 6
commit = sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else 'unknown'
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
THR, KIND, PERSIST = 0.15, 'breakup', 5

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
launches = [np.ascontiguousarray(c, dtype=np.float32) for c in np.asarray(ds.x)[:, -1, ..., 0]]
clim_fields = np.stack([nfp.get_climatology_array(clim, torch.tensor([t])).cpu().numpy()[..., 0] for t in ds.launch_dates])

host_ms = []          # (a)'s numpy part alone, per clip


def way_a():
    frames = nfp.predict(loader, clim, mask=mask, use_graph=True)[..., 0]
    t0 = time.perf_counter()
    fields = [{'observed': truth[c], 'model': frames[c], 'climatology': clim_fields[c]} for c in range(n)]
    out = restated_events(fields, launches, mask, THR, KIND, PERSIST)
    host_ms.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def way_b():
    ev = nfp.event_dates(loader, clim, mask=mask, use_graph=True, threshold=THR, kind=KIND, persist=PERSIST)
    return ev.dates, ev.sums


ways = {'a': way_a, 'b': way_b}
first = {k: f() for k, f in ways.items()}          # untimed: packing, caches, allocator, code objects
host_ms.clear()
assert np.array_equal(first['a'][0], first['b'][0]) and np.array_equal(first['a'][1], first['b'][1])
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
scan = lambda: ops.rollout_event_dates(y_hat, meshes, y, x[..., -1, :, :, 0], THR, KIND, PERSIST, concat)
for _ in range(5):
    scan()
calls, scan_ms = 50, []
for r in range(repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        scan()
    e1.record()
    torch.cuda.synchronize()
    scan_ms.append(e0.elapsed_time(e1) / calls)

tot = first['b'][1][:, 0].sum(axis=0)
names = {'a': 'predict(use_graph=True) + numpy on the host', 'b': 'event_dates(use_graph=True)'}
lines = [f'python tools/bench_events.py --repeats {repeats} --commit {commit}',
         f'ice: {n} clips of {nfp.input_timesteps} in / {T} out, {tuple(ds.image_shape)}, 3 sources, {KIND} persist {PERSIST} at '
         f'{THR}, {repeats} repeats (order a b / b a alternating), commit {commit}',
         f'ice: model sums over the clips [n, sum e, sum |e|, sum e^2, hits, false alarms, misses, neither] {tot.tolist()}']
for k in 'ab':
    v = np.array(ms[k])
    lines.append(f'ice: ({k}) {names[k]:<46} median {np.median(v):7.2f} ms per clip, min {v.min():7.2f}, max {v.max():7.2f}')
lines.append(f'ice:     of (a), the numpy pass alone: median {np.median(host_ms):7.2f} ms per clip, min {min(host_ms):7.2f}, '
             f'max {max(host_ms):7.2f}')
v = np.array(scan_ms)
lines.append(f'ice: (c) scan + sums launches alone ({-(T // -16)} + 1 launches, one clip, device events over {calls} calls): '
             f'median {np.median(v):7.3f} ms per clip, min {v.min():7.3f}, max {v.max():7.3f}')
print('\n'.join(lines))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
