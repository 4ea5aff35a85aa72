"""The six default verification products (score, reliability, fss, edge_distance, extent, event_dates) of one loader, two ways:
    (s) six separate calls, one pass over the loader and one rollout per batch each
    (v) one verify() call: one rollout per batch, the six products' launches after it
and, with --parent FILE (the parent commit's model/mpnnlstm.py, e.g. from `git show HEAD~1:quadtree-mpnnlstm_amd/model/mpnnlstm.py`),
    (p) the six separate calls of that file's NextFramePredictorS2S on the same weights, in the same process
each eagerly and with use_graph=True (a graphed call includes its captures: one per product and batch shape for (p) and (s), one
per batch shape for (v)).  Two configurations:
    test   the 64 x 64 masked quadtree case of tests/test_gpu_verify_all.py: 3 in / 4 out, hidden 16, batches of 2, 2 and 1 clips
           (event_dates with persist=2: the default 5 exceeds four output steps)
    bench  bench.py's: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, --batches batches of 32 clips
    python tools/exp_verify.py [--repeats R] [--batches N] [--parent FILE] [--commit TEXT] [--out FILE]
One untimed call of every variant comes first (packing, caches, allocator, code objects) and is compared: every array of (v) and
(p) must equal (s)'s bit for bit.  Every repeat then times each variant over the whole loader, host clock around work that ends
in a synchronise; the order of the variants rotates between repeats.  Prints the median and the spread per variant and the
ratios of the medians; --out also writes the lines to a file."""
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

from helpers import TinyLoader
from model.mpnnlstm import DEFAULT_PRODUCTS, NextFramePredictorS2S
from qtmpnn import synthetic

dev = torch.device('cuda', 0)
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default
repeats, n_batches = arg('--repeats', 7, int), arg('--batches', 4, int)
parent_path, commit, out_path = arg('--parent', None), arg('--commit', 'unknown'), arg('--out', None)
LAUNCH, DAY = 1_483_228_800_000_000_000, 86_400_000_000_000


def parent_class(path):
    spec = importlib.util.spec_from_file_location('parent_mpnnlstm', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.NextFramePredictorS2S


def configurations():
    from test_gpu_score import _case
    nfp, loader, clim, extra = _case('quadtree_masked_64')
    yield ('test', nfp, loader, extra, {'event_dates': dict(persist=2)},
           dict(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=4,
                model_kwargs=dict(hidden_size=16, dropout=0.0, n_layers=2, n_conv_layers=2)))
    torch.manual_seed(0)
    kw = dict(thresh=0.1, input_features=1, input_timesteps=10, output_timesteps=10,
              model_kwargs=dict(hidden_size=16, dropout=0.1, n_layers=2))
    nfp = NextFramePredictorS2S(device=dev, **kw)
    items = []
    for i in range(n_batches):
        x, y = synthetic.make_batch(2, i * 32, 32, 10, 10, n_digits=2, pixel_noise=0.05, canvas=(64, 64))
        items.append((torch.from_numpy(x), torch.from_numpy(y), torch.tensor([LAUNCH + DAY * i])))
    yield 'bench', nfp, TinyLoader(items, (64, 64)), {}, {}, kw


def arrays(result):
    return [result.sums] + ([result.dates] if hasattr(result, 'dates') else [])


lines = []


def emit(line):
    lines.append(line)
    print(line, flush=True)


for line in [f'python tools/exp_verify.py --repeats {repeats} --batches {n_batches}' + (' --parent <parent mpnnlstm.py>' if parent_path else '')
         + f' --commit {commit}',
         f'six products {DEFAULT_PRODUCTS}; ms per call over the whole loader, median (min-max) of {repeats} repeats, the order of the '
         'variants rotating; a graphed call includes its captures']:
    emit(line)
for name, nfp, loader, extra, options, ctor in configurations():
    nfp.model.eval()
    products = {p: options.get(p, {}) for p in DEFAULT_PRODUCTS}
    old = None
    if parent_path:
        old = parent_class(parent_path)(device=dev, **ctor)
        old.model.load_state_dict(nfp.model.state_dict())
        old.model.eval()
    clips = sum(item[0].shape[0] for item in loader)
    emit(f'{name}: {len(loader)} batches, {clips} clips, {nfp.input_timesteps} in / {nfp.output_timesteps} out, '
                 f'{tuple(loader.dataset.image_shape)}, {"masked, " if "mask" in extra else ""}eval mode')
    for use_graph in (False, True):
        separate = lambda who: {p: getattr(who, p)(loader, None, use_graph=use_graph, **extra, **kw) for p, kw in products.items()}
        ways = {'s': lambda: separate(nfp), 'v': lambda: dict(nfp.verify(loader, None, use_graph=use_graph, products=products, **extra).items())}
        if old is not None:
            ways['p'] = lambda: separate(old)
        first = {k: f() for k, f in ways.items()}          # untimed
        for k in first:
            for p in DEFAULT_PRODUCTS:
                for a, b in zip(arrays(first[k][p]), arrays(first['s'][p])):
                    assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (name, use_graph, k, p)
        order, ms = sorted(ways), {k: [] for k in ways}
        for r in range(repeats):
            for k in order[r % len(order):] + order[:r % len(order)]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ways[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        mode = 'graphed' if use_graph else 'eager  '
        label = {'p': 'six separate calls, parent commit', 's': 'six separate calls', 'v': 'one verify() call'}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in sorted(ways):
            emit(f'{name}: {mode} ({k}) {label[k]:<34} median {med[k]:9.1f} ms, min {min(ms[k]):9.1f}, max {max(ms[k]):9.1f}')
        emit(f'{name}: {mode} ratio of the medians (s) / (v) = {med["s"] / med["v"]:.2f}'
                     + (f', (p) / (v) = {med["p"] / med["v"]:.2f}, (s) / (p) = {med["s"] / med["p"]:.2f}' if old is not None else '')
                     + '; every array of the variants equal bit for bit')
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
