"""Eager against graphed NextFramePredictorS2S.predict(), ms per clip, as ice_inf.py / the end of ice_exp.py call it (a loader of
single clips).
    python tools/exp_predict.py mnist     (a) the notebook's predictor: 64 x 64, in = 10 / out = 10, hidden 16, 2 layers, ChebConv
    python tools/exp_predict.py ice       (b) 128 x 128 pixelwise, TransformerConv, hidden 32, 3 conv layers, land mask, climatology,
                                              in = 10 / out = 90 (I10O90)
    --hidden 32: (a) at hidden 32;  --quick: one timed call per variant; --eager: eager predict only (for a profiler run)."""
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
quick = '--quick' in sys.argv
eager_only = '--eager' in sys.argv
hidden = int(sys.argv[sys.argv.index('--hidden') + 1]) if '--hidden' in sys.argv else 16       # (a) only: 32 takes k_gemm_fwd's cell


def build():
    torch.manual_seed(0)
    if kind == 'mnist':
        ds = TinyMovingMNISTDataset(16, 10, 10, n_digits=1, canvas_size=(64, 64), digit_size=(28, 28))
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=10, output_timesteps=10, device=dev,
                                    model_kwargs=dict(hidden_size=hidden, dropout=0.1, n_layers=2))
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


ds, nfp, mask, clim = build()
nfp.model.eval()
loader = DataLoader(ds, batch_size=1, shuffle=False)
n = len(ds)
ref = None
print(f'{kind}: {n} clips of {nfp.input_timesteps} in / {nfp.output_timesteps} out, {tuple(ds.image_shape)}')
for use_graph in ((False,) if eager_only else (False, True)):
    nfp.predict(loader, clim, mask=mask, use_graph=use_graph)          # first call: packing, caches, allocator
    reps = 1 if quick else 3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        pred = nfp.predict(loader, clim, mask=mask, use_graph=use_graph)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / (reps * n)
    if ref is None:
        ref = pred
    diff = float(np.nanmax(np.abs(pred - ref)))
    print(f'{kind}: {"graphed" if use_graph else "eager  "} predict: '
          f'{ms:8.2f} ms per clip (capture included, once per call of {n} clips; max |diff| vs first row {diff:.2e})')

if eager_only:
    sys.exit(0)
# steady state of a captured rollout: replay + the one host copy per clip (what every clip after the first of a key costs)
x, _, launch = next(iter(loader))
x = nfp._clip(x)
concat = nfp.get_climatology_array(clim, launch) if clim is not None else None
static0 = nfp.model.static_shapes
roll = nfp.make_graphed_rollout(x, concat, mask=mask)
for _ in range(2):
    roll(x, concat).cpu()
torch.cuda.synchronize()
k = 5 if quick else 20
t0 = time.perf_counter()
for _ in range(k):
    roll(x, concat).cpu().numpy()
ms = (time.perf_counter() - t0) * 1e3 / k
nfp.model.static_shapes = static0
print(f'{kind}: graphed replay + host copy alone: {ms:8.2f} ms per clip')
