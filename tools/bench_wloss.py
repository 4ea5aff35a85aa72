"""ms per graphed training step with and without loss weights (informational; bench.py stays as it is).

    python tools/bench_wloss.py mnist|ice [--steps N] [--repeats R] [--commit TEXT]
mnist: BASELINE configs[1] (64x64 Moving-MNIST-like, 2 digits, in=10/out=10, 32 clips, hidden 16, 2 layers).
ice:   the 128x128 masked ice configuration (5 channels, in=12/out=6, 16 clips, land mask, transform_func, hidden 32, 3 conv layers).
Two predictors from the same seed, both with the learning rate at 0 (the frozen model: the same meshes in both and in every
repeat), one captured step each: (u) the unweighted loss, (w) loss_weights = cell_area_weights of 50N..80N and lead_weights
falling linearly from 1 to 0.5.  Every repeat times `steps` replays of each; the order u w / w u alternates between repeats.
Prints the median and the spread of the repeats."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np
import torch

from model.mpnnlstm import NextFramePredictorS2S
from model.utils import cell_area_weights
from qtmpnn import synthetic

dev = torch.device('cuda', 0)
kind = sys.argv[1] if len(sys.argv) > 1 else 'mnist'
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
steps, repeats, commit = arg('--steps', 20), arg('--repeats', 6), arg('--commit', 'unknown')

if kind == 'mnist':
    B, t_in, t_out, shape = 32, 10, 10, (64, 64)
    kw, thresh, tf, feat = dict(hidden_size=16, dropout=0.1, n_layers=2), 0.1, None, 1
    mask = np.zeros(shape, dtype=bool)

    def batch(i):
        return synthetic.make_batch(2, i * B, B, t_in, t_out, n_digits=2, pixel_noise=0.05, canvas=shape)
else:
    B, t_in, t_out, shape = 16, 12, 6, (128, 128)
    tf = lambda a: abs(abs(a - 0.5) - 0.5)
    kw, thresh, feat = dict(hidden_size=32, dropout=0.1, n_layers=1, n_conv_layers=3, transform_func=tf), 0.15, 5
    mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]

    def batch(i):
        clips = [synthetic.make_ice_like(1000 * i + k, shape=shape, channels=5, n_frames=t_in + t_out)[0] for k in range(B)]
        return np.stack([c[:t_in] for c in clips]), np.stack([c[t_in:, ..., :1] for c in clips])

pool = []
for i in range(2):
    x, y = batch(i)
    pool.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.zeros(B, t_out, *shape, 1, device=dev)))
weights = dict(loss_weights=cell_area_weights(np.linspace(80.0, 50.0, shape[0]), shape[1]),
               lead_weights=np.linspace(1.0, 0.5, t_out).astype(np.float32))


def captured(**lw):
    torch.manual_seed(1)
    nfp = NextFramePredictorS2S(thresh=thresh, input_features=feat, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                                transform_func=tf, model_kwargs=kw)
    nfp.initiate_training(lr=0.0, lr_decay=0.95, capturable=True)
    nfp.model.train()
    step = nfp.make_graphed_step(*pool[0], mask=mask, warmup=2, **lw)
    for i in range(3):
        step(*pool[i % 2])
    return nfp, step


ways = {'u': captured(), 'w': captured(**weights)}
ms = {k: [] for k in ways}
for r in range(repeats):
    for k in ('uw' if r % 2 == 0 else 'wu'):
        step = ways[k][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loss = step(*pool[i % 2])
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
        assert torch.isfinite(loss).item()
names = {'u': 'unweighted loss', 'w': 'loss_weights + lead_weights'}
print(f'{kind}: {B} clips of {t_in} in / {t_out} out, {shape}, frozen model, {steps} replays per repeat, {repeats} repeats '
      f'(order u w / w u alternating), commit {commit}')
for k in 'uw':
    v = np.array(ms[k])
    print(f'{kind}: ({k}) {names[k]:<30} median {np.median(v):7.3f} ms per step, min {v.min():7.3f}, max {v.max():7.3f}')
