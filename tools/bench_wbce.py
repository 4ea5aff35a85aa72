"""The weighted binary cross-entropy of a binary=True predictor against the unweighted fused one (informational; bench.py stays as
it is).

    python tools/bench_wbce.py [--steps N] [--repeats R] [--commit TEXT] [--out FILE]
BASELINE configs[1] shapes (64x64 Moving-MNIST-like, 2 digits, in=10/out=10, 32 clips, hidden 16, 2 layers) with binary=True, the
learning rate at 0 (the frozen model: the same meshes in every repeat), as tools/bench_bce.py.
(1) The loss alone, forward + backward down to the gradients of the ten output steps, on the outputs and meshes of one rollout:
    (f) masked_mse(binary=True, fused=True), qt_bce_rollout / _bwd;  (w) masked_bce with cell-area pixel weights, rising lead-time
    weights and pos_weight = 3, qt_wbce_rollout / _bwd.
(2) One replay of the captured training step (make_graphed_step) on the same two batches: (u) unweighted, the step a binary
    predictor captured before the weighted loss existed (its launches are unchanged), (g) with the three weights.
Every repeat times `steps` calls of each between two device synchronisations; the order alternates between repeats.  Prints the
median and the spread of the repeats; --out FILE also writes every printed line to FILE.  The loss kernels' own durations in
profiles/wbce.txt come from a `rocprofv3 --kernel-trace --stats` run of this script, taken on its own."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np
import torch

from model.mpnnlstm import NextFramePredictorS2S, masked_bce, masked_mse
from model.utils import cell_area_weights
from qtmpnn import synthetic

dev = torch.device('cuda', 0)
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
steps, repeats, commit, out_path = arg('--steps', 20), arg('--repeats', 6), arg('--commit', 'unknown'), arg('--out', '')
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


B, t_in, t_out, shape = 32, 10, 10, (64, 64)
kw = dict(hidden_size=16, dropout=0.1, n_layers=2)
mask = np.zeros(shape, dtype=bool)
weights = dict(loss_weights=cell_area_weights(np.linspace(50.0, 85.0, shape[0]), shape[1]),
               lead_weights=np.linspace(0.5, 1.5, t_out).astype(np.float32), pos_weight=3.0)
pool = []
for i in range(2):
    x, y = synthetic.make_batch(2, i * B, B, t_in, t_out, n_digits=2, pixel_noise=0.05, canvas=shape)
    pool.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).clamp(0, 1).to(dev), torch.zeros(B, t_out, *shape, 1, device=dev)))


def predictor():
    torch.manual_seed(1)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev, binary=True,
                                model_kwargs=kw)
    nfp.initiate_training(lr=0.0, lr_decay=0.95, capturable=True)
    nfp.model.train()
    return nfp


def timed(ways, order):
    ms = {k: [] for k in ways}
    for r in range(repeats):
        for k in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                ways[k](i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return ms


def report(ms, names):
    for k, name in names.items():
        v = np.array(ms[k])
        say(f'wbce: ({k}) {name:<52} median {np.median(v):8.3f} ms, min {v.min():8.3f}, max {v.max():8.3f}')


say(f'wbce: {B} clips of {t_in} in / {t_out} out, {shape}, binary=True, frozen model, {steps} calls per repeat, {repeats} repeats '
    f'(order alternating), commit {commit}')
plain = predictor()
xt, yt, ct = pool[0]
with torch.no_grad():
    outs, meshes = plain.model(xt, yt, ct, teacher_forcing_ratio=0, mask=mask)
leaves = [o.detach().clone().requires_grad_(True) for o in outs]
lw = plain._loss_weights(xt, mask, weights['loss_weights'], weights['lead_weights'], weights['pos_weight'])
losses = {'f': lambda: masked_mse(leaves, meshes, yt, mask, binary=True, fused=True),
          'w': lambda: masked_bce(leaves, meshes, yt, mask, weights=lw, pos_weight=lw.pos_weight)}
ways = {k: (lambda i, fn=fn: torch.autograd.grad(fn(), leaves)) for k, fn in losses.items()}
say(f'wbce: loss unweighted {float(losses["f"]().detach()):.8f}, weighted {float(losses["w"]().detach()):.8f}')
for k in ways:
    for i in range(3):
        ways[k](i)
report(timed(ways, 'fw'), {'f': 'loss alone, unweighted fused (fwd + bwd)', 'w': 'loss alone, weighted (fwd + bwd)'})
del leaves, outs, meshes

unweighted, weighted = predictor(), predictor()
step_u = unweighted.make_graphed_step(*pool[0], mask=mask, warmup=2)
step_g = weighted.make_graphed_step(*pool[0], mask=mask, warmup=2, **weights)
ways = {'u': lambda i: step_u(*pool[i % 2]), 'g': lambda i: step_g(*pool[i % 2])}
for k in ways:
    for i in range(3):
        assert torch.isfinite(ways[k](i)).item()
report(timed(ways, 'ug'), {'u': 'captured training step, unweighted (one replay)', 'g': 'captured training step, weighted (one replay)'})
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
