"""The binary cross-entropy of a binary=True predictor, torch path against the fused launches (informational; bench.py stays as
it is).

    python tools/bench_bce.py [--steps N] [--repeats R] [--commit TEXT]
BASELINE configs[1] shapes (64x64 Moving-MNIST-like, 2 digits, in=10/out=10, 32 clips, hidden 16, 2 layers) with binary=True, the
learning rate at 0 (the frozen model: the same meshes in every repeat).
(1) The loss alone, forward + backward down to the gradients of the ten output steps, on the outputs and meshes of one rollout:
    (t) masked_mse(binary=True), torch's path: ten frames, a boolean index, BCELoss;  (f) masked_mse(binary=True, fused=True).
(2) One training step: (e) the eager train_step on the torch path, which is all a binary predictor could run before, against
    (g) one replay of the captured step (make_graphed_step; it runs the fused loss).
Every repeat times `steps` calls of each between two device synchronisations; the order alternates between repeats.  Prints the
median and the spread of the repeats."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np
import torch

from model.mpnnlstm import NextFramePredictorS2S, masked_mse
from qtmpnn import synthetic

dev = torch.device('cuda', 0)
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
steps, repeats, commit = arg('--steps', 20), arg('--repeats', 6), arg('--commit', 'unknown')

B, t_in, t_out, shape = 32, 10, 10, (64, 64)
kw = dict(hidden_size=16, dropout=0.1, n_layers=2)
mask = np.zeros(shape, dtype=bool)
pool = []
for i in range(2):
    x, y = synthetic.make_batch(2, i * B, B, t_in, t_out, n_digits=2, pixel_noise=0.05, canvas=shape)
    pool.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).clamp(0, 1).to(dev), torch.zeros(B, t_out, *shape, 1, device=dev)))


def predictor(capturable):
    torch.manual_seed(1)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev, binary=True,
                                model_kwargs=kw)
    nfp.initiate_training(lr=0.0, lr_decay=0.95, capturable=capturable)
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
        print(f'bce: ({k}) {name:<44} median {np.median(v):8.3f} ms, min {v.min():8.3f}, max {v.max():8.3f}')


print(f'bce: {B} clips of {t_in} in / {t_out} out, {shape}, binary=True, frozen model, {steps} calls per repeat, {repeats} repeats '
      f'(order alternating), commit {commit}')
eager = predictor(False)
xt, yt, ct = pool[0]
with torch.no_grad():
    outs, meshes = eager.model(xt, yt, ct, teacher_forcing_ratio=0, mask=mask)
leaves = [o.detach().clone().requires_grad_(True) for o in outs]


def loss_alone(**kw_):
    def run(i):
        loss = masked_mse(leaves, meshes, yt, mask, binary=True, **kw_)
        return torch.autograd.grad(loss, leaves)
    return run


ways = {'t': loss_alone(), 'f': loss_alone(fused=True)}
lt, lf = (float(masked_mse(leaves, meshes, yt, mask, binary=True, **k).detach()) for k in ({}, dict(fused=True)))
gt, gf = ways['t'](0), ways['f'](0)
gerr = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(gt, gf))
print(f'bce: loss torch path {lt:.8f}, fused {lf:.8f}; largest gradient difference / largest entry of a step {gerr:.2e}')
for k in ways:
    for i in range(3):
        ways[k](i)
report(timed(ways, 'tf'), {'t': 'loss alone, torch path (fwd + bwd)', 'f': 'loss alone, fused (fwd + bwd)'})
del leaves, outs, meshes, gt, gf

graphed = predictor(True)
step = graphed.make_graphed_step(*pool[0], mask=mask, warmup=2)
ways = {'e': lambda i: eager.train_step(*pool[i % 2], mask), 'g': lambda i: step(*pool[i % 2])}
for k in ways:
    for i in range(3):
        assert torch.isfinite(ways[k](i)).item()
report(timed(ways, 'eg'), {'e': 'training step, eager, torch path', 'g': 'training step, one replay of the captured step'})
