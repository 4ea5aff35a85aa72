"""Size of a checkpoint and the time of save_checkpoint() / load_checkpoint() for the headline configuration of bench.py (64 x 64,
10 in / 10 out, hidden 16, 2 layers, 32 clips, the captured training step).  Recorded only (profiles/checkpoint.txt): neither
figure is compared with anything.  The load is the in-place one, into the predictor whose captured step then replays once.

    python tools/bench_checkpoint.py [--repeats 7] [--out DIR]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch
    import bench
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='directory of the checkpoint file (default: a temporary one)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    nfp = NextFramePredictorS2S(thresh=bench.THRESH, input_features=1, input_timesteps=bench.T_IN, output_timesteps=bench.T_OUT,
                                device=dev, model_kwargs=dict(hidden_size=bench.HIDDEN, dropout=bench.DROPOUT, n_layers=bench.N_LAYERS))
    nfp.initiate_training(lr=bench.LR, lr_decay=0.95, capturable=True)
    x, y = synthetic.make_batch(2, 0, 32, bench.T_IN, bench.T_OUT, n_digits=bench.N_DIGITS, pixel_noise=bench.NOISE, canvas=bench.CANVAS)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    mask = np.zeros(bench.CANVAS, dtype=bool)
    step = nfp.make_graphed_step(x, y, None, mask, warmup=2)
    losses = [float(step(x, y)) for _ in range(3)]
    with tempfile.TemporaryDirectory(dir=args.out) as d:
        path = os.path.join(d, 'headline.ckpt')
        save, load = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nfp.save_checkpoint(path)
            t1 = time.perf_counter()
            nfp.load_checkpoint(path)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            save.append(1e3 * (t1 - t0))
            load.append(1e3 * (t2 - t1))
        size = os.path.getsize(path)
    after = float(step(x, y))
    n = sum(p.numel() for p in nfp.model.parameters())
    line = lambda v: f'median {statistics.median(v):7.2f} ms, min {min(v):7.2f}, max {max(v):7.2f}'
    print(f'headline: {n} parameters in {len(list(nfp.model.parameters()))} tensors, flat path {nfp.flat is not None}, captured step, '
          f'{args.repeats} repeats')
    print(f'headline: checkpoint file {size} bytes ({size / 1024:.1f} KiB)')
    print(f'headline: save_checkpoint  {line(save)}')
    print(f'headline: load_checkpoint  {line(load)}   (in place, into the predictor of the captured step)')
    print(f'headline: losses of the replays before {losses}, of the replay after the last load {after}')
    assert np.isfinite(losses + [after]).all()


if __name__ == '__main__':
    main()
