"""What a climatology costs a graphed epoch of batches, against the only thing the parent commit offers for that workload -- the
same windows at batch_size=1 -- and whether the epoch without a climatology moved (profiles/climatology_batches.txt).  The two
configurations of tools/exp_clipbank.py (its models, series and stamps):
    bench   64 x 64, 10 in / 10 out, hidden 16, 2 layers; 532 days, 512 windows, 32 clips a step
    ice256  256 x 256 masked, 5 channels, 12 in / 12 out, hidden 32; 56 days, 32 windows, 4 clips a step
Every line is a process of its own under its own time limit: train(use_graph=True, n_epochs=1 + repeats) over ClipBank loaders
(shuffle=False, a test pass of one batch), with normals (1, 366, W, H) of a fixed seed on the device or without; the captures
fall into epoch 0 and the wall time of every later epoch is taken between the epochs' 'Loss/test' reports (tools/exp_clipbank.py's
EpochClock).  The time spent inside get_climatology_array is summed per epoch on the host (time.perf_counter around the call;
the device is not waited for) and reported per batch for the first epoch and for the later ones.
--parent DIR (a checkout of the parent commit with the built library copied in): the batch_size=1 run with a climatology and the
run without a climatology are made on that tree, the latter alternated with this tree's: this, parent, this, parent.

    python tools/exp_climatology_batches.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG BATCH CLIM REPEATS  is such a child (EXP_CLIM_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def one(name, batch, with_clim, repeats):
    import torch
    import exp_clipbank
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, full, what = exp_clipbank.configuration(name)
    batch = full if batch == 0 else batch
    n_test = t_in + t_out + batch           # (the test pass: the first `batch` windows)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    test = ClipBank(series[:n_test], times[:n_test], t_in, t_out, y_channels=yc, device=nfp.device).loader(batch)
    train = bank.loader(batch)
    clim = None
    if with_clim:
        clim = torch.rand(1, 366, *bank.image_shape, generator=torch.Generator().manual_seed(3)).to(nfp.device)
    spent, inner = [0.0, 0], nfp.get_climatology_array

    def timed(climatology, launch_date):
        t0 = time.perf_counter()
        out = inner(climatology, launch_date)
        spent[0] += time.perf_counter() - t0
        spent[1] += 1
        return out
    nfp.get_climatology_array = timed
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    clock = nfp.writer = exp_clipbank.EpochClock()
    per_epoch, add_scalar = [], clock.add_scalar

    def add(tag, value, step):
        add_scalar(tag, value, step)
        if tag == 'Loss/test':
            per_epoch.append(tuple(spent))
    clock.add_scalar = add
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        nfp.train(train, test, clim, n_epochs=1 + repeats, mask=mask, truncated_backprop=0, use_graph=True)
    finally:
        sys.stdout = so
    calls = [(b[0] - a[0], b[1] - a[1]) for a, b in zip([(0.0, 0)] + per_epoch, per_epoch)]
    us = lambda rows: 1e6 * sum(s for s, _ in rows) / max(1, sum(n for _, n in rows))
    rec = {'what': what, 'windows': len(bank), 'batch': batch, 'steps': len(train), 'clim': bool(with_clim),
           'ms': [(b - a) * 1e3 for a, b in zip(clock.stamps, clock.stamps[1:])], 'peak': torch.cuda.max_memory_allocated(),
           'train': nfp.train_loss[-1], 'test': nfp.test_loss[-1], 'clim_us_first': us(calls[:1]), 'clim_us_later': us(calls[1:]),
           'clim_bytes': batch * t_out * bank.image_shape[0] * bank.image_shape[1] * 4}
    print('RESULT ' + json.dumps(rec))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_CLIM_ROOT=root)
    res = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [line[7:] for line in res.stdout.splitlines() if line.startswith('RESULT ')]
    if res.returncode != 0 or len(recs) != 1:
        sys.exit(f'{" ".join(cmd)} ended with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}')
    return json.loads(recs[0])


def main():
    import numpy as np
    repeats, parent, commit, out_path = arg('--repeats', 7, int), arg('--parent', None), arg('--commit', 'unknown'), arg('--out', None)
    configs = arg('--configs', 'bench,ice256').split(',')
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            with open(out_path, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
    med = lambda rec: float(np.median(rec['ms']))
    show = lambda rec: (f'{rec["batch"]:3d} clips a step, {rec["steps"]:3d} steps: epoch median {med(rec):9.2f} ms ({min(rec["ms"]):.2f}-'
                        f'{max(rec["ms"]):.2f}) = {med(rec) / rec["windows"]:7.3f} ms a window   peak {rec["peak"] / 2 ** 20:8.1f} MiB   '
                        f'last epoch train {rec["train"]:.8f} test {rec["test"]:.8f}')
    emit(f'python tools/exp_climatology_batches.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; train(use_graph=True) of {1 + repeats} epochs over '
         f'ClipBank loaders, shuffle=False, a test pass of one batch; times: wall time of an epoch after the epoch of the captures, ms, '
         f'median (min-max) of {repeats}; get_climatology_array: host time per call (one call per batch, the test pass included)')
    for name in configs:
        a = child(HERE, name, 0, 1, repeats)
        emit(f'{name}: {a["what"]}, train mode; {a["windows"]} windows')
        emit(f'{name}: this tree, climatology  {show(a)}')
        emit(f'{name}: get_climatology_array at {a["batch"]} clips: {a["clim_us_first"]:.1f} us a batch in the first epoch, '
             f'{a["clim_us_later"]:.1f} us in the later ones (the day indices of every launch date are kept); it gathers '
             f'{a["clim_bytes"] / 2 ** 20:.2f} MiB a batch')
        if parent:
            root = os.path.abspath(parent)
            b = child(root, name, 1, 1, repeats)
            emit(f'{name}: parent,    climatology  {show(b)}')
            emit(f'{name}: a climatology epoch, this tree at {a["batch"]} clips / parent at 1 clip (all the parent runs: B > 1 raises there): '
                 f'{med(a) / med(b):.3f} x  ({med(b) / med(a):.2f} x the windows a second)')
            emit(f'{name}: get_climatology_array on the parent at 1 clip: {b["clim_us_first"]:.1f} us a batch in the first epoch, '
                 f'{b["clim_us_later"]:.1f} us later')
        runs = [('this tree', child(HERE, name, 0, 0, repeats))]
        if parent:
            for tree, r in (('parent', root), ('this tree', HERE), ('parent', root)):
                runs.append((tree, child(r, name, 0, 0, repeats)))
        for tree, rec in runs:
            emit(f'{name}: {tree + ",":<10} no climatology  {show(rec)}')
        emit(f'{name}: climatology / no climatology on this tree: epoch {med(a) / med(runs[0][1]):.3f} x')
        if parent:
            this = [m for tree, rec in runs if tree == 'this tree' for m in rec['ms']]
            par = [m for tree, rec in runs if tree == 'parent' for m in rec['ms']]
            same = len({(rec['train'], rec['test']) for _, rec in runs}) == 1
            emit(f'{name}: no climatology, this tree: median {np.median(this):.2f} ms ({min(this):.2f}-{max(this):.2f}) of {len(this)} epochs;  '
                 f'parent: median {np.median(par):.2f} ms ({min(par):.2f}-{max(par):.2f}) of {len(par)};  this / parent '
                 f'{np.median(this) / np.median(par):.4f} x;  the losses of the four runs are ' + ('equal' if same else 'NOT equal'))


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_CLIM_ROOT', HERE)
        for p in (os.path.join(root, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one(a[0], int(a[1]), int(a[2]), int(a[3]))
    else:
        main()
