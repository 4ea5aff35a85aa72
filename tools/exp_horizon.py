"""What the rollout horizon (set_horizon, train(horizon=)) costs and saves (profiles/horizon.txt).  The two configurations of
tools/exp_clipbank.py:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, 32 clips a step
    ice256  the 256 x 256 sea-ice configuration: 5 channels, 12 in / 12 out, hidden 32, 1 layer, 3 conv layers, land mask, 4 clips
and these measurements, each variant a process of its own under its own time limit:
    step        the captured training step (make_graphed_step, clipping at 10) replayed on one batch: REPLAYS replays between two
                synchronisations, timed `repeats` times -> us per step, median (min-max), the last loss and the peak device memory
                of the process.  Variants: horizon k for every k of the configuration's list (the predictor is built with the
                last one; y keeps the built steps and is read through its clip stride), `none` (no horizon set) and, with
                --parent DIR, the parent commit's tree (which has no horizon).  The medians and peaks over k get a least-squares
                line a + b k, with the largest residual, to say whether they are affine in k.
    curriculum  train(use_graph=True, horizon=[1, 2, 4, ...]) from the start weights, a few epochs: whether it gets past
                train()'s own `Diverged :(` guard, which reads the test pass at the BUILT horizon.

    python tools/exp_horizon.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one KIND CONFIG VARIANT REPEATS  is such a child (EXP_HORIZON_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
REPLAYS = 40            # of the captured step per timed repeat
HORIZONS = {'bench': (1, 2, 5, 10), 'ice256': (3, 6, 12)}          # the last one is what the predictor is built with
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def one_step(name, variant, repeats):
    import torch
    from exp_clipbank import configuration
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    assert t_out == HORIZONS[name][-1], (t_out, HORIZONS[name])
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    x, y, _ = next(iter(bank.loader(batch)))
    x, y = nfp._clip(x), nfp._clip(y)
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    if variant not in ('none', 'parent'):
        nfp.set_horizon(int(variant))
    step = nfp.make_graphed_step(x, y, None, mask)
    for _ in range(5):
        step(x, y)
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPLAYS):
            loss = step(x, y)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / REPLAYS)
    print('RESULT ' + json.dumps({'what': what, 'us': us, 'loss': float(loss), 'steps': int(nfp.output_timesteps),
                                  'peak': torch.cuda.max_memory_allocated()}))


def one_curriculum(name, variant, repeats):
    import torch
    from exp_clipbank import configuration
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    nfp.model.train()
    schedule = [k for k in (1, 2, 4, 8, 16, 32, 64) if k < t_out] + [t_out]
    kw = {} if variant == 'plain' else dict(horizon=schedule)
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    t0, refused = time.perf_counter(), None
    try:
        nfp.train(bank.loader(batch), bank.loader(batch), None, n_epochs=len(schedule), lr=2e-4, mask=mask, truncated_backprop=0,
                  use_graph=True, **kw)
    except ValueError as e:         # (train()'s own guards on the test loss: 'NaN loss :(' and 'Diverged :(' above 4)
        refused = f'{e} in epoch {len(nfp.test_loss)}'
    finally:
        sys.stdout = so
    torch.cuda.synchronize()
    print('RESULT ' + json.dumps({'what': what, 'schedule': schedule, 'refused': refused, 'train': nfp.train_loss, 'test': nfp.test_loss,
                                  'steps': len(bank.loader(batch)), 's': time.perf_counter() - t0, 'peak': torch.cuda.max_memory_allocated()}))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_HORIZON_ROOT=root)
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
    med = lambda v: float(np.median(v))
    us = lambda v: f'{med(v):9.1f} us ({min(v):.1f}-{max(v):.1f})'

    def line_fit(ks, vs, unit):
        b, a = np.polyfit(ks, vs, 1)
        worst = max(abs(a + b * k - v) / v for k, v in zip(ks, vs))
        return f'{a:.1f} + {b:.1f} k {unit}, largest residual {100 * worst:.2f} % of the value'
    emit(f'python tools/exp_horizon.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; captured step, {REPLAYS} replays a repeat, median '
         f'(min-max) of {repeats}')
    for name in configs:
        ks = HORIZONS[name]
        steps = {}
        for variant, root in [('parent', parent), ('none', HERE)] + [(str(k), HERE) for k in ks]:
            if root:
                steps[variant] = child(os.path.abspath(root), 'step', name, variant, repeats)
        emit(f'{name}: {steps["none"]["what"]}, train mode, built with {ks[-1]} output steps')
        for variant, rec in steps.items():
            label = variant if variant in ('parent', 'none') else f'k = {variant}'
            emit(f'{name}: horizon {label:<7} {rec["steps"]:3d} steps  {us(rec["us"])} a step   last loss {rec["loss"]:.8f}   '
                 f'peak device memory {rec["peak"]} bytes')
        none, built = steps['none'], steps[str(ks[-1])]
        emit(f'{name}: horizon = the built value against none set: {med(built["us"]) / med(none["us"]):.4f} x; the losses are '
             + ('equal' if built['loss'] == none['loss'] else 'NOT equal') + f'; peak {built["peak"] - none["peak"]:+d} bytes')
        if parent:
            par = steps['parent']
            inside = min(par['us']) <= med(none['us']) <= max(par['us']) or min(none['us']) <= med(par['us']) <= max(none['us'])
            emit(f'{name}: horizon=None / parent: {med(none["us"]) / med(par["us"]):.4f} x (spread of the repeats: parent '
                 f'{min(par["us"]) / med(par["us"]):.3f}-{max(par["us"]) / med(par["us"]):.3f}, this tree '
                 f'{min(none["us"]) / med(none["us"]):.3f}-{max(none["us"]) / med(none["us"]):.3f} of the median); the medians lie '
                 + ('inside' if inside else 'OUTSIDE') + ' the min-max of the other\'s repeats; the losses are '
                 + ('equal' if none['loss'] == par['loss'] else 'NOT equal') + f'; peak {none["peak"] - par["peak"]:+d} bytes')
        emit(f'{name}: step time over k = {ks}: ' + line_fit(ks, [med(steps[str(k)]['us']) for k in ks], 'us'))
        emit(f'{name}: peak device memory over k = {ks}: ' + line_fit(ks, [steps[str(k)]['peak'] / 2 ** 20 for k in ks], 'MiB'))
        for variant in ('plain', 'curriculum'):
            rec = child(HERE, 'curriculum', name, variant, repeats)
            asked = '' if variant == 'plain' else f', horizon={rec["schedule"]}'
            said = f'train(use_graph=True{asked}), {len(rec["schedule"])} epochs of {rec["steps"]} steps from the start weights'
            fmt = lambda v: '[' + ', '.join(f'{e:.4f}' for e in v) + ']'
            if rec['refused']:
                emit(f'{name}: {said}: ended with ValueError({rec["refused"]!r}), its guard on the test loss at the built horizon; '
                     f'epochs finished: train {fmt(rec["train"])} test {fmt(rec["test"])}')
            else:
                emit(f'{name}: {said}: finished in {rec["s"]:.1f} s; train {fmt(rec["train"])} test {fmt(rec["test"])}; peak device '
                     f'memory {rec["peak"]} bytes')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_HORIZON_ROOT', HERE)
        for p in (os.path.join(HERE, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        (one_step if a[0] == 'step' else one_curriculum)(a[1], a[2], int(a[3]))
    else:
        main()
