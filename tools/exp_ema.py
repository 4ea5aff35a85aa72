"""What the averaged weights (set_ema, train(ema=)) cost (profiles/ema.txt).  The two configurations of tools/exp_clipbank.py:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, 32 clips a step
    ice256  the 256 x 256 sea-ice configuration: 5 channels, 12 in / 12 out, hidden 32, 1 layer, 3 conv layers, land mask, 4 clips
and these measurements, each variant a process of its own under its own time limit:
    step   the captured training step (make_graphed_step, clipping at 10) replayed on one batch: REPLAYS replays between two
           synchronisations, timed `repeats` times -> us per step, median (min-max); variants: ema=None, ema=0.999 and, with
           --parent DIR, the parent commit's tree (which has no `ema`).  Also the last loss (the variants must agree) and the
           peak device memory of the process.
    epoch  one epoch of train(use_graph=True, test_graph=True) over a ClipBank loader with a test loader of the same size
           (tools/exp_validation.py's clock): no ema, ema=0.999 with ema_eval=False, ema=0.999 with ema_eval=True -- the last
           two differ by the two parameter copies and the division per test pass.

    python tools/exp_ema.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one KIND CONFIG VARIANT REPEATS  is such a child (EXP_EMA_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
REPLAYS = 40            # of the captured step per timed repeat
DECAY = 0.999
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def one_step(name, variant, repeats):
    import torch
    from exp_clipbank import configuration
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    x, y, _ = next(iter(bank.loader(batch)))
    x, y = nfp._clip(x), nfp._clip(y)
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    if variant == 'ema':
        nfp.set_ema(DECAY)
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
    n = sum(p.numel() for p in nfp.model.parameters())
    print('RESULT ' + json.dumps({'what': what, 'us': us, 'loss': float(loss), 'params': n, 'flat': nfp.flat is not None,
                                  'peak': torch.cuda.max_memory_allocated(), 'updates': nfp.ema.updates if variant == 'ema' else None}))


def one_epoch(name, variant, repeats):
    import torch
    from exp_clipbank import configuration
    from exp_validation import Clock, Stamped
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    clock = nfp.writer = Clock()
    kw = {} if variant == 'none' else dict(ema=DECAY, ema_eval=variant == 'ema_eval')
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        nfp.train(bank.loader(batch), Stamped(bank.loader(batch), clock), None, n_epochs=1 + repeats, mask=mask, truncated_backprop=0,
                  use_graph=True, test_graph=True, **kw)
    except ValueError as e:         # (train()'s own guards on the test loss: 'NaN loss :(' and 'Diverged :(' above 4)
        sys.stdout = so
        print('RESULT ' + json.dumps({'what': what, 'refused': f'{e} after {len(nfp.test_loss)} epochs'}))
        return
    finally:
        sys.stdout = so
    print('RESULT ' + json.dumps({'what': what, 'steps': len(bank.loader(batch)), 'train': nfp.train_loss[-1], 'test': nfp.test_loss[-1],
                                  'epoch_ms': [(b - a) * 1e3 for a, b in zip(clock.ends, clock.ends[1:])],
                                  'test_ms': [(e - b) * 1e3 for b, e in zip(clock.begins[1:], clock.ends[1:])],
                                  'peak': torch.cuda.max_memory_allocated()}))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_EMA_ROOT=root)
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
    ms = lambda v: f'{med(v):8.2f} ms ({min(v):.2f}-{max(v):.2f})'
    emit(f'python tools/exp_ema.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; median (min-max) of {repeats}; decay {DECAY}')
    for name in configs:
        steps = {}
        for variant, root in (('parent', parent), ('none', HERE), ('ema', HERE)):
            if root:
                steps[variant] = child(os.path.abspath(root), 'step', name, variant, repeats)
        first = steps['none']
        emit(f'{name}: {first["what"]}, train mode; {first["params"]} parameters, '
             + ('one flat vector (FlatAdam)' if first['flat'] else 'a parameter list (torch Adam)'))
        for variant, rec in steps.items():
            emit(f'{name}: captured step, {REPLAYS} replays a repeat  {variant:<7} {us(rec["us"])} a step   last loss {rec["loss"]:.8f}   '
                 f'peak device memory {rec["peak"]} bytes')
        none, ema = steps['none'], steps['ema']
        if parent:
            par = steps['parent']
            inside = min(par['us']) <= med(none['us']) <= max(par['us']) or min(none['us']) <= med(par['us']) <= max(none['us'])
            emit(f'{name}: ema=None / parent: {med(none["us"]) / med(par["us"]):.4f} x; the medians lie '
                 + ('inside' if inside else 'OUTSIDE') + ' the min-max of the other\'s repeats; the losses are '
                 + ('equal' if none['loss'] == par['loss'] else 'NOT equal'))
        emit(f'{name}: ema={DECAY} - ema=None: {med(ema["us"]) - med(none["us"]):+.1f} us a step, {med(ema["us"]) / med(none["us"]):.4f} x '
             f'({ema["updates"]} updates counted); the losses are ' + ('equal' if ema['loss'] == none['loss'] else 'NOT equal')
             + f'; peak device memory {ema["peak"] - none["peak"]:+d} bytes (the shadow: {4 * first["params"]} bytes)')
        epochs = {v: child(HERE, 'epoch', name, v, repeats) for v in ('none', 'ema_only', 'ema_eval')}
        refused = {v: rec['refused'] for v, rec in epochs.items() if 'refused' in rec}
        for variant, why in refused.items():
            emit(f'{name}: epoch of train(use_graph=True, test_graph=True)  {variant:<9} NOT MEASURED: train() ended with ValueError({why!r}), '
                 "its guard on the test loss of the weights it evaluates")
        if refused:
            continue
        for variant, rec in epochs.items():
            emit(f'{name}: epoch of train(use_graph=True, test_graph=True), {rec["steps"]} steps + {rec["steps"]} test batches  {variant:<9} '
                 f'epoch {ms(rec["epoch_ms"])}   test pass {ms(rec["test_ms"])}   last epoch train {rec["train"]:.8f} test {rec["test"]:.8f}   '
                 f'peak device memory {rec["peak"]} bytes')
        a, b, c = epochs['none'], epochs['ema_only'], epochs['ema_eval']
        emit(f'{name}: ema_eval=True - ema_eval=False: test pass {1e3 * (med(c["test_ms"]) - med(b["test_ms"])):+.1f} us (two parameter copies and '
             f'the division), epoch {med(c["epoch_ms"]) / med(b["epoch_ms"]):.4f} x; ema / no ema: epoch {med(b["epoch_ms"]) / med(a["epoch_ms"]):.4f} x; '
             f'train losses ' + ('equal' if a['train'] == b['train'] == c['train'] else 'NOT equal')
             + f'; test loss of the live weights {a["test"]:.8f}, of the averaged {c["test"]:.8f}; peak device memory with the average and '
             f'its stash {c["peak"] - a["peak"]:+d} bytes')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_EMA_ROOT', HERE)
        for p in (os.path.join(HERE, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        (one_step if a[0] == 'step' else one_epoch)(a[1], a[2], int(a[3]))
    else:
        main()
