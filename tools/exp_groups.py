"""What parameter groups (set_param_groups, train(param_groups=)) cost, and how close the grouped step stays to its float64 model
(profiles/groups.txt).  The two configurations of tools/exp_clipbank.py:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, 32 clips a step
    ice256  the 256 x 256 sea-ice configuration: 5 channels, 12 in / 12 out, hidden 32, 1 layer, 3 conv layers, land mask, 4 clips
and one measurement, each variant a process of its own under its own time limit: the captured training step
(make_graphed_step, clipping at 10) replayed on one batch, REPLAYS replays between two synchronisations, timed `repeats` times
-> us per step, median (min-max), the last loss and the peak device memory of the process.  Variants:
    parent    with --parent DIR, the parent commit's tree (which has no setting): the plain step
    none      this tree, no setting (param_groups=None)
    mixed     set_param_groups(MIXED): norms and biases plain, the encoder at lr_scale 0.1 with decay 1e-2, the rest with decay 1e-2
              (it trains another model: the predicted frames, hence the decoder's meshes and the work of a step, differ)
    launches  set_param_groups(LAUNCHES): every entry at lr_scale 1 - 2^-24 and decay 1e-30 -- all eight launches run on every entry,
              the decay factor rounds to 1 and the blend moves an update by at most its last bit, so the model trained, and with it
              the meshes, stay the plain run's: the cost of the mechanism alone
With --bounds the four tiny models of tests/test_gpu_groups.py run its case (b) in one more process and the worst
|device - float64 model| / bound of parameters, first and second moments over its three steps is recorded per convolution type.

    python tools/exp_groups.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--bounds] [--out FILE]
stops at the first child that fails;  --one CONFIG VARIANT REPEATS  is such a child (EXP_GROUPS_ROOT: the tree it imports)."""
import json
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
REPLAYS = 40            # of the captured step per timed repeat
MIXED = [('*norm*', {}), ('*bias*', {}), ('encoder.*', dict(lr_scale=0.1, weight_decay=1e-2)), ('*', dict(weight_decay=1e-2))]
LAUNCHES = [('*', dict(lr_scale=1.0 - 2.0 ** -24, weight_decay=1e-30))]
SETTINGS = {'mixed': MIXED, 'launches': LAUNCHES}
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def one_step(name, variant, repeats):
    import torch
    from exp_clipbank import Windows, configuration
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    windows = Windows(series, times, t_in, t_out, yc)           # (this file's own windows: the same batch on either tree)
    x = torch.from_numpy(windows.x[:batch]).to(nfp.device)
    y = torch.from_numpy(windows.y[:batch]).to(nfp.device)
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    if variant in SETTINGS:
        nfp.set_param_groups(SETTINGS[variant])
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
    kinds = {}
    if variant == 'mixed':
        for k, v in nfp.param_group_table.items():
            kinds[str(v)] = kinds.get(str(v), 0) + 1
    print('RESULT ' + json.dumps({'what': what, 'us': us, 'loss': float(loss), 'peak': torch.cuda.max_memory_allocated(),
                                  'floats': n, 'tensors': len(list(nfp.model.parameters())), 'kinds': kinds}))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_GROUPS_ROOT=root)
    res = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [line[7:] for line in res.stdout.splitlines() if line.startswith('RESULT ')]
    if res.returncode != 0 or len(recs) != 1:
        sys.exit(f'{" ".join(cmd)} ended with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}')
    return json.loads(recs[0])


def bounds():
    """tests/test_gpu_groups.py's case (b) in a process of its own -> {conv: (p, m, v) worst ratios}."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, '-m', 'pytest', os.path.join(HERE, 'tests', 'test_gpu_groups.py'), '-q', '-s',
           '-m', 'gpu', '-k', 'float64_bound', '-p', 'no:cacheprovider']
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=HERE)
    found = re.findall(r'RATIO (\w+) (\S+) (\S+) (\S+)', res.stdout)
    if res.returncode != 0 or not found:
        sys.exit(f'{" ".join(cmd)} ended with {res.returncode}:\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}')
    return {conv: (float(p), float(m), float(v)) for conv, p, m, v in found}


def main():
    import numpy as np
    repeats, parent, commit, out_path = arg('--repeats', 7, int), arg('--parent', None), arg('--commit', 'unknown'), arg('--out', None)
    configs = [c for c in arg('--configs', 'bench,ice256').split(',') if c]
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            with open(out_path, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
    med = lambda v: float(np.median(v))
    us = lambda v: f'{med(v):9.1f} us ({min(v):.1f}-{max(v):.1f})'
    emit(f'python tools/exp_groups.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}' + (' --bounds' if '--bounds' in sys.argv else ''))
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; captured step, {REPLAYS} replays a repeat, median '
         f'(min-max) of {repeats}')
    emit(f'mixed: param_groups={MIXED}')
    emit(f'launches: param_groups={LAUNCHES} (all eight launches on every entry, the trajectory the plain one to the last bit of an update)')
    for name in configs:
        steps = {}
        for variant, root in [('parent', parent), ('none', HERE), ('mixed', HERE), ('launches', HERE)]:
            if root:
                steps[variant] = child(os.path.abspath(root), name, variant, repeats)
        none, mixed = steps['none'], steps['mixed']
        emit(f'{name}: {none["what"]}, train mode; {none["floats"]} parameters ({4 * none["floats"]} bytes) in {none["tensors"]} tensors')
        emit(f'{name}: mixed resolves to (lr_scale, weight_decay): tensors = {mixed["kinds"]}')
        for variant, rec in steps.items():
            said = {'parent': 'parent commit, plain step', 'none': 'param_groups=None', 'mixed': 'param_groups=mixed',
                    'launches': 'param_groups=launches'}[variant]
            emit(f'{name}: {said:<28} {us(rec["us"])} a step   last loss {rec["loss"]:.8f}   peak device memory {rec["peak"]} bytes')
        if parent:
            par = steps['parent']
            inside = min(par['us']) <= med(none['us']) <= max(par['us'])
            emit(f'{name}: param_groups=None / parent: {med(none["us"]) / med(par["us"]):.4f} x; the median lies '
                 + ('inside' if inside else 'OUTSIDE') + f' the min-max of the parent\'s repeats ({min(par["us"]):.1f}-{max(par["us"]):.1f} us)'
                 + (': did not move' if inside else '') + '; the losses are ' + ('equal' if none['loss'] == par['loss'] else 'NOT equal')
                 + f'; peak {none["peak"] - par["peak"]:+d} bytes')
        for variant in ('mixed', 'launches'):
            rec = steps[variant]
            delta = rec['peak'] - none['peak']
            emit(f'{name}: {variant} / param_groups=None: {med(rec["us"]) / med(none["us"]):.4f} x the step time '
                 f'({med(rec["us"]) - med(none["us"]):+.1f} us, as measured; no target was set); peak {delta:+d} bytes = '
                 f'{delta / (4 * none["floats"]):.2f} parameter vectors (s, nsl, work and stash: 4, and the selector: 0.25; the '
                 'allocator rounds each to 512 bytes)')
    if '--bounds' in sys.argv:
        emit('worst |device - float64 model| / derived bound over three steps (one StepLR change) of tests/test_gpu_groups.py, case (b): '
             '64 x 64, 2 clips, 2 in / 2 out, hidden 8, 2 layers; a value <= 1 keeps the bound')
        for conv, (p, m, v) in bounds().items():
            emit(f'bounds: {conv:<18} parameters {p:.4f}   exp_avg {m:.4f}   exp_avg_sq {v:.4f}')
    emit('not measured: eager steps, the 90-step rollout, several ranks, the step time of the parameter-list form (MHTransformerConv)')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_GROUPS_ROOT', HERE)
        for p in (os.path.join(HERE, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one_step(a[0], a[1], int(a[2]))
    else:
        main()
