"""What a selection of trainable parameters (set_trainable, train(trainable=)) costs and saves (profiles/finetune.txt).  The two
configurations of tools/exp_clipbank.py:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, 32 clips a step
    ice256  the 256 x 256 sea-ice configuration: 5 channels, 12 in / 12 out, hidden 32, 1 layer, 3 conv layers, land mask, 4 clips
and one measurement, each variant a process of its own under its own time limit: the captured training step
(make_graphed_step, clipping at 10) replayed on one batch, REPLAYS replays between two synchronisations, timed `repeats` times
-> us per step, median (min-max), the last loss and the peak device memory of the process.  Variants:
    parent    with --parent DIR, the parent commit's tree (which has no selection): the plain step
    none      this tree, no selection set (trainable=None)
    decoder   set_trainable(('decoder.*',)): the encoder is frozen and its phase runs without autograd (the encoder cut)
    masking   set_trainable(('decoder.*', 'encoder.norm_h.*')): two encoder tensors stay trainable, so the whole rollout keeps its
              graph and only the mask multiplication is added

    python tools/exp_finetune.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG VARIANT REPEATS  is such a child (EXP_FINETUNE_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
REPLAYS = 40            # of the captured step per timed repeat
SELECTIONS = {'decoder': ('decoder.*',), 'masking': ('decoder.*', 'encoder.norm_h.*')}
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
    if variant in SELECTIONS:
        nfp.set_trainable(SELECTIONS[variant])
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
    trainable = len(nfp.trainable_names) if variant != 'parent' else len(list(nfp.model.parameters()))
    print('RESULT ' + json.dumps({'what': what, 'us': us, 'loss': float(loss), 'peak': torch.cuda.max_memory_allocated(),
                                  'trainable': trainable, 'tensors': len(list(nfp.model.parameters())),
                                  'cut': bool(getattr(nfp.model, 'encoder_cut', False))}))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_FINETUNE_ROOT=root)
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
    emit(f'python tools/exp_finetune.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; captured step, {REPLAYS} replays a repeat, median '
         f'(min-max) of {repeats}')
    for name in configs:
        steps = {}
        for variant, root in [('parent', parent), ('none', HERE), ('decoder', HERE), ('masking', HERE)]:
            if root:
                steps[variant] = child(os.path.abspath(root), name, variant, repeats)
        none = steps['none']
        emit(f'{name}: {none["what"]}, train mode')
        for variant, rec in steps.items():
            said = {'parent': 'parent commit, plain step', 'none': 'trainable=None', 'decoder': f'trainable={SELECTIONS["decoder"]}',
                    'masking': f'trainable={SELECTIONS["masking"]}'}[variant]
            emit(f'{name}: {said:<55} {rec["trainable"]:3d} of {rec["tensors"]} tensors trainable, encoder cut '
                 f'{"on " if rec["cut"] else "off"}  {us(rec["us"])} a step   last loss {rec["loss"]:.8f}   peak device memory '
                 f'{rec["peak"]} bytes')
        if parent:
            par = steps['parent']
            inside = min(par['us']) <= med(none['us']) <= max(par['us'])
            emit(f'{name}: trainable=None / parent: {med(none["us"]) / med(par["us"]):.4f} x; the median lies '
                 + ('inside' if inside else 'OUTSIDE') + f' the min-max of the parent\'s repeats ({min(par["us"]):.1f}-{max(par["us"]):.1f} us); '
                 'the losses are ' + ('equal' if none['loss'] == par['loss'] else 'NOT equal') + f'; peak {none["peak"] - par["peak"]:+d} bytes')
        for variant in ('decoder', 'masking'):
            rec = steps[variant]
            emit(f'{name}: {variant} / trainable=None: {med(rec["us"]) / med(none["us"]):.4f} x the step time, '
                 f'{rec["peak"] / none["peak"]:.4f} x the peak device memory ({(rec["peak"] - none["peak"]) / 2 ** 20:+.1f} MiB); the '
                 'first losses of the runs differ by what was trained, the last loss is reported above')
    emit('not measured: eager steps, the 90-step rollout, several ranks, the parameter-list form (MHTransformerConv)')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_FINETUNE_ROOT', HERE)
        for p in (os.path.join(HERE, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one_step(a[0], a[1], int(a[2]))
    else:
        main()
