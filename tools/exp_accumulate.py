"""Time and peak memory of gradient accumulation on one GPU (profiles/accumulate.txt).  Two configurations:
    bench   bench.py's: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, micro-batches of 32 clips
    ice256  the 256 x 256 sea-ice configuration of tools/bench_configs.py (cfg5): 5 channels, 12 in / 12 out, hidden 32, 1 layer,
            3 conv layers, land mask, micro-batches of 4 clips
and per configuration
    time    one graphed accumulated step (make_graphed_step(accumulate=k)) of k micro-batches, k = 1 (today's single graph), 2, 4,
            against k replays of the single graphed step, and, with --parent FILE (the parent commit's model/mpnnlstm.py, e.g. from
            `git show HEAD~1:quadtree-mpnnlstm_amd/model/mpnnlstm.py`), against k replays of that file's single graphed step on the
            same weights in the same process; the update graph alone; median (min-max) of --repeats repeats, host clock around work
            that ends in a synchronise, the order of the variants rotating.  Recorded, not asserted: time ~ k * (step - update) + update
    memory  torch.cuda.max_memory_allocated of a process that captures and replays an accumulated step of k micro-batches of B
            clips, against a process that captures and replays one step on k * B clips (where that fits).  Recorded, not asserted:
            the accumulated step's peak ~ that of one micro-batch

    python tools/exp_accumulate.py [--repeats 7] [--parent FILE] [--commit TEXT] [--out profiles/accumulate.txt]
runs every measurement as a child process of its own (a fresh allocator for every memory figure) under a time limit, one after
the other, and stops at the first that fails;  --one CONFIG time | --one CONFIG memory acc|big K  is such a child."""
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quadtree-mpnnlstm_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
KS = (1, 2, 4)
LIMIT_S = 240           # per child process
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def configuration(name, clips, n_batches, cls):
    """(predictor of class cls, mask, [n_batches batches (x, y, concat) of `clips` clips on the device], description)."""
    import numpy as np
    import torch
    from qtmpnn import synthetic
    dev = torch.device('cuda', 0)
    torch.manual_seed(1)
    if name == 'bench':
        import bench
        t_in, t_out, shape, mask = bench.T_IN, bench.T_OUT, bench.CANVAS, np.zeros(bench.CANVAS, dtype=bool)
        nfp = cls(thresh=bench.THRESH, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                  model_kwargs=dict(hidden_size=bench.HIDDEN, dropout=bench.DROPOUT, n_layers=bench.N_LAYERS))
        batch = lambda i: synthetic.make_batch(2, i * clips, clips, t_in, t_out, n_digits=bench.N_DIGITS, pixel_noise=bench.NOISE,
                                               canvas=shape)
        what = f'64 x 64, {t_in} in / {t_out} out, hidden {bench.HIDDEN}, {bench.N_LAYERS} layers'
    else:
        t_in, t_out, shape = 12, 12, (256, 256)
        tf = lambda a: abs(abs(a - 0.5) - 0.5)
        mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]
        nfp = cls(thresh=0.15, input_features=5, input_timesteps=t_in, output_timesteps=t_out, device=dev, transform_func=tf,
                  model_kwargs=dict(hidden_size=32, dropout=0.1, n_layers=1, n_conv_layers=3, transform_func=tf))

        def batch(i):
            cs = [synthetic.make_ice_like(1000 * i + c, shape=shape, channels=5, n_frames=t_in + t_out)[0] for c in range(clips)]
            return np.stack([c[:t_in] for c in cs]), np.stack([c[t_in:, ..., :1] for c in cs])
        what = f'256 x 256 masked, 5 channels, {t_in} in / {t_out} out, hidden 32, 1 layer, 3 conv layers'
    pool = []
    for i in range(n_batches):
        x, y = batch(i)
        pool.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.zeros(clips, t_out, *shape, 1, device=dev)))
    nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=True)
    nfp.model.train()
    return nfp, mask, pool, what


def parent_class(path):
    spec = importlib.util.spec_from_file_location('parent_mpnnlstm', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.NextFramePredictorS2S


def one_time(name, clips, repeats, parent_path):
    import numpy as np
    import torch
    from model.mpnnlstm import NextFramePredictorS2S
    ways, mask, pool, what, state, update = {}, None, None, None, None, None
    for k in KS:
        nfp, mask, pool, what = configuration(name, clips, max(KS), NextFramePredictorS2S)
        if state is None:
            state = {n: v.clone() for n, v in nfp.model.state_dict().items()}
        nfp.model.load_state_dict(state)
        if k == 1:
            single = nfp.make_graphed_step(*pool[0], mask=mask, warmup=2)
            for j in KS:
                ways[f'single x{j}'] = lambda j=j, single=single: [single(*pool[i]) for i in range(j)]
        else:
            step = nfp.make_graphed_step(*pool[0], mask=mask, warmup=2, accumulate=k)
            ways[f'accumulate={k}'] = lambda k=k, step=step: step(pool[:k])
            update = step.graphs[1]
    if parent_path:
        old, _, _, _ = configuration(name, clips, 1, parent_class(parent_path))
        old.model.load_state_dict(state)
        parent = old.make_graphed_step(*pool[0], mask=mask, warmup=2)
        for j in KS:
            ways[f'parent x{j}'] = lambda j=j: [parent(*pool[i]) for i in range(j)]
    order, ms = list(ways), {w: [] for w in ways}
    for r in range(2 + repeats):            # (two untimed rounds first)
        for w in order[r % len(order):] + order[:r % len(order)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ways[w]()
            torch.cuda.synchronize()
            if r >= 2:
                ms[w].append((time.perf_counter() - t0) * 1e3)
    upd = []
    for r in range(2 + repeats):            # (last: replayed alone it steps Adam on a zero gradient)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        update.replay()
        torch.cuda.synchronize()
        if r >= 2:
            upd.append((time.perf_counter() - t0) * 1e3)
    ms['update graph alone'] = upd
    print('RESULT ' + json.dumps({'what': what, 'clips': clips, 'ms': ms}))


def one_memory(name, clips, mode, k):
    import torch
    from model.mpnnlstm import NextFramePredictorS2S
    try:
        if mode == 'acc':
            nfp, mask, pool, what = configuration(name, clips, k, NextFramePredictorS2S)
            step = nfp.make_graphed_step(*pool[0], mask=mask, warmup=1, accumulate=k)
            losses = [float(step(pool) if k > 1 else step(*pool[0])) for _ in range(2)]
        else:
            nfp, mask, pool, what = configuration(name, clips * k, 1, NextFramePredictorS2S)
            step = nfp.make_graphed_step(*pool[0], mask=mask, warmup=1)
            losses = [float(step(*pool[0])) for _ in range(2)]
        torch.cuda.synchronize()
        rec = {'peak': torch.cuda.max_memory_allocated(), 'losses': losses}
    except torch.cuda.OutOfMemoryError:
        rec = {'peak': None}
    print('RESULT ' + json.dumps(rec))


def child(*args):
    """Run this file with --one `args` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))))
    res = subprocess.run(cmd, capture_output=True, text=True, env=env)
    recs = [line[7:] for line in res.stdout.splitlines() if line.startswith('RESULT ')]
    if res.returncode != 0 or len(recs) != 1:
        sys.exit(f'{" ".join(cmd)} ended with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}')
    return json.loads(recs[0])


def main():
    import numpy as np
    repeats, parent_path, commit, out_path = arg('--repeats', 7, int), arg('--parent', None), arg('--commit', 'unknown'), arg('--out', None)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f'python tools/exp_accumulate.py --repeats {repeats}' + (' --parent <parent mpnnlstm.py>' if parent_path else '')
         + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every measurement a process of its own; times: ms, median (min-max) of {repeats} '
         'repeats after two untimed rounds, the order of the variants rotating')
    for name, clips in (('bench', 32), ('ice256', 4)):
        rec = child(name, 'time', clips, repeats, *( [parent_path] if parent_path else []))
        ms = rec['ms']
        med = {w: float(np.median(v)) for w, v in ms.items()}
        emit(f'{name}: {rec["what"]}, micro-batches of {clips} clips, train mode, graphed')
        for w, v in ms.items():
            emit(f'{name}: time   {w:<20} median {med[w]:8.2f} ms ({min(v):.2f}-{max(v):.2f})')
        step, upd = med['single x1'], med['update graph alone']
        for k in KS[1:]:
            emit(f'{name}: time   accumulate={k}: {med[f"accumulate={k}"]:.2f} ms; k x (step - update) + update = {k} x ({step:.2f} - '
                 f'{upd:.2f}) + {upd:.2f} = {k * (step - upd) + upd:.2f} ms; k single steps {med[f"single x{k}"]:.2f} ms'
                 + (f', of the parent commit {med[f"parent x{k}"]:.2f} ms' if parent_path else ''))
        base = None
        for k in KS:
            acc = child(name, 'memory', clips, 'acc', k)['peak']
            big = acc if k == 1 else child(name, 'memory', clips, 'big', k)['peak']
            base = acc if base is None else base
            mib = lambda b: 'does not fit' if b is None else f'{b / 2 ** 20:9.1f} MiB'
            emit(f'{name}: memory k = {k}: accumulated step of {k} x {clips} clips {mib(acc)} ({acc / base:.2f} x one micro-batch\'s); '
                 f'one step on {k * clips} clips {mib(big)}' + ('' if big is None else f' ({big / base:.2f} x)'))
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if '--one' in sys.argv:
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        a = sys.argv[sys.argv.index('--one') + 1:]
        if a[1] == 'time':
            one_time(a[0], int(a[2]), int(a[3]), a[4] if len(a) > 4 else None)
        else:
            one_memory(a[0], int(a[2]), a[3], int(a[4]))
    else:
        main()
