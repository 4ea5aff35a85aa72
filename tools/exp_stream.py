"""Time, peak memory and what still grows per output step under set_recompute('stream') (profiles/stream.txt).  Two configurations:
    bench   bench.py's: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers, 32 clips
    ice256  the 256 x 256 sea-ice configuration of tools/bench_configs.py (cfg5): 5 channels, 12 in / 12 out, hidden 32, 1 layer,
            3 conv layers, land mask, 4 clips
and per configuration, every variant a process of its own (a fresh allocator for every memory figure) under its own time limit:
    plain / step / stream  make_graphed_step captured under None / 'step' / 'stream' on this tree: the replay time, median (min-max)
                           of --repeats replays after two untimed ones, host clock around a replay that ends in a synchronise; and
                           torch.cuda.max_memory_allocated of the process (warm-up steps, capture and replays)
    parent plain / step    with --parent DIR (a checkout of the parent commit with the built library copied in): the same two there
    horizon                the three peaks and times with output_timesteps x2 and x4, and the growth per output step of every mode
    held                   what a 'stream' pass holds when its forward ends, by kind, eager in static mode (the capture's shapes):
                           at x1 and x2 the output steps, and the difference per output step
    long                   (ice256 only) 10 in / 90 out as the sea-ice scripts roll out, at the first of 16, 8, 4 clips that 'stream'
                           holds, then 'step' once at that clip count

    python tools/exp_stream.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG MODE T_OUT_FACTOR REPEATS [CLIPS T_IN T_OUT]  and  --held CONFIG FACTOR  are
such children (EXP_STREAM_ROOT in their environment: the tree they import)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
MODES = {'plain': None, 'step': 'step', 'stream': 'stream'}
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def configuration(name, factor, clips=None, t_in=None, t_out=None):
    """(predictor, mask, (x, y, concat) on the device, description) with output_timesteps = factor x the configuration's (or the
    clip count and step counts given)."""
    import numpy as np
    import torch
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    dev = torch.device('cuda', 0)
    torch.manual_seed(1)
    if name == 'bench':
        import bench
        clips, t_in, t_out = clips or 32, t_in or bench.T_IN, t_out or bench.T_OUT * factor
        shape, mask = bench.CANVAS, np.zeros(bench.CANVAS, dtype=bool)
        nfp = NextFramePredictorS2S(thresh=bench.THRESH, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                                    model_kwargs=dict(hidden_size=bench.HIDDEN, dropout=bench.DROPOUT, n_layers=bench.N_LAYERS))
        x, y = synthetic.make_batch(2, 0, clips, t_in, t_out, n_digits=bench.N_DIGITS, pixel_noise=bench.NOISE, canvas=shape)
        what = f'64 x 64, {clips} clips, {t_in} in / {t_out} out, hidden {bench.HIDDEN}, {bench.N_LAYERS} layers'
    else:
        clips, t_in, t_out, shape = clips or 4, t_in or 12, t_out or 12 * factor, (256, 256)
        tf = lambda a: abs(abs(a - 0.5) - 0.5)
        mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]
        nfp = NextFramePredictorS2S(thresh=0.15, input_features=5, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                                    transform_func=tf, model_kwargs=dict(hidden_size=32, dropout=0.1, n_layers=1, n_conv_layers=3,
                                                                         transform_func=tf))
        base = synthetic.make_ice_like(0, shape=shape, channels=5, n_frames=min(t_in + t_out, 48))[0]
        # (the generator's cost grows with the frame count: a long clip repeats its first 48 frames, shifted per clip)
        cs = [np.concatenate([np.roll(base, c, axis=1)] * (1 + (t_in + t_out) // len(base)))[:t_in + t_out] for c in range(clips)] \
            if t_in + t_out > 48 else \
            [synthetic.make_ice_like(c, shape=shape, channels=5, n_frames=t_in + t_out)[0] for c in range(clips)]
        x, y = np.stack([c[:t_in] for c in cs]), np.stack([c[t_in:, ..., :1] for c in cs])
        what = f'256 x 256 masked, {clips} clips, 5 channels, {t_in} in / {t_out} out, hidden 32, 1 layer, 3 conv layers'
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.zeros(clips, t_out, *shape, 1, device=dev))
    nfp.initiate_training(lr=1e-3, lr_decay=0.95, capturable=True)
    nfp.model.train()
    return nfp, mask, batch, what


def one(name, mode, factor, repeats, shape=()):
    import torch
    try:
        nfp, mask, batch, what = configuration(name, factor, *shape)
        if MODES[mode] is not None:
            nfp.set_recompute(MODES[mode])
        step = nfp.make_graphed_step(*batch, mask=mask, warmup=2)
        ms, losses = [], []
        for r in range(2 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step(*batch)
            torch.cuda.synchronize()
            if r >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
            losses.append(float(loss))
        rec = {'what': what, 'ms': ms, 'peak': torch.cuda.max_memory_allocated(), 'loss': losses[-1]}
    except torch.cuda.OutOfMemoryError:
        rec = {'peak': None}
    print('RESULT ' + json.dumps(rec))


def held(name, factor):
    """What a 'stream' pass holds when its forward ends: the bytes autograd saved in the first pass (the step nodes' inputs, by
    kind; what the operations between the nodes saved), the meshes of the rollout, and the allocator's own count."""
    import torch
    from qtmpnn import recompute
    from qtmpnn.mesh import Mesh
    nfp, mask, (x, y, concat), what = configuration(name, factor)
    nfp.set_recompute('stream')
    nfp.model.static_shapes = True
    dev = x.device

    def tensors_of(obj, out):
        vals = obj.values() if isinstance(obj, dict) else obj if isinstance(obj, (list, tuple)) else ()
        if torch.is_tensor(obj):
            out.append(obj)
        for v in vals:
            tensors_of(v, out)
        return out

    def unique_bytes(ts, seen):
        n = 0
        for t in ts:
            if t.is_cuda and t.untyped_storage().data_ptr() not in seen:
                seen.add(t.untyped_storage().data_ptr())
                n += t.untyped_storage().nbytes()
        return n
    for warm in range(2):               # (the plans, the flat buffer, the optimiser state: none of it is the rollout's)
        nfp.train_step(x, y, concat, mask)
    nfp.zero_grad()
    torch.cuda.synchronize()
    seen, kinds = set(), {}
    params = {p.untyped_storage().data_ptr() for p in nfp.model.parameters()}
    h = nfp.model.hidden_size

    def pack(t):
        if t.is_cuda and not recompute.replaying() and t.untyped_storage().data_ptr() not in params:
            if t.dim() == 2 and t.shape[1] == h:
                kind = f'saved rows (N, {h}): hidden / cell at the step boundaries'
            elif t.dim() == 2:
                kind = f'saved rows (N, {t.shape[1]}): step inputs, outputs, pooled columns'
            else:
                kind = f'saved {t.dim()}-d tensors: dropout slices, index maps, weights of the pass'
            kinds[kind] = kinds.get(kind, 0) + unique_bytes([t], seen)
        return t
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        outs, meshes = nfp.model(x, y, concat, teacher_forcing_ratio=0, mask=mask)
    mesh_ts = []
    for m in {id(m): m for m in meshes}.values():
        assert isinstance(m, Mesh)
        for v in vars(m).values():
            tensors_of(v, mesh_ts)
    kinds['meshes of the rollout (labels, cells, CSR, ELL, tails, maps between meshes)'] = unique_bytes(mesh_ts, set())
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    from model.mpnnlstm import masked_mse
    loss = masked_mse(outs, meshes, y, mask)
    loss.backward()
    torch.cuda.synchronize()
    rec = {'what': what, 'kinds': kinds, 'forward_holds': after - before, 'peak_over_forward_end': torch.cuda.max_memory_allocated() - after,
           't_out': nfp.output_timesteps}
    print('RESULT ' + json.dumps(rec))


def child(root, flag, *args):
    """Run this file with `flag` `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), flag, *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_STREAM_ROOT=root)
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
    mib = lambda b: 'does not fit' if b is None else f'{b / 2 ** 20:9.1f} MiB'
    med = lambda rec: float(np.median(rec['ms']))
    show = lambda rec: f'median {med(rec):8.2f} ms ({min(rec["ms"]):.2f}-{max(rec["ms"]):.2f})   peak {mib(rec["peak"])}'
    emit(f'python tools/exp_stream.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every variant a process of its own; times: one replay of the captured step, ms, '
         f'median (min-max) of {repeats} after two untimed; peak: torch.cuda.max_memory_allocated of the process')
    for name in configs:
        base = 10 if name == 'bench' else 12
        recs = {}
        for factor in (1, 2, 4):
            for mode in ('plain', 'step', 'stream'):
                rec = recs[mode, factor] = child(HERE, '--one', name, mode, factor, repeats)
                if (mode, factor) == ('plain', 1):
                    emit(f'{name}: {rec["what"]}, train mode, captured')
                emit(f'{name}: output steps x{factor} {mode:<7} {show(rec)}   loss after the replays {rec["loss"]:.8f}')
            emit(f'{name}: output steps x{factor}: stream / step: time {med(recs["stream", factor]) / med(recs["step", factor]):.3f} x, peak '
                 f'{recs["stream", factor]["peak"] / recs["step", factor]["peak"]:.3f} x;  step / plain: time '
                 f'{med(recs["step", factor]) / med(recs["plain", factor]):.3f} x;  stream / plain: time '
                 f'{med(recs["stream", factor]) / med(recs["plain", factor]):.3f} x, peak '
                 f'{recs["stream", factor]["peak"] / recs["plain", factor]["peak"]:.3f} x')
        slope = {m: (recs[m, 4]['peak'] - recs[m, 1]['peak']) / (3 * base) / 2 ** 20 for m in MODES}
        emit(f'{name}: growth per output step between x1 and x4: ' + ', '.join(f'{m} {slope[m]:.1f} MiB' for m in MODES)
             + f';  stream / step {slope["stream"] / slope["step"]:.3f} x: in the same memory stream holds '
             f'{slope["step"] / slope["stream"]:.2f} x the output steps of step')
        if parent:
            for mode in ('plain', 'step'):
                rec = child(os.path.abspath(parent), '--one', name, mode, 1, repeats)
                emit(f'{name}: parent {mode:<7} x1     {show(rec)}   loss after the replays {rec["loss"]:.8f}   '
                     f'(this tree / parent: time {med(recs[mode, 1]) / med(rec):.3f} x, peak {recs[mode, 1]["peak"] / rec["peak"]:.4f} x)')
                if mode == 'step':
                    emit(f'{name}: stream on this tree / step on the parent commit: time {med(recs["stream", 1]) / med(rec):.3f} x')
        h1, h2 = child(HERE, '--held', name, 1), child(HERE, '--held', name, 2)
        emit(f'{name}: what a stream pass holds when its forward ends (eager, static shapes), at {h1["t_out"]} and {h2["t_out"]} output '
             f'steps, and per output step:')
        for k in sorted(set(h1['kinds']) | set(h2['kinds']), key=lambda k: -h2['kinds'].get(k, 0)):
            a, b = h1['kinds'].get(k, 0), h2['kinds'].get(k, 0)
            emit(f'{name}:   {k:<82} {mib(a)} {mib(b)}   {(b - a) / base / 2 ** 20:7.2f} MiB / step')
        for k, label in (('forward_holds', 'allocated at the end of the forward over its start (all of the above, and the outputs)'),
                         ('peak_over_forward_end', 'peak of forward + backward over the end of the forward (one step replayed)')):
            emit(f'{name}:   {label:<82} {mib(h1[k])} {mib(h2[k])}   {(h2[k] - h1[k]) / base / 2 ** 20:7.2f} MiB / step')
        if name == 'ice256':
            for clips in (16, 8, 4):
                rec = child(HERE, '--one', name, 'stream', 1, 1, clips, 10, 90)
                emit(f'ice256 long: 10 in / 90 out, {clips} clips, stream: '
                     + ('does not fit' if rec['peak'] is None else f'{rec["ms"][0]:.1f} ms a step, peak {mib(rec["peak"])}'))
                if rec['peak'] is not None:
                    other = child(HERE, '--one', name, 'step', 1, 1, clips, 10, 90)
                    emit(f'ice256 long: 10 in / 90 out, {clips} clips, step:   '
                         + ('does not fit' if other['peak'] is None else f'{other["ms"][0]:.1f} ms a step, peak {mib(other["peak"])}'))
                    break


if __name__ == '__main__':
    flag = next((f for f in ('--one', '--held') if f in sys.argv), None)
    if flag:
        a = sys.argv[sys.argv.index(flag) + 1:]
        root = os.environ.get('EXP_STREAM_ROOT', HERE)
        for p in (root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        if flag == '--one':
            one(a[0], a[1], int(a[2]), int(a[3]), tuple(int(v) for v in a[4:7]))
        else:
            held(a[0], int(a[1]))
    else:
        main()
