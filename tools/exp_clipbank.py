"""What the loader costs a graphed epoch, and what the windows cost in memory (profiles/clipbank.txt).  Two configurations:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers; a series of 532 days, 512
            windows, 16 steps of 32 clips an epoch
    ice256  the 256 x 256 sea-ice configuration of tools/bench_configs.py (cfg5): 5 channels, 12 in / 12 out, hidden 32, 1 layer,
            3 conv layers, land mask, y on channel 0; a series of 56 days, 32 windows, 8 steps of 4 clips an epoch
and three loaders over the same windows in the same order (shuffle=False), each a process of its own under its own time limit:
    bank    ClipBank(series).loader(batch)                              (the series on the device, windows gathered there)
    host    DataLoader(windows materialised on the host, num_workers=0) (what the reference's IceDataset gives)
    pinned  the same with pin_memory=True
One process runs train(use_graph=True, n_epochs=1 + repeats) with a test pass of one batch; the captures fall into epoch 0, and
the wall time of every later epoch is taken between the epochs' 'Loss/test' reports (the loss has been read by then, so the
device is idle; a synchronise is made all the same).  Reported: median (min-max) of the epochs, the peak of
torch.cuda.max_memory_allocated, the host bytes of the materialised windows against bank.nbytes, the last epoch's losses.
With --parent DIR (a checkout of the parent commit with the built library copied in) the host loader also runs on that tree,
alternated with further runs on this one: this, parent, this, parent.

    python tools/exp_clipbank.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG LOADER REPEATS  is such a child (EXP_CLIPBANK_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def configuration(name):
    """(predictor, mask, series (D, W, H, C) float32, times, T_in, T_out, y channels, batch, description)."""
    import numpy as np
    import torch
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    dev = torch.device('cuda', 0)
    torch.manual_seed(1)
    if name == 'bench':
        import bench
        t_in, t_out, batch, D = bench.T_IN, bench.T_OUT, 32, 532
        mask = np.zeros(bench.CANVAS, dtype=bool)
        nfp = NextFramePredictorS2S(thresh=bench.THRESH, input_features=1, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                                    model_kwargs=dict(hidden_size=bench.HIDDEN, dropout=bench.DROPOUT, n_layers=bench.N_LAYERS))
        series = synthetic.make_clip(2000, canvas=bench.CANVAS, n_digits=bench.N_DIGITS, n_frames=D, pixel_noise=bench.NOISE)
        what = f'64 x 64, {batch} clips, {t_in} in / {t_out} out, hidden {bench.HIDDEN}, {bench.N_LAYERS} layers'
    else:
        t_in, t_out, batch, D, shape = 12, 12, 4, 56, (256, 256)
        tf = lambda a: abs(abs(a - 0.5) - 0.5)
        mask = synthetic.make_ice_like(40, shape=shape, channels=5, n_frames=2)[1]
        nfp = NextFramePredictorS2S(thresh=0.15, input_features=5, input_timesteps=t_in, output_timesteps=t_out, device=dev,
                                    transform_func=tf, model_kwargs=dict(hidden_size=32, dropout=0.1, n_layers=1, n_conv_layers=3,
                                                                         transform_func=tf))
        base = synthetic.make_ice_like(0, shape=shape, channels=5, n_frames=48)[0]
        # (the generator's cost grows with the frame count: the series runs its 48 days forth and then back)
        series = np.concatenate([base, base[::-1]])[:D]
        what = f'256 x 256 masked, {batch} clips, 5 channels, {t_in} in / {t_out} out, hidden 32, 1 layer, 3 conv layers'
    times = (np.datetime64('2012-01-01T12', 'ns') + np.arange(D) * np.timedelta64(1, 'D')).astype(np.int64)
    return nfp, mask, np.ascontiguousarray(series, dtype=np.float32), times, t_in, t_out, [0], batch, what


class Windows:
    """Every window of a series materialised on the host, as the reference's IceDataset holds them (this file's own loop: the
    parent commit has no ClipBank to ask)."""

    def __init__(self, series, times, t_in, t_out, y_channels):
        import numpy as np
        n = len(series) - t_in - t_out
        self.x = np.stack([series[i:i + t_in] for i in range(n)])
        self.y = np.stack([series[i + t_in:i + t_in + t_out][..., y_channels] for i in range(n)])
        self.launch_dates = times[t_in:t_in + n]
        self.image_shape = self.x.shape[2:4]

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], self.y[i], self.launch_dates[i]


class EpochClock:
    """A SummaryWriter stand-in: train() reports 'Loss/test' once per epoch, after the epoch's last loss has been read."""

    def __init__(self):
        self.stamps, self.test, self.train = [], [], []

    def add_scalar(self, tag, value, step):
        import torch
        if tag == 'Loss/test':
            torch.cuda.synchronize()
            self.stamps.append(time.perf_counter())
            self.test.append(value)
        else:
            self.train.append(value)

    def flush(self):
        pass


def one(name, kind, repeats):
    import torch
    from torch.utils.data import DataLoader
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    n_test = t_in + t_out + batch           # (the test pass: the first `batch` windows)
    rec = {'what': what, 'days': len(series), 'windows': len(series) - t_in - t_out}
    if kind == 'bank':
        from qtmpnn.data import ClipBank
        bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
        train = bank.loader(batch)
        test = ClipBank(series[:n_test], times[:n_test], t_in, t_out, y_channels=yc, device=nfp.device).loader(batch)
        rec['bank_bytes'] = bank.nbytes
    else:
        ds, ds_test = Windows(series, times, t_in, t_out, yc), Windows(series[:n_test], times[:n_test], t_in, t_out, yc)
        train, test = (DataLoader(d, batch_size=batch, shuffle=False, num_workers=0, pin_memory=kind == 'pinned') for d in (ds, ds_test))
        rec['host_bytes'] = ds.x.nbytes + ds.y.nbytes
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    clock = nfp.writer = EpochClock()
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        nfp.train(train, test, None, n_epochs=1 + repeats, mask=mask, truncated_backprop=0, use_graph=True)
    finally:
        sys.stdout = so
    rec.update(steps=len(train), ms=[(b - a) * 1e3 for a, b in zip(clock.stamps, clock.stamps[1:])], peak=torch.cuda.max_memory_allocated(),
               train=nfp.train_loss[-1], test=nfp.test_loss[-1])
    print('RESULT ' + json.dumps(rec))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_CLIPBANK_ROOT=root)
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
    mib = lambda b: f'{b / 2 ** 20:9.1f} MiB'
    med = lambda rec: float(np.median(rec['ms']))
    show = lambda rec: (f'epoch median {med(rec):8.2f} ms ({min(rec["ms"]):.2f}-{max(rec["ms"]):.2f}) = {med(rec) / rec["steps"]:6.2f} ms '
                        f'a step incl. the test pass   peak {mib(rec["peak"])}   last epoch train {rec["train"]:.8f} test {rec["test"]:.8f}')
    emit(f'python tools/exp_clipbank.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; train(use_graph=True) of {1 + repeats} epochs, shuffle=False, '
         f'a test pass of one batch; times: wall time of an epoch after the epoch of the captures, ms, median (min-max) of {repeats}; '
         'peak: torch.cuda.max_memory_allocated of the process')
    for name in configs:
        recs = {kind: child(HERE, name, kind, repeats) for kind in ('bank', 'host', 'pinned')}
        a, b = recs['bank'], recs['host']
        emit(f'{name}: {a["what"]}, train mode; {a["days"]} days, {a["windows"]} windows, {a["steps"]} steps an epoch')
        emit(f'{name}: windows materialised on the host (float32) {mib(b["host_bytes"])}; bank.nbytes (device) {mib(a["bank_bytes"])}: '
             f'{b["host_bytes"] / a["bank_bytes"]:.2f} x')
        for kind in ('bank', 'host', 'pinned'):
            emit(f'{name}: {kind:<7} {show(recs[kind])}')
        emit(f'{name}: bank / host: epoch {med(a) / med(b):.3f} x, peak {a["peak"] / b["peak"]:.4f} x ({mib(a["peak"] - b["peak"])} more);  '
             f'pinned / host: epoch {med(recs["pinned"]) / med(b):.3f} x;  the losses of the three are '
             + ('equal' if len({(r["train"], r["test"]) for r in recs.values()}) == 1 else 'NOT equal'))
        if parent:
            runs = [('this tree', b)]
            for tree, root in (('parent', os.path.abspath(parent)), ('this tree', HERE), ('parent', os.path.abspath(parent))):
                runs.append((tree, child(root, name, 'host', repeats)))
            for tree, rec in runs:
                emit(f'{name}: host on {tree:<9} {show(rec)}')
            this = [m for tree, rec in runs if tree == 'this tree' for m in rec['ms']]
            par = [m for tree, rec in runs if tree == 'parent' for m in rec['ms']]
            emit(f'{name}: host, this tree: median {np.median(this):.2f} ms ({min(this):.2f}-{max(this):.2f}) of {len(this)} epochs;  parent: '
                 f'median {np.median(par):.2f} ms ({min(par):.2f}-{max(par):.2f}) of {len(par)};  this / parent {np.median(this) / np.median(par):.4f} x')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_CLIPBANK_ROOT', HERE)
        for p in (root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one(a[0], a[1], int(a[2]))
    else:
        main()
