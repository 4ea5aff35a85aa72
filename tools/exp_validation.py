"""What the test pass costs an epoch of train(use_graph=True), and what the validation keywords cost (profiles/validation.txt).
Two configurations, those of tools/exp_clipbank.py:
    bench   bench.py's model: 64 x 64, 2 digits, noise 0.05, 10 in / 10 out, hidden 16, 2 layers; 512 windows, 16 steps of 32 clips
    ice256  the 256 x 256 sea-ice configuration (cfg5): 5 channels, 12 in / 12 out, hidden 32, 1 layer, 3 conv layers, land mask;
            32 windows, 8 steps of 4 clips
each with a test loader of the training loader's size (the same ClipBank, so no loader cost on either side), and these variants,
each a process of its own under its own time limit:
    default        train(use_graph=True), no new keyword             (also run on the parent commit with --parent DIR)
    graph          ... test_graph=True
    monitor        ... monitor=Monitor(('extent',), mean IIEE of the model)
    monitor_graph  ... the same with test_graph=True
    costs          after one epoch: one improving epoch's restore_best copy and keep_best checkpoint, timed on their own
Every variant runs in two processes (two rounds over the variants) and the ratios are taken over the pooled epochs of both: a whole
process now and then runs slower than its twin.  One process runs 1 + repeats epochs; the captures fall into epoch 0.  The test loader stamps the moment its iteration begins
(after a synchronise: the last training loss has been read by then) and the writer the moment 'Loss/test' is reported, so every
later epoch gives its wall time and its test pass's.  Reported: median (min-max) over the epochs and the test pass's share.

    python tools/exp_validation.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG VARIANT REPEATS  is such a child (EXP_VALIDATION_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


class Stamped:
    """The test loader, telling when a pass over it begins."""

    def __init__(self, loader, clock):
        self.loader, self.clock, self.dataset = loader, clock, loader.dataset

    def __iter__(self):
        import torch
        torch.cuda.synchronize()
        self.clock.begins.append(time.perf_counter())
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


class Clock:
    """A SummaryWriter stand-in: train() reports 'Loss/test' once per epoch, after the test pass's value has been read."""

    def __init__(self):
        self.begins, self.ends = [], []

    def add_scalar(self, tag, value, step):
        if tag == 'Loss/test':
            import torch
            torch.cuda.synchronize()
            self.ends.append(time.perf_counter())

    def flush(self):
        pass


def one(name, variant, repeats):
    import torch
    sys.path.insert(0, os.path.join(HERE, 'tools'))
    from exp_clipbank import configuration
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, batch, what = configuration(name)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    nfp.model.train()
    nfp.initiate_training(lr=2e-4, lr_decay=0.95, capturable=True)
    clock = nfp.writer = Clock()
    kw = {}
    if variant in ('graph', 'monitor_graph'):
        kw['test_graph'] = True
    if variant.startswith('monitor'):
        from qtmpnn.validation import Monitor
        kw['monitor'] = Monitor(('extent',), lambda v: v.extent.by_lead('model')['iiee'].mean())
    epochs = 1 if variant == 'costs' else 1 + repeats
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        nfp.train(bank.loader(batch), Stamped(bank.loader(batch), clock), None, n_epochs=epochs, mask=mask, truncated_backprop=0,
                  use_graph=True, **kw)
    finally:
        sys.stdout = so
    rec = {'what': what, 'steps': len(bank.loader(batch)), 'train': nfp.train_loss[-1], 'test': nfp.test_loss[-1],
           'monitor': nfp.monitor_history[-1] if variant.startswith('monitor') else None}
    if variant == 'costs':
        state = list(nfp.model.state_dict().values())
        best = [torch.empty_like(t) for t in state]
        rec['bytes'] = sum(t.numel() * t.element_size() for t in state)

        def timed(fn):
            out = []
            for _ in range(repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return out[1:]
        rec['copy_ms'] = timed(lambda: torch._foreach_copy_(best, state))
        with tempfile.TemporaryDirectory() as d:
            rec['save_ms'] = timed(lambda: nfp.save_checkpoint(os.path.join(d, 'best.pt')))
            rec['file_bytes'] = os.path.getsize(os.path.join(d, 'best.pt'))
    else:
        rec['epoch_ms'] = [(b - a) * 1e3 for a, b in zip(clock.ends, clock.ends[1:])]
        rec['test_ms'] = [(e - b) * 1e3 for b, e in zip(clock.begins[1:], clock.ends[1:])]
    print('RESULT ' + json.dumps(rec))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_VALIDATION_ROOT=root)
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
    span = lambda v: f'{med(v):8.2f} ms ({min(v):.2f}-{max(v):.2f})'
    show = lambda rec: (f'epoch {span(rec["epoch_ms"])}   test pass {span(rec["test_ms"])} = {100 * med(rec["test_ms"]) / med(rec["epoch_ms"]):5.1f} % '
                        f'of the epoch   last epoch train {rec["train"]:.8f} test {rec["test"]:.8f}'
                        + (f' monitor {rec["monitor"]:.6f}' if rec['monitor'] is not None else ''))
    emit(f'python tools/exp_validation.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; train(use_graph=True) of {1 + repeats} epochs over a '
         f'ClipBank loader, the test loader of the same size; times: wall time after the epoch of the captures, ms, median (min-max) of {repeats}')
    for name in configs:
        # two rounds, so that every variant is measured in two processes: a whole process now and then runs slower than its twin
        # (seen on the parent commit as on this one), and a ratio must not rest on one of those
        runs = []
        for round_ in (1, 2):
            if parent:
                runs.append(('parent', 'default', child(os.path.abspath(parent), name, 'default', repeats)))
            for variant in ('default', 'graph', 'monitor', 'monitor_graph'):
                runs.append(('this commit', variant, child(HERE, name, variant, repeats)))
        first = runs[0][2]
        emit(f'{name}: {first["what"]}, train mode; {first["steps"]} training steps and {first["steps"]} test batches an epoch')
        for tree, variant, rec in runs:
            emit(f'{name}: {tree:<12} {variant:<14} {show(rec)}')
        pool = lambda tree, variant, key: [m for t, v, rec in runs if (t, v) == (tree, variant) for m in rec[key]]
        last = lambda tree, variant: {(rec['train'], rec['test'], rec['monitor']) for t, v, rec in runs if (t, v) == (tree, variant)}
        ep = {v: pool('this commit', v, 'epoch_ms') for v in ('default', 'graph', 'monitor', 'monitor_graph')}
        tp = {v: pool('this commit', v, 'test_ms') for v in ep}
        emit(f'{name}: pooled over the two processes of a variant ({len(ep["default"])} epochs each): '
             + '; '.join(f'{v} epoch {span(ep[v]).strip()} test pass {span(tp[v]).strip()}' for v in ep))
        if parent:
            par, part = pool('parent', 'default', 'epoch_ms'), pool('parent', 'default', 'test_ms')
            emit(f'{name}: parent, pooled: epoch {span(par).strip()} test pass {span(part).strip()} = {100 * med(part) / med(par):.1f} % of the epoch')
            emit(f'{name}: default / parent: epoch {med(ep["default"]) / med(par):.4f} x, test pass {med(tp["default"]) / med(part):.4f} x; the losses are '
                 + ('equal' if len(last('this commit', 'default') | last('parent', 'default')) == 1 else 'NOT equal'))
        same = lambda a, b, i: len({r[i] for r in last('this commit', a) | last('this commit', b)}) == 1
        emit(f'{name}: test_graph=True / default: epoch {med(ep["graph"]) / med(ep["default"]):.3f} x, test pass '
             f'{med(tp["graph"]) / med(tp["default"]):.3f} x; the test losses are ' + ('equal' if same('graph', 'default', 1) else 'NOT equal'))
        emit(f'{name}: Monitor((extent,)) / default: epoch {med(ep["monitor"]) / med(ep["default"]):.3f} x eager, '
             f'{med(ep["monitor_graph"]) / med(ep["default"]):.3f} x with test_graph=True; the monitored values are '
             + ('equal' if same('monitor', 'monitor_graph', 2) else 'NOT equal'))
        c = child(HERE, name, 'costs', repeats)
        emit(f'{name}: an improving epoch: restore_best copies {c["bytes"]} bytes in {span(c["copy_ms"])}; keep_best writes '
             f'{c["file_bytes"]} bytes in {span(c["save_ms"])}')

if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_VALIDATION_ROOT', HERE)
        for p in (root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one(a[0], a[1], int(a[2]))
    else:
        main()
