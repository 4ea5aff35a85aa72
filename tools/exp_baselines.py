"""What references= costs verify(), and whether the default call moved against the parent commit (profiles/baselines.txt).  The
two configurations of tools/exp_clipbank.py (its models, series and stamps):
    bench   64 x 64, 10 in / 10 out, hidden 16, 2 layers; 532 days, 512 windows, 32 clips a batch
    ice256  256 x 256 masked, 5 channels, 12 in / 12 out, hidden 32; 56 days, 32 windows, 4 clips a batch
Every line is a process of its own under its own time limit: verify() with its six default products over a ClipBank loader
(shuffle=False, eval mode) with normals (1, 366, W, H) of a fixed seed on the device, one untimed call and then `repeats` timed
ones, the device waited for before and after each; eager and use_graph=True (a graphed call captures its shapes anew: that is
what a call costs).  Variants:
    default   references=None
    three     ('persistence', 'climatology', 'anomaly_persistence'): two launches per product
    four      ('anomaly_persistence', 'persistence', 'climatology', AnomalyPersistence(damping=(T_out,))): the tests' list
The host time inside get_climatology_array and get_launch_climatology is summed per call (time.perf_counter around them; the
device is not waited for) and reported per batch for the first call and for the later ones.
--parent DIR (a checkout of the parent commit with the built library copied in): the default variant is also run on that tree,
alternated with this tree's: this, parent, this, parent.

    python tools/exp_baselines.py [--configs bench,ice256] [--repeats 7] [--parent DIR] [--commit TEXT] [--out FILE]
stops at the first child that fails;  --one CONFIG VARIANT GRAPH REPEATS  is such a child (EXP_BASE_ROOT: the tree it imports)."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 280           # per child process
arg = lambda flag, default, kind=str: kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def one(name, variant, graph, repeats):
    import numpy as np
    import torch
    import exp_clipbank
    from qtmpnn.data import ClipBank
    nfp, mask, series, times, t_in, t_out, yc, full, what = exp_clipbank.configuration(name)
    bank = ClipBank(series, times, t_in, t_out, y_channels=yc, device=nfp.device)
    loader = bank.loader(full)
    clim = torch.rand(1, 366, *bank.image_shape, generator=torch.Generator().manual_seed(3)).to(nfp.device)
    kw = {}
    if variant != 'default':
        from qtmpnn.baselines import AnomalyPersistence
        kw['references'] = {'three': ('persistence', 'climatology', 'anomaly_persistence'),
                            'four': ('anomaly_persistence', 'persistence', 'climatology',
                                     AnomalyPersistence(damping=np.linspace(1.0, 0.2, t_out)))}[variant]
    spent = {}
    for meth in ('get_climatology_array', 'get_launch_climatology'):
        if hasattr(nfp, meth):
            def timed(*a, _inner=getattr(nfp, meth), _acc=spent.setdefault(meth, [0.0, 0])):
                t0 = time.perf_counter()
                out = _inner(*a)
                _acc[0] += time.perf_counter() - t0
                _acc[1] += 1
                return out
            setattr(nfp, meth, timed)
    nfp.model.eval()
    ms, host = [], []
    for r in range(1 + repeats):
        before = {k: tuple(v) for k, v in spent.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = nfp.verify(loader, clim, mask=mask, use_graph=bool(graph), **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        host.append({k: 1e6 * (spent[k][0] - before[k][0]) / max(1, spent[k][1] - before[k][1]) for k in spent})
    rec = {'what': what, 'windows': len(bank), 'batch': full, 'batches': len(loader), 'variant': variant, 'graph': bool(graph),
           'first_ms': ms[0], 'ms': ms[1:], 'sources': list(v.sources), 'peak': torch.cuda.max_memory_allocated(),
           'host_us_first': host[0], 'host_us_later': {k: float(np.median([h[k] for h in host[1:]])) for k in spent},
           'rmse': [float(x) for x in v.score.by_lead('model')['rmse']]}
    print('RESULT ' + json.dumps(rec))


def child(root, *args):
    """Run this file with --one `args` on the tree at `root` as a process of its own under the time limit -> its RESULT record."""
    cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--one', *map(str, args)]
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get('OMP_NUM_THREADS', '16')))), EXP_BASE_ROOT=root)
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
    show = lambda rec: (f'{"graphed" if rec["graph"] else "eager  "} {rec["variant"]:<7} {len(rec["sources"])} sources: call median '
                        f'{med(rec):9.2f} ms ({min(rec["ms"]):.2f}-{max(rec["ms"]):.2f}), first call {rec["first_ms"]:9.2f} ms, '
                        f'peak {rec["peak"] / 2 ** 20:8.1f} MiB')
    emit(f'python tools/exp_baselines.py --configs {",".join(configs)} --repeats {repeats}'
         + (' --parent <checkout of the parent commit>' if parent else '') + f' --commit {commit}')
    emit(f'parent commit: {commit}; one MI355X; every line a process of its own; verify() with its six default products over a '
         f'ClipBank loader with a climatology, eval mode; times: wall time of a call, device waited for, ms, median (min-max) of '
         f'{repeats} calls after one untimed call; host times: per batch inside the named method')
    for name in configs:
        for graph in (0, 1):
            base = child(HERE, name, 'default', graph, repeats)
            if not graph:
                emit(f'{name}: {base["what"]}; {base["windows"]} windows, {base["batches"]} batches of {base["batch"]} clips')
            runs = [('this tree', base)]
            if parent:
                root = os.path.abspath(parent)
                for tree, r in (('parent', root), ('this tree', HERE), ('parent', root)):
                    runs.append((tree, child(r, name, 'default', graph, repeats)))
            for tree, rec in runs:
                emit(f'{name}: {tree + ",":<10} {show(rec)}')
            if parent:
                this = [m for tree, rec in runs if tree == 'this tree' for m in rec['ms']]
                par = [m for tree, rec in runs if tree == 'parent' for m in rec['ms']]
                same = len({tuple(rec['rmse']) for _, rec in runs}) == 1
                emit(f'{name}: (a) default call, {"graphed" if graph else "eager"}: this tree median {np.median(this):.2f} ms '
                     f'({min(this):.2f}-{max(this):.2f}) of {len(this)} calls; parent median {np.median(par):.2f} ms ({min(par):.2f}-'
                     f'{max(par):.2f}) of {len(par)}; this / parent {np.median(this) / np.median(par):.4f} x; the model rmse of the '
                     f'four runs is ' + ('equal' if same else 'NOT equal'))
            for variant in ('three', 'four'):
                rec = child(HERE, name, variant, graph, repeats)
                emit(f'{name}: this tree, {show(rec)}')
                emit(f'{name}: (b) {variant} / default, {"graphed" if graph else "eager"}: {med(rec) / med(base):.3f} x '
                     f'(+{med(rec) - med(base):.2f} ms a call, +{(med(rec) - med(base)) / rec["batches"]:.3f} ms a batch)')
                if not graph and variant == 'four':
                    f, l = rec['host_us_first'], rec['host_us_later']
                    emit(f'{name}: (c) host time a batch at {rec["batch"]} clips: get_launch_climatology {f["get_launch_climatology"]:.1f} us '
                         f'in the first call, {l["get_launch_climatology"]:.1f} us in the later ones; get_climatology_array '
                         f'{f["get_climatology_array"]:.1f} us and {l["get_climatology_array"]:.1f} us')


if __name__ == '__main__':
    if '--one' in sys.argv:
        a = sys.argv[sys.argv.index('--one') + 1:]
        root = os.environ.get('EXP_BASE_ROOT', HERE)
        for p in (os.path.join(root, 'tools'), root, os.path.join(root, 'quadtree-mpnnlstm_amd')):
            sys.path.insert(0, p)
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        one(a[0], a[1], int(a[2]), int(a[3]))
    else:
        main()
