"""Every number the four training losses produce on fixed inputs, written to one .npz: run it at two commits and compare the files
to show that a change of the loss code moves no bit (a recorded comparison: profiles/loss_refactor.txt).

    python tools/dump_loss.py --out FILE          # needs a GPU
    python tools/dump_loss.py --compare A B       # numpy.array_equal on every array; exit status 1 when any differs
Only masked_mse, masked_bce and ops.rollout_*_partials / ops.step_*_partials are called, with the arguments they have had since the
weighted binary cross-entropy was added.  For the squared error, the binary cross-entropy and their weighted forms (pos_weight 1 and
3), on a 24 x 32 mesh (smaller than a tile) and a 64 x 40 mesh (a ragged tile), 2 clips, 18 output steps (two launches), a
different mesh at every step, outputs (N_t, 4): the partial sums and every step's gradient rows through the rollout launches, and
the same through the composed per-step fall-back.  Then the values of masked_mse / masked_bce, plain, fused and weighted, on the
rollouts of tests/golden/variant_binary.npz and rollout_ice64_masked_h8.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'))
import numpy as np
import torch

T, B, G = 18, 2, 0.37
PWS = (1.0, 3.0)


def compare(a, b):
    fa, fb = np.load(a), np.load(b)
    diff = [k for k in fa.files if k not in fb.files or not np.array_equal(fa[k], fb[k], equal_nan=True)]
    diff += [k for k in fb.files if k not in fa.files]
    print(f'dump_loss: {len(fa.files)} arrays, {sum(fa[k].size for k in fa.files)} numbers, {len(diff)} differ' +
          ''.join(f'\n  {k}' for k in diff))
    return 1 if diff else 0


def main(out_path):
    from model.mpnnlstm import masked_bce, masked_mse
    from model.seq2seq import Seq2Seq
    from qtmpnn import ops
    from qtmpnn.mesh import build_mesh
    dev = torch.device('cuda', 0)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    np_ = lambda t: t.detach().cpu().numpy()
    res = {}
    for tag, (n, m) in (('S', (24, 32)), ('C', (64, 40))):
        rng = np.random.default_rng(ord(tag))
        crit = np.zeros((B, n, m), np.float32)
        crit[0, n // 3:n // 3 + 5, m // 2:m // 2 + 7] = 1.0
        crit[1] = rng.random((n, m)) < 0.03
        meshes = []
        for t in range(T):
            c = crit.copy()
            for b in range(B):
                r, q = rng.integers(0, n - 4), rng.integers(0, m - 4)
                c[b, r:r + 1 + t % 4, q:q + 2] = 1.0
            meshes.append(build_mesh(src=t_(c), thresh=0.5))
        os_ = []
        for ms in meshes:
            o = (rng.standard_normal((ms.N, 4)) * 3.0).astype(np.float32)
            o[:, 0] = rng.uniform(0.02, 0.98, ms.N)
            os_.append(o)
        kind = rng.integers(0, 3, (B, T, n, m, 1))
        y = t_(np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.random(kind.shape))))
        y2 = t_(rng.random((B, 2 * T, n, m, 1)))[:, ::2]         # not contiguous: what sends masked_* step by step
        w = rng.uniform(0.25, 4.0, (n, m)).astype(np.float32)
        w[rng.random((n, m)) < 0.125] = 0.0
        lam = (0.5 + rng.random(T)).astype(np.float32)
        lam[T - 2] = 0.0
        wd, ld = t_(w).view(-1), t_(lam)
        losses = {'sse': (ops.rollout_sse_partials, ops.step_sse_partials, ()),
                  'bce': (ops.rollout_bce_partials, ops.step_bce_partials, ()),
                  'wsse': (ops.rollout_wsse_partials, ops.step_wsse_partials, ())}
        for pw in PWS:
            losses[f'wbce_pw{pw:g}'] = (ops.rollout_wbce_partials, ops.step_wbce_partials, (pw,))
        for name, (rollout, step, tail) in losses.items():
            bases = [t_(o).requires_grad_(True) for o in os_]
            outs = [b[:, :1] for b in bases]
            part = rollout(outs, y, meshes, *((wd, ld) if name[0] == 'w' else ()), *tail)
            assert part is not None, name
            res[f'{tag}/{name}/part'] = np_(part)
            for t, g in enumerate(torch.autograd.grad(part.sum() * G, bases)):
                res[f'{tag}/{name}/grad{t}'] = np_(g)
            assert rollout(outs, y2, meshes, *((wd, ld) if name[0] == 'w' else ()), *tail) is None, name
            bases = [t_(o).requires_grad_(True) for o in os_]
            parts = [step(b[:, :1], y2[:, t], ms, *((wd, ld[t]) if name[0] == 'w' else ()), *tail)
                     for t, (b, ms) in enumerate(zip(bases, meshes))]
            res[f'{tag}/{name}/step_part'] = np.concatenate([np_(p) for p in parts])
            for t, g in enumerate(torch.autograd.grad(torch.cat(parts).sum() * G, bases)):
                res[f'{tag}/{name}/step_grad{t}'] = np_(g)
        # the same through the trainer's functions: all steps in one launch, and step by step
        mask = np.zeros((n, m), bool)
        mask[n // 2:n // 2 + 3, 1:m - 2] = True
        outs = [t_(o)[:, :1] for o in os_]
        for form, yy in (('rollout', y), ('per_step', y2)):
            calls = {'mse': lambda: masked_mse(outs, meshes, yy, mask),
                     'mse_weighted': lambda: masked_mse(outs, meshes, yy, mask, weights=w, lead_weights=lam),
                     'bce_fused': lambda: masked_mse(outs, meshes, yy, mask, binary=True, fused=True),
                     'bce_weighted_pw1': lambda: masked_bce(outs, meshes, yy, mask, weights=w, lead_weights=lam),
                     'bce_weighted_pw3': lambda: masked_bce(outs, meshes, yy, mask, weights=w, lead_weights=lam, pos_weight=3.0)}
            for name, call in calls.items():
                res[f'{tag}/masked/{form}/{name}'] = np_(call())

    golden = lambda name: np.load(os.path.join(ROOT, 'tests', 'golden', name), allow_pickle=False)
    for name, binary in (('variant_binary.npz', True), ('rollout_ice64_masked_h8.npz', False)):
        g = golden(name)
        x, y, concat = (torch.from_numpy(g[k]).to(dev) for k in ('x', 'y', 'concat'))
        if binary:
            model = Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.1, input_timesteps=3, input_features=4, output_timesteps=4,
                            n_layers=1, n_conv_layers=2, convolution_type='ChebConv', binary=True)
        else:
            model = Seq2Seq(hidden_size=int(g['hidden']), dropout=0.0, thresh=float(g['thresh']), input_timesteps=x.shape[0],
                            input_features=x.shape[-1] + 3, output_timesteps=y.shape[0], n_layers=int(g['n_layers']),
                            n_conv_layers=int(g['n_conv']),
                            transform_func=(lambda a: abs(abs(a - 0.5) - 0.5)) if bool(g['has_transform']) else None)
        model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}, strict=True)
        model = model.to(dev)
        n, m, T_out = y.shape[-3], y.shape[-2], y.shape[-4]
        w = np.linspace(0.5, 2.0, n * m, dtype=np.float32).reshape(n, m)
        lam = np.linspace(0.5, 1.5, T_out).astype(np.float32)
        calls = {'mse': dict(), 'mse_weighted': dict(weights=w, lead_weights=lam)}
        if binary:
            calls.update({'bce_torch': dict(binary=True), 'bce_fused': dict(binary=True, fused=True),
                          'bce_weighted_pw1': dict(weights=w, lead_weights=lam), 'bce_weighted_pw3': dict(weights=w, lead_weights=lam,
                                                                                                       pos_weight=3.0)})
        for key, kw in calls.items():
            model.zero_grad(set_to_none=True)
            outs, meshes = model(x, y, concat, teacher_forcing_ratio=0, mask=g['mask'])
            loss = (masked_bce if key.startswith('bce_weighted') else masked_mse)(outs, meshes, y, g['mask'], **kw)
            loss.backward()
            res[f'{name}/{key}/loss'] = np_(loss)
            for k, p in model.named_parameters():
                if p.grad is not None:
                    res[f'{name}/{key}/g/{k}'] = np_(p.grad)
    np.savez(out_path, **res)
    print(f'dump_loss: {len(res)} arrays, {sum(v.size for v in res.values())} numbers -> {out_path}')
    return 0


if __name__ == '__main__':
    if '--compare' in sys.argv:
        i = sys.argv.index('--compare')
        sys.exit(compare(sys.argv[i + 1], sys.argv[i + 2]))
    sys.exit(main(sys.argv[sys.argv.index('--out') + 1]))
