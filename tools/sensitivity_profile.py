"""Measure what profiles/sensitivity.txt records (needs the GPU): for every case of tests/test_gpu_sensitivity.py the distance of
the maps to the float64 oracle -- of the oracle evaluated in float32, and of NextFramePredictorS2S.sensitivity on the GPU -- and
the wall time of sensitivity calls on the benchmark's model (64 x 64 frames, 10 steps in, 10 out) beside one eager train_step
on the same clip in the same process.

    python tools/sensitivity_profile.py > profiles/sensitivity.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quadtree-mpnnlstm_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


class _Patch:
    """The two methods of pytest's monkeypatch the cases use; nothing is put back (the process ends)."""

    def setitem(self, d, k, v):
        d[k] = v

    def setattr(self, o, k, v):
        setattr(o, k, v)


def distances():
    import sensitivity_cases as S
    import test_gpu_sensitivity as T
    print('distance of the maps to the float64 oracle, per case: worst |got - ref| / max|ref| over the (clip, lead) maps, and the')
    print(f'worst ratio to the bound of grad_close (rtol {S.RTOL}, floor {S.REL_ATOL} x the map\'s largest entry; <= 1 passes)')
    print(f'{"case":42s} {"float32 oracle":>26s} {"GPU":>26s}')
    row = lambda tag, a, b: print(f'{tag:42s} {a[0]:14.3e} {a[1]:11.3f} {b[0]:14.3e} {b[1]:11.3f}')
    for name in S.CASES:
        case = T.Case(name, _Patch())
        for tag, w in (('default', None),) + ((('region', S.region_target()),) if name == 'cheb_preset' else ()):
            ref = case.oracle(w)[1]
            f32 = case.oracle(w, torch.float32)[1]
            got = case.sensitivity(target=w).maps
            row(f'{name}/{tag}', S.distance(f32, ref), S.distance(got, ref))
        if name == 'cheb_preset':
            wm = S.weights_of(None, case.mask)
            base = np.full_like(case.x[0], 0.05)
            for tag, baseline, bb in (('zero baseline', None, np.zeros_like(case.x)), ('baseline 0.05', base, np.stack([base] * S.B))):
                args = (case.ref, case.x, bb, case.concat, wm, T.LEADS, 4)
                ref = S.oracle_integrated(*args, torch.float64, case.mask, None, case.gsr)
                f32 = S.oracle_integrated(*args, torch.float32, case.mask, None, case.gsr)
                s = case.sensitivity(method='integrated', steps=4, baseline=baseline)
                row(f'{name}/integrated 4, {tag}', S.distance(f32[2], ref[2]), S.distance(s.maps, ref[2]))
                print(f'    completeness residual: float64 oracle {np.abs(ref[3]).max():.3e}, float32 oracle - float64 '
                      f'{np.abs(f32[3] - ref[3]).max():.3e}, GPU - float64 {np.abs(s.completeness() - ref[3]).max():.3e}')
            grads = case.oracle()[1]
            g32 = case.oracle(None, torch.float32)[1]
            d = (case.x.astype(np.float64) - base)[:, None]
            s = case.sensitivity(method='gradient_x_input', baseline=base)
            row(f'{name}/gradient_x_input', S.distance(g32 * d, grads * d), S.distance(s.maps, grads * d))


def timings(reps=7):
    import bench
    from qtmpnn import synthetic
    dev = torch.device('cuda', 0)
    nfp = bench.make_predictor(dev)
    x, y = synthetic.make_batch(2, 0, 1, bench.T_IN, bench.T_OUT, n_digits=bench.N_DIGITS, pixel_noise=bench.NOISE, canvas=bench.CANVAS)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)
    nfp.model.eval()
    with torch.no_grad():
        fwd = median_ms(lambda: nfp.model(x, concat_layers=None, teacher_forcing_ratio=0))
    g2 = median_ms(lambda: nfp.sensitivity(x, leads=(4, 9)))
    g10 = median_ms(lambda: nfp.sensitivity(x))
    ig = median_ms(lambda: nfp.sensitivity(x, leads=(4, 9), method='integrated', steps=16))
    nfp.model.train()
    step = median_ms(lambda: nfp.train_step(x, y))
    print()
    print(f'wall time on the benchmark model ({bench.CANVAS[0]} x {bench.CANVAS[1]}, {bench.T_IN} in / {bench.T_OUT} out, hidden {bench.HIDDEN}, '
          f'{bench.N_LAYERS} layers), one clip, median of {reps} after a warm-up call, ms:')
    print(f"  eager no-grad rollout                           {fwd:8.2f}")
    print(f"  eager train_step (forward, backward, Adam)      {step:8.2f}")
    print(f"  sensitivity 'gradient', leads (4, 9)            {g2:8.2f}   = {g2 / step:.2f} train steps, {g2 / fwd:.2f} rollouts")
    print(f"  sensitivity 'gradient', all 10 leads            {g10:8.2f}   = {g10 / step:.2f} train steps")
    print(f"  sensitivity 'integrated', steps=16, leads (4, 9){ig:8.2f}   = {ig / step:.2f} train steps (16 path clips in one rollout, + one of the 2 ends)")


if __name__ == '__main__':
    print(f'{torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    distances()
    timings()
