"""Parity of the BENCHMARKED workload (BASELINE.json configs[1]: 64x64, 2 digits, noise 0.05, in=10/out=10, 32 clips,
hidden 16, 2 layers, static capacities + hipGraph replay) against a trace captured from the reference
(tests/golden/rollout_cfg2_mnist64.npz = clip 0 of bench.py's first batch), and one training step at every BASELINE
configuration's full image size."""
import numpy as np
import pytest
import torch

from helpers import close, dev, golden, grad_close, load_state

pytestmark = pytest.mark.gpu

T_IN = T_OUT = 10
B = 32


def _bench_batch():
    from qtmpnn import synthetic
    return synthetic.make_batch(2, 0, B, T_IN, T_OUT, n_digits=2, pixel_noise=0.05, canvas=(64, 64))


def _predictor(g, dropout=0.0):
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                model_kwargs=dict(hidden_size=16, dropout=dropout, n_layers=2))
    load_state(nfp.model, g, 'w/')
    nfp.model.train()
    return nfp


def _capture(nfp, sx, sy, sc, mask):
    """forward + loss + backward of the static-capacity step captured in ONE hipGraph (what bench.py replays, minus clip +
    Adam, so that the gradients stay readable); returns (graph, outs, meshes, loss) -- static buffers the replay refills."""
    from model.mpnnlstm import masked_mse
    nfp.model.static_shapes = True
    params = list(nfp.model.parameters())
    keep = {}

    def fwd_bwd():
        for p in params:
            p.grad = None
        outs, meshes = nfp.model(sx, sy, sc, teacher_forcing_ratio=0, mask=mask)
        loss = masked_mse(outs, meshes, sy, mask)
        loss.backward()
        keep.update(outs=outs, meshes=meshes, loss=loss.detach())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for p in params:
        p.grad = None
    with torch.cuda.graph(graph, stream=side):
        fwd_bwd()
    return graph, keep


def _clip_losses(outs, meshes, y, shape):
    """Per-clip MSE (model/mpnnlstm.py:243-246) from the device outputs, with plain torch indexing (no product kernel)."""
    Bc = meshes[0].B
    sse = torch.zeros(Bc, dtype=torch.float64, device=y.device)
    for t, (o, ms) in enumerate(zip(outs, meshes)):
        img = o[:, 0][ms.labels.view(Bc, -1).long()]                      # unflatten: pixel <- its node
        sse += ((img - y[:, t].reshape(Bc, -1)).double() ** 2).sum(1)
    return sse / (len(outs) * shape[0] * shape[1])


def test_headline_batch32_graph_replay_matches_reference_trace():
    """Clip 0 of the benchmarked 32-clip batch is the golden clip: after a hipGraph replay of the B=32 static step, its
    meshes are bit-identical to the reference's at every decoder step (a first difference must be explained by a pixel
    on the threshold), its outputs match at rtol 1e-4 and its share of the loss equals the reference's loss."""
    g = golden('rollout_cfg2_mnist64.npz')
    x, y = _bench_batch()
    assert np.array_equal(x[0], g['x']) and np.array_equal(y[0], g['y']), 'bench clip 0 is no longer the golden clip'
    mask = np.zeros((64, 64), dtype=bool)
    xt, yt = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    ct = torch.zeros(B, T_OUT, 64, 64, 1, device=dev())
    nfp = _predictor(g)
    sx, sy = torch.zeros_like(xt), torch.zeros_like(yt)
    # captured on another batch (the golden clip repeated with a roll), replayed on the bench batch: the replay must
    # follow the data, meshes included
    sx.copy_(xt.roll(1, 0))
    sy.copy_(yt.roll(1, 0))
    graph, k = _capture(nfp, sx, sy, ct, mask)
    sx.copy_(xt)
    sy.copy_(yt)
    graph.replay()
    torch.cuda.synchronize()
    outs, meshes, loss = k['outs'], k['meshes'], k['loss']
    thresh, flipped = float(g['thresh']), None
    for i, ms in enumerate(meshes):
        off = ms.node_off.cpu().numpy()
        assert ms.N == B * 64 * 64 and ms.n_dev is not None and int(ms.n_dev.item()) == off[B]
        lab = ms.labels[0].cpu().numpy()
        if not np.array_equal(lab, g[f'labels_{i}']):
            near = np.abs(g[f'image_{i}'] - thresh).min()
            assert near < 1e-5, f'mesh {i} of clip 0 differs and no pixel sits on the threshold ({near})'
            flipped = i
            break
        assert off[1] - off[0] == len(g[f'out_{i}'])
        close(outs[i][off[0]:off[1], :1], g[f'out_{i}'], msg=f'clip 0 output step {i}')
    per_clip = _clip_losses(outs, meshes, yt, (64, 64))
    assert abs(float(per_clip.mean()) - float(loss)) <= 1e-5 * float(loss), (float(per_clip.mean()), float(loss))
    # the fixture's seeds keep every pixel of every step away from the threshold (margin checked when it was generated): a
    # flipped mesh is a regression, not chaos -- fail (everything before the flipped step was asserted above)
    assert flipped is None, f'mesh {flipped} of clip 0 differs from the reference trace (earlier steps matched)'
    assert abs(float(per_clip[0]) - float(g['loss'])) <= 1e-4 * float(g['loss']), (float(per_clip[0]), float(g['loss']))
    # every clip's meshes obey the size-independent invariants
    for ms in meshes:
        nv = int(ms.n_dev.item())
        assert float(ms.npix[:nv].sum()) == B * 64 * 64
        assert int(ms.labels.max()) == nv - 1 and int(ms.labels.min()) >= 0


def test_headline_batch32_gradients_match_reference():
    """32 copies of the golden clip through the same captured B=32 step: loss and all 238 parameter gradients (mean over
    clips = the single clip's) against the reference's backward pass."""
    g = golden('rollout_cfg2_mnist64.npz')
    mask = np.zeros((64, 64), dtype=bool)
    rep = lambda a: torch.from_numpy(a).to(dev()).unsqueeze(0).repeat(B, 1, 1, 1, 1).contiguous()
    xt, yt = rep(g['x']), rep(g['y'])
    ct = torch.zeros(B, T_OUT, 64, 64, 1, device=dev())
    nfp = _predictor(g)
    sx, sy = xt.clone(), yt.clone()
    graph, k = _capture(nfp, sx, sy, ct, mask)
    graph.replay()
    torch.cuda.synchronize()
    for i, ms in enumerate(k['meshes']):
        for c in (0, B - 1):
            off = ms.node_off.cpu().numpy()
            lab = ms.labels[c].cpu().numpy() - off[c]
            if not np.array_equal(lab, g[f'labels_{i}']):
                near = np.abs(g[f'image_{i}'] - float(g['thresh'])).min()
                pytest.fail(f'mesh {i} of clip {c} differs from the reference trace (nearest pixel to the threshold: {near})')
    assert abs(float(k['loss']) - float(g['loss'])) <= 1e-4 * float(g['loss'])
    for name, p in nfp.model.named_parameters():
        ref = g['g/' + name]
        if p.grad is None:
            assert not ref.any(), name
            continue
        grad_close(p.grad, ref, msg=name)


def test_headline_split_bf16_dgrad_is_optin_and_its_error_is_known():
    """The default backward is exact fp32 (ops.DGRAD_SPLIT_BF16 False: the gradient test above ran it).  The opt-in split-bf16
    data gradient of the gate GEMM (bench.py reports it beside the headline as `split_bf16_dgrad`) stays alive here: the same
    captured B=32 step in both modes, worst per-tensor error of split vs exact relative to the tensor's largest entry, and the
    split gradients still inside the reference tolerance."""
    from qtmpnn import ops
    g = golden('rollout_cfg2_mnist64.npz')
    mask = np.zeros((64, 64), dtype=bool)
    rep = lambda a: torch.from_numpy(a).to(dev()).unsqueeze(0).repeat(B, 1, 1, 1, 1).contiguous()
    xt, yt = rep(g['x']), rep(g['y'])
    ct = torch.zeros(B, T_OUT, 64, 64, 1, device=dev())
    assert ops.DGRAD_SPLIT_BF16 is False, 'the exact fp32 data gradient must be the default'
    grads = {}
    for mode in (False, True):
        prev = ops.set_dgrad_split_bf16(mode)
        try:
            nfp = _predictor(g)
            graph, k = _capture(nfp, xt.clone(), yt.clone(), ct, mask)
            graph.replay()
            torch.cuda.synchronize()
            grads[mode] = {n: p.grad.detach().clone() for n, p in nfp.model.named_parameters() if p.grad is not None}
            assert abs(float(k['loss']) - float(g['loss'])) <= 1e-4 * float(g['loss'])
        finally:
            ops.set_dgrad_split_bf16(prev)
    worst, worst_name, differs = 0.0, None, False
    for n, ge in grads[False].items():
        gs = grads[True][n]
        differs |= not torch.equal(ge, gs)
        scale = float(ge.abs().max())
        if scale > 0:
            e = float((gs - ge).abs().max()) / scale
            if e > worst:
                worst, worst_name = e, n
        grad_close(gs, g['g/' + n], msg=n + ' (split-bf16 data gradient)')
    assert differs, 'the split-bf16 switch changed nothing: the opt-in path did not run'
    print(f'split-bf16 vs exact data gradient: worst per-tensor max-error / max-entry = {worst:.3e} ({worst_name})')
    assert worst < 2e-4, (worst, worst_name)


@pytest.mark.parametrize('cfg', ['cfg1_mnist64_b4', 'cfg2_mnist64_b32'])
def test_baseline_mnist64_configs_train(cfg):
    """BASELINE.json configs[0] (1 digit, 4 clips) and configs[1] (2 digits, 32 clips) at full size: a hipGraph-replayed
    training step (what bench.py times) gives the eager step's loss from the same state, the loss falls over a few steps,
    and the meshes satisfy the size-independent invariants."""
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import synthetic
    nb, digits = (4, 1) if cfg == 'cfg1_mnist64_b4' else (32, 2)
    x, y = synthetic.make_batch(1 if digits == 1 else 2, 0, nb, T_IN, T_OUT, n_digits=digits, pixel_noise=0.05, canvas=(64, 64))
    xt, yt = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    ct = torch.zeros(nb, T_OUT, 64, 64, 1, device=dev())
    mask = np.zeros((64, 64), dtype=bool)

    def fresh():
        torch.manual_seed(1)
        nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                    model_kwargs=dict(hidden_size=16, dropout=0.0, n_layers=2))
        nfp.initiate_training(lr=0.01, lr_decay=0.95, capturable=True)
        nfp.model.static_shapes = True
        nfp.model.train()
        return nfp
    eager, graphed = fresh(), fresh()
    assert eager.get_n_params() == 34513
    le = [float(eager.train_step(xt, yt, ct, mask)) for _ in range(5)]
    # the flat path is live: one optimizer tensor, and every parameter's gradient is a view of the backward's one vector
    assert eager.flat is not None and len(eager.optimizer.param_groups[0]['params']) == 1
    assert eager.flat.grad_vector() is not None and eager.flat.param.grad.data_ptr() == eager.flat.grad_vector().data_ptr()
    step = graphed.make_graphed_step(xt, yt, ct, mask=mask, warmup=2)
    lg = [float(step(xt, yt, ct)) for _ in range(3)]
    assert np.isfinite(le).all() and le[-1] < le[0], le
    for a, b in zip(le[2:], lg):
        assert abs(a - b) <= 1e-4 * abs(a), (le, lg)
    outs, meshes = eager.model(xt, yt, ct, teacher_forcing_ratio=0, mask=mask)
    for ms in meshes:
        nv = ms.n_valid
        assert float(ms.npix[:nv].sum()) == nb * 64 * 64
        assert int(ms.labels.max()) == nv - 1 and int(ms.labels.min()) >= 0


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """bench.py without --full: exactly --steps timed steps behind `ms_per_step` / `value`, none of the --full records, and
    --dump-outputs holds the last timed step's loss (the line's final_loss), its updated parameters and its clipped gradient.
    --full computes the same timed steps (its frozen phase is the plain run's untimed one): the same outputs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(out, *extra):
        cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4',
               '--dump-outputs', str(out), *extra]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, res.stdout[-2000:]
        return json.loads(lines[0]), [np.load(out / f) for f in ('loss.npy', 'params.npy', 'grad.npy')]

    rec, (loss, params, grad) = run(tmp_path / 'plain')
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['unit'] == 'frames/s' and rec['dtype'] == 'f32'
    assert rec['higher_is_better'] is True and rec['ms_per_step'] > 0
    assert abs(rec['value'] - 4 * (T_IN + T_OUT) * 1e3 / rec['ms_per_step']) <= 1e-3 * rec['value']
    assert rec['window_ms_per_step'] == [rec['ms_per_step']] and rec['frozen_ms_per_step'] is None
    assert not {'roofline', 'mfma', 'rollout_sizes', 'split_bf16_dgrad', 'step', 'cpu_baseline'} & set(rec)
    assert sorted(os.listdir(tmp_path / 'plain')) == ['grad.npy', 'loss.npy', 'params.npy']
    assert loss.dtype == params.dtype == grad.dtype == np.float32
    assert loss.shape == () and params.shape == grad.shape == (34513,)
    assert np.isfinite(params).all() and np.isfinite(grad).all()
    assert abs(float(loss) - rec['config']['final_loss']) <= 1e-6 * max(1.0, abs(float(loss)))
    assert 0 < np.linalg.norm(grad.astype(np.float64)) <= 10.0 * (1 + 1e-4)          # clip_grad_norm_(10) before Adam

    full, outs = run(tmp_path / 'full', '--full', '--repeats', '0', '--no-roofline', '--no-split-variant', '--no-cpu-baseline')
    assert full['frozen_ms_per_step'] > 0
    for a, b in zip(outs, (loss, params, grad)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7)
