"""Break-up / freeze-up dates on the GPU (qt_event_scan, qt_event_sums, ops.rollout_event_dates,
NextFramePredictorS2S.event_dates) against the numpy restatement of tests/events_restated.py.

Everything is an integer (dates, counts, sums of date differences) and both sides decide a state by the same strict fp32
comparison of the same fp32 values, so every comparison is equality.

The op-level fields are designed, not model output: an ice edge with a wavy front that moves across a 64 x 64 frame, faster or
slower in the model than in the observed frames, with pixel noise that breaks runs.  Before anything is compared the tests assert
on the restatement's output that every class of the contingency table, runs that begin in one 16-step launch and complete in the
next, and pixels already in the target state at launch are all well populated."""
import copy
import functools

import numpy as np
import pytest
import torch

from events_restated import restated_events
from helpers import dev, golden

pytestmark = pytest.mark.gpu

THR = 0.15
KINDS = ('breakup', 'freezeup')


def edge_field(speed, phase, seed, T, shape=(64, 64)):
    """(T + 1, W, H) fp32, steps t = -1 (the launch frame) .. T - 1: clip(0.15 + (j - edge) / 10 + 0.12 * N(0, 1), 0, 1) with
    edge = 8 + phase + speed * (t + 1) + 6 * sin(i / 9): ice to the right of a front that moves right by `speed` per step."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(shape[0], dtype=np.float32), np.arange(shape[1], dtype=np.float32), indexing='ij')
    frames = []
    for t in range(-1, T):
        edge = np.float32(8 + phase) + np.float32(speed) * np.float32(t + 1) + np.float32(6) * np.sin(i / np.float32(9))
        f = np.float32(0.15) + (j - edge) / np.float32(10) + np.float32(0.12) * rng.standard_normal(shape, dtype=np.float32)
        frames.append(np.clip(f, 0, 1).astype(np.float32))
    return np.stack(frames)


@functools.lru_cache(maxsize=None)
def designed(kind, T=18):
    """{'launch' (2, W, H), 'observed' / 'model' / 'climatology' (2, T, W, H)} fp32 for two clips.  Observed: speed 2.0, phase 0
    (seeds 5, 6); model: speed 2.6, phase -3, seed 7 (clip 0) and speed 1.4, phase +3, seed 8 (clip 1), its launch frame the
    observed one; climatology: speed 2.0, seed 9 (clip 0) and 10 (clip 1).  Freeze-up uses 1 - f."""
    obs = np.stack([edge_field(2.0, 0, 5, T), edge_field(2.0, 0, 6, T)])
    model = np.stack([edge_field(2.6, -3, 7, T), edge_field(1.4, 3, 8, T)])
    clim = np.stack([edge_field(2.0, 0, 9, T), edge_field(2.0, 0, 10, T)])
    if kind == 'freezeup':
        obs, model, clim = (np.float32(1) - a for a in (obs, model, clim))
    out = {'launch': obs[:, 0], 'observed': obs[:, 1:], 'model': model[:, 1:], 'climatology': clim[:, 1:]}
    for a in out.values():
        a.setflags(write=False)
    return out


def _populated(dates, sums, launch, kind, k, mask=None):
    """The condition under which a comparison says something (model source, both clips): every class >= 100, >= 50 dates of runs
    that begin in the first 16-step launch and complete in the second (k >= 2: a run of one step cannot straddle), >= 50
    counted pixels in the target state at launch."""
    tot = sums[:, 0].sum(axis=0)
    print(f'{kind} k={k}: hits {tot[4]} false alarms {tot[5]} misses {tot[6]} neither {tot[7]}')
    assert (tot[4:8] >= 100).all(), tot
    if k >= 2:
        straddle = int(((dates[:, :2] >= 16 - k + 1) & (dates[:, :2] <= 15)).sum())
        print(f'  dates in {16 - k + 1}..15: {straddle}')
        assert straddle >= 50, straddle
    keep = np.ones(launch.shape[1:], bool) if mask is None else ~mask
    at_target = int((((launch > np.float32(THR)) == (kind == 'freezeup')) & keep).sum())
    assert at_target >= 50, at_target


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _pixel_mesh(B, shape, mask=None):
    from qtmpnn.mesh import build_pixel_mesh
    return build_pixel_mesh(B, shape[0], shape[1], mask, dev())


def _frames(outs, meshes, shape, mask=None):
    """What the restatement sees of the model: unflatten of every step's node values, (B, T, W, H) on the host."""
    from model.graph_functions import unflatten
    fr = [unflatten(o[:, :1], ms, shape, mask).cpu().numpy() for o, ms in zip(outs, meshes)]
    fr = [f[None] if ms.B == 1 else f for f, ms in zip(fr, meshes)]
    return np.stack([f[..., 0] for f in fr], axis=1)


def _fields(d, frames, with_clim):
    """Per clip {source: (T, W, H)} for the restatement."""
    out = []
    for b in range(len(frames)):
        f = {'observed': d['observed'][b], 'model': frames[b]}
        if with_clim:
            f['climatology'] = d['climatology'][b]
        out.append(f)
    return out


def _compare(got, want, shape):
    dates, sums = got
    B, S1 = want[0].shape[:2]
    assert dates.dtype == torch.int32 and sums.dtype == torch.int64 and dates.is_cuda and sums.is_cuda
    assert tuple(dates.shape) == (B, S1, shape[0] * shape[1]) and tuple(sums.shape) == (B, S1 - 1, 8)
    np.testing.assert_array_equal(dates.cpu().numpy().reshape(B, S1, *shape), want[0])
    np.testing.assert_array_equal(sums.cpu().numpy(), want[1])


@pytest.mark.parametrize('with_clim', [False, True])
@pytest.mark.parametrize('k', [1, 3, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_pixelwise_rollout_equals_restatement(kind, k, with_clim):
    """B = 2, T = 18 (two launches: 16 + 2 steps), every pixel a node; outputs[z] = flatten(field_z, mesh)."""
    from model.graph_functions import flatten
    from qtmpnn import ops
    d = designed(kind)
    B, T, shape = 2, 18, (64, 64)
    mesh = _pixel_mesh(B, shape)
    outs = [flatten(_t(d['model'][:, z])[:, None, :, :, None], mesh, None)[0] for z in range(T)]
    assert outs[0].shape == (B * 64 * 64, 1)
    frames = _frames(outs, [mesh] * T, shape)
    np.testing.assert_array_equal(frames, d['model'])
    want = restated_events(_fields(d, frames, with_clim), list(d['launch']), None, THR, kind, k)
    _populated(*want, d['launch'], kind, k)
    args = (outs, [mesh] * T, _t(d['observed']), _t(d['launch']), THR, kind, k, _t(d['climatology']) if with_clim else None)
    got = ops.rollout_event_dates(*args)
    _compare(got, want, shape)
    again = ops.rollout_event_dates(*args)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    assert not got[0].requires_grad and not got[1].requires_grad


@functools.lru_cache(maxsize=None)
def _quadtree_rollout(kind):
    """A mesh per step from image_to_graph of that step's model field (thresh 0.1, masked), outputs = the node means, and the
    frames the restatement sees."""
    from model.graph_functions import flatten, image_to_graph
    from test_gpu_predict_graph import _mask
    d = designed(kind)
    mask = _mask((64, 64), 4)
    meshes, outs = [], []
    for z in range(18):
        img = _t(d['model'][:, z])[:, None, :, :, None]
        mesh = image_to_graph(img, thresh=0.1, mask=mask)['mapping']
        meshes.append(mesh)
        outs.append(flatten(img, mesh, None)[0].contiguous())
    return mask, meshes, outs, _frames(outs, meshes, (64, 64), mask)


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_remeshing_quadtree_rollout_equals_restatement(kind, k):
    """A different mesh at every step, a mask, node means as outputs, climatology: the state is carried per pixel across meshes
    and across the two launches."""
    from qtmpnn import ops
    d = designed(kind)
    mask, meshes, outs, frames = _quadtree_rollout(kind)
    Ns = [ms.N for ms in meshes]
    assert len(set(Ns)) > 4 and max(Ns) < 2 * int((~mask).sum()), Ns           # re-meshing, with cells larger than a pixel
    lab = np.stack([ms.labels.cpu().numpy().reshape(2, 64, 64) for ms in meshes])
    assert ((lab < 0) == mask).all()
    want = restated_events(_fields(d, frames, True), list(d['launch']), mask, THR, kind, k)
    _populated(*want, d['launch'], kind, k, mask)
    assert (want[0][..., mask] == -2).all() and (want[0][..., ~mask] > -2).all()
    args = (outs, meshes, _t(d['observed']), _t(d['launch']), THR, kind, k, _t(d['climatology']))
    got = ops.rollout_event_dates(*args)
    _compare(got, want, (64, 64))
    again = ops.rollout_event_dates(*args)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_frame_that_is_no_multiple_of_the_block():
    """100 x 100 (the blob fixture's shape): P = 10000 = 39 * 256 + 16, the last workgroup is partly empty.  T = 3, k = 2, B = 2;
    fields: uniform noise around the threshold 0.5 plus the fixture's two frames."""
    from qtmpnn import ops
    g = golden('graph_100_2blob_clean.npz')
    shape = tuple(g['x'].shape[1:3])
    assert shape == (100, 100) and (shape[0] * shape[1]) % 256 == 16
    B, T = 2, 3
    rng = np.random.default_rng(11)
    blob = g['x'][..., 0].astype(np.float32)                                # (2, 100, 100)
    mk = lambda: (0.8 * rng.random((B, T, *shape), dtype=np.float32) + 0.3 * blob[:, None]).astype(np.float32)
    obs, model, launch = mk(), mk(), mk()[:, 0]
    mesh = _pixel_mesh(B, shape)
    outs = [_t(model[:, z].reshape(-1, 1)) for z in range(T)]
    fields = [{'observed': obs[b], 'model': model[b]} for b in range(B)]
    for kind in KINDS:
        want = restated_events(fields, list(launch), None, 0.5, kind, 2)
        tot = want[1][:, 0].sum(axis=0)
        assert (tot[4:8] >= 100).all() and (want[0][:, :, -1, -16:] >= 0).any(), tot
        got = ops.rollout_event_dates(outs, [mesh] * T, _t(obs), _t(launch), 0.5, kind, 2)
        _compare(got, want, shape)


def test_stale_node_count_uncounts_the_rows_beyond_it():
    """n_devs given and smaller than Ns at one step (13 of 18): the pixels whose label lies beyond it -- the last two rows of
    clip 1 -- become -2 for every source although most had their event before that step; the rest is unchanged."""
    from qtmpnn import ops
    kind, k, T, shape = 'breakup', 3, 18, (64, 64)
    d = designed(kind)
    mesh = _pixel_mesh(2, shape)
    stale = copy.copy(mesh)
    n_dev = mesh.N - 2 * 64
    stale.n_dev = torch.tensor([n_dev], dtype=torch.int32, device=dev())
    meshes = [mesh] * 13 + [stale] + [mesh] * 4
    outs = [_t(d['model'][:, z].reshape(-1, 1)) for z in range(T)]
    frames = np.array(d['model'])
    frames[1, 13, 62:] = np.nan
    want = restated_events(_fields(d, frames, True), list(d['launch']), None, THR, kind, k)
    full = restated_events(_fields(d, np.array(d['model']), True), list(d['launch']), None, THR, kind, k)
    assert (want[0][1, :, 62:] == -2).all() and (full[0][1, :, 62:] >= 0).sum() >= 50
    assert ((full[0][1, :, 62:] >= 0) & (full[0][1, :, 62:] < 13 - k)).sum() >= 50      # found before the stale step
    assert np.array_equal(want[0][0], full[0][0]) and np.array_equal(want[0][1, :, :62], full[0][1, :, :62])
    assert want[1][1, 0, 0] == 64 * 64 - 128 and want[1][0, 0, 0] == 64 * 64
    got = ops.rollout_event_dates(outs, meshes, _t(d['observed']), _t(d['launch']), THR, kind, k, _t(d['climatology']))
    _compare(got, want, shape)
    assert (got[0].view(2, 3, 64, 64)[1, :, 62:] == -2).all()


def test_run_across_the_launch_boundary():
    """T = 17, k = 2, break-up: column 20 of the model is ice up to step 14 and open at steps 15 and 16 -- the run begins as the
    last step of the first launch and completes as the first step of the second.  Its date is 15; it would be -1 if the run
    lengths did not survive between the launches.  Column 30 opens at step 16 only (cut off by the end: -1), column 40 at steps
    14, 15 (inside the first launch: 14); the observed frames open column 20 one step earlier."""
    from qtmpnn import ops
    B, T, shape = 1, 17, (64, 64)
    model = np.full((B, T, *shape), 0.9, np.float32)
    model[:, 15:, :, 20] = 0.05
    model[:, 16:, :, 30] = 0.05
    model[:, 14:16, :, 40] = 0.05
    obs = np.full((B, T, *shape), 0.9, np.float32)
    obs[:, 14:, :, 20] = 0.05
    launch = np.full((B, *shape), 0.9, np.float32)
    mesh = _pixel_mesh(B, shape)
    outs = [_t(model[:, z].reshape(-1, 1)) for z in range(T)]
    dates, sums = ops.rollout_event_dates(outs, [mesh] * T, _t(obs), _t(launch), THR, 'breakup', 2)
    dates = dates.cpu().numpy().reshape(2, 64, 64)
    expect = np.full((64, 64), -1, np.int32)
    expect[:, 20], expect[:, 40] = 15, 14
    np.testing.assert_array_equal(dates[1], expect)
    assert (dates[0][:, 20] == 14).all() and (np.delete(dates[0], 20, axis=1) == -1).all()
    assert sums.cpu().numpy().tolist() == [[[4096, 64, 64, 64, 64, 64, 0, 4096 - 128]]]
    want = restated_events([{'observed': obs[0], 'model': model[0]}], [launch[0]], None, THR, 'breakup', 2)
    np.testing.assert_array_equal(dates, want[0][0])


def _restated_for(nfp, loader, clim, extra, thr, kind, k, frames):
    from test_gpu_score import _clips
    fields, launches = [], []
    for c, (x, y, launch) in enumerate(_clips(loader)):
        f = {'observed': y.astype(np.float32), 'model': frames[c, ..., 0]}
        if clim is not None:
            f['climatology'] = nfp.get_climatology_array(clim, launch).cpu().numpy()[..., 0]
        fields.append(f)
        launches.append(np.ascontiguousarray(x[-1, ..., 0], dtype=np.float32))
    return restated_events(fields, launches, extra.get('mask'), thr, kind, k)


@pytest.mark.parametrize('name', ['cheb_quadtree', 'transformer_pixelwise'])
def test_event_dates_of_a_predictor(name):
    """cheb_quadtree: re-meshing rollout, batches of 2, 2 and 1 clips; transformer_pixelwise: mask + climatology, single clips.
    Freeze-up, persist 2, at the median of the predicted frames."""
    from test_gpu_predict_graph import _config
    nfp, loader, clim, extra = _config(name)
    nfp.model.eval()
    frames = nfp.predict(loader, clim, **extra)
    score0 = nfp.score(loader, clim, **extra)
    thr = float(np.nanmedian(frames))
    kind, k = 'freezeup', 2
    want = _restated_for(nfp, loader, clim, extra, thr, kind, k, frames)
    tot = want[1][:, 0].sum(axis=0)
    print(f'{name}: threshold {thr:.6f}, model sums {tot.tolist()}')
    assert (want[0][:, 1] >= 0).any() and (want[0][:, 1] == -1).any()                    # the model crosses the threshold
    ev = nfp.event_dates(loader, clim, threshold=thr, kind=kind, persist=k, **extra)
    assert nfp.model.static_shapes is False
    S1 = 3 if clim is not None else 2
    assert ev.sources == ('observed', 'model', 'climatology')[:S1] and (ev.kind, ev.persist, ev.threshold) == (kind, k, thr)
    assert ev.dates.shape == want[0].shape == (len(frames), S1, *loader.dataset.image_shape) and ev.dates.dtype == np.int32
    assert ev.sums.shape == want[1].shape and ev.sums.dtype == np.int64
    np.testing.assert_array_equal(ev.dates, want[0])
    np.testing.assert_array_equal(ev.sums, want[1])
    if 'mask' in extra:
        assert (ev.dates[..., extra['mask']] == -2).all() and (ev.dates[..., ~extra['mask']] > -2).all()
    # graphed == eager in static mode, bit for bit, twice
    nfp.model.static_shapes = True
    static = nfp.event_dates(loader, clim, threshold=thr, kind=kind, persist=k, **extra)
    assert nfp.model.static_shapes is True
    nfp.model.static_shapes = False
    for _ in range(2):
        graphed = nfp.event_dates(loader, clim, use_graph=True, threshold=thr, kind=kind, persist=k, **extra)
        assert nfp.model.static_shapes is False
        assert graphed.sources == static.sources
        np.testing.assert_array_equal(graphed.dates, static.dates)
        np.testing.assert_array_equal(graphed.sums, static.sums)
    # predict() and score() of the same model are what they were
    assert np.array_equal(nfp.predict(loader, clim, **extra), frames, equal_nan=True)
    assert np.array_equal(nfp.score(loader, clim, **extra).sums, score0.sums)
    with pytest.raises(ValueError, match='event_dates: kind must be'):
        nfp.event_dates(loader, clim, kind='melt', **extra)
    for bad in (0, nfp.output_timesteps + 1):
        with pytest.raises(ValueError, match='event_dates: persist must be'):
            nfp.event_dates(loader, clim, persist=bad, **extra)


def test_rollout_event_dates_refuses_by_name():
    from qtmpnn import ops
    from test_gpu_predict_graph import _config
    nfp, loader, clim, extra = _config('cheb_quadtree')
    nfp.model.eval()
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    with torch.no_grad():
        y_hat, meshes = nfp.model(x, teacher_forcing_ratio=0)
    T, launch = len(y_hat), x[:, -1, :, :, 0]
    dates, sums = ops.rollout_event_dates(y_hat, meshes, y, launch, persist=T)
    assert tuple(dates.shape) == (2, 2, 64 * 64) and tuple(sums.shape) == (2, 1, 8)
    with pytest.raises(ValueError, match='rollout_event_dates: y has'):
        ops.rollout_event_dates(y_hat, meshes, y[:, :2], launch, persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: launch has'):
        ops.rollout_event_dates(y_hat, meshes, y, launch[0], persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: launch has'):
        ops.rollout_event_dates(y_hat, meshes, y, y, persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: climatology has'):
        ops.rollout_event_dates(y_hat, meshes, y, launch, persist=2, climatology=y[:, :2])
    with pytest.raises(ValueError, match='rollout_event_dates: outputs must be fp32'):
        ops.rollout_event_dates([o.double() for o in y_hat], meshes, y, launch, persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: outputs must be fp32'):
        ops.rollout_event_dates([o.cpu() for o in y_hat], meshes, y, launch, persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: 3 output steps for 4 meshes'):
        ops.rollout_event_dates(y_hat[:3], meshes, y, launch, persist=2)
    with pytest.raises(ValueError, match='rollout_event_dates: kind must be'):
        ops.rollout_event_dates(y_hat, meshes, y, launch, kind='melt', persist=2)
    for bad in (0, T + 1, -1, 2.0):
        with pytest.raises(ValueError, match='rollout_event_dates: persist must be'):
            ops.rollout_event_dates(y_hat, meshes, y, launch, persist=bad)
    # outputs under autograd are detached, not refused
    outs, meshes = nfp.model(x, teacher_forcing_ratio=0)
    assert outs[0].requires_grad
    d2, s2 = ops.rollout_event_dates(outs, meshes, y, launch, persist=2)
    assert not d2.requires_grad and not s2.requires_grad
