"""extent(): regional ice extent, ice area and over- / under-forecast areas on the GPU (qt_extent_rollout, ops.rollout_extent,
NextFramePredictorS2S.extent) against the float64 numpy restatement of tests/extent_restated.py.  At the op level the restatement
is fed the hand-made node values themselves (the 33 x 72 frame of tests/test_gpu_verify_rule.py: holes, stale labels, a mask,
three ragged tiles, a launch of 16 steps and one of 1); through extent() it is fed the project's own eager predict() frames of the
same model and inputs, so both sides read identical fp32 forecasts.

n is a count and must be equal.  Under unit areas A, E_o, E_s, O_s and U_s are counts too and must be equal.  Float slots: the
restatement forms its terms in float64 from the fp32 values and fp32 areas.  The kernel rounds a * y and a * f once (the terms of
A, E, O and U are a itself: no rounding), and a (region, tile) sum then passes through at most 3 rounded sequential adds per
thread (four pixels in pixel order, the first add to +0 is exact, pixels of other regions add +0 exactly), 6 butterfly steps and 2
combines: 12 roundings on the longest chain, plus 2 for the second-order terms, 14 <= 16.  So |gpu - f64| <= 16 * 2^-24 * sum
|term| per tile, region and slot and hence for the total (the tile totals are added in float64): the suite's EPS, with the bound
computed from the restatement's sum |term|."""
import copy
import functools

import numpy as np
import pytest
import torch

from extent_restated import restated_extent
from helpers import climatology_from_base, dev
from test_gpu_score import _case, _clips, _fields, _loader
from test_gpu_verify_rule import B, M_, N_, P, STALE, T, THR, _frame

pytestmark = pytest.mark.gpu

EPS = 16 * 2.0 ** -24
GAP = 13                                  # the column of -1
# (row, slot) pairs whose terms are a or 1: counts under unit areas
ROW0_COUNTS, SRC_COUNTS = (0, 1, 2), (0, 2, 3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def _regions(R):
    """(N_, M_) int64 region map: vertical bands of columns (72 columns per row against waves of 64 and tiles of 1024 flat
    pixels: every band border falls inside waves and inside tiles, in every row), column GAP of -1; for R > 1 region 1 holds
    exactly the pixels under the loss mask (no counted pixel) and, for R = 32, region 31 a single counted pixel."""
    labels, n_stale, mask, counted = _frame()
    reg = np.zeros((N_, M_), np.int64)
    if R > 1:
        ids = [r for r in range(R) if r != 1 and not (R == 32 and r == 31)]
        reg[:] = np.array(ids)[(np.arange(M_) * len(ids)) // M_][None]
        reg[mask] = 1
        if R == 32:
            assert counted[:, :, 20, 40].all()
            reg[20, 40] = 31
    reg[:, GAP] = -1
    assert reg.max() + 1 == R and (R == 1 or not counted[:, :, reg == 1].any())
    return reg


@functools.lru_cache(maxsize=None)
def _values(kind):
    """Three source fields, the truth (B, T, N_, M_) fp32 and the (N_, M_) areas (None: unit) of a case; persistence is one frame
    for every lead time.  'random': uniform values, unit areas.  'cosine': the same with the cosine of the row's latitude (50 to
    82 degrees north).  'exact': fields in multiples of 1/256 in [0, 1] and areas in multiples of 1/8 up to 4, so that a * f is a
    multiple of 1/2048 and a tile's sum at most 1024 * 4 = 2^23 such units: every partial sum is exact in fp32."""
    rng = np.random.default_rng({'random': 58, 'cosine': 58, 'exact': 59}[kind])
    if kind == 'exact':
        fields = [(rng.integers(0, 257, (B, T, N_, M_)) / 256).astype(np.float32) for _ in range(3)]
        y = (rng.integers(0, 257, (B, T, N_, M_)) / 256).astype(np.float32)
        areas = (rng.integers(0, 33, (N_, M_)) / 8).astype(np.float32)
        assert float(areas.max()) * 1024 * 2048 <= 2 ** 24 and (areas == 0).any()
    else:
        fields = [rng.random((B, T, N_, M_), dtype=np.float32) for _ in range(3)]
        y = rng.random((B, T, N_, M_), dtype=np.float32)
        areas = None
        if kind == 'cosine':
            areas = np.repeat(np.cos(np.deg2rad(np.linspace(50, 82, N_)))[:, None], M_, axis=1).astype(np.float32)
    fields[1] = np.repeat(fields[1][:, :1], T, axis=1)
    return fields, y, areas


@functools.lru_cache(maxsize=None)
def _restated(kind, S, R):
    """(sums, absterms), each (T, B, R, 1 + S, 4): made once per case, not modified."""
    counted = _frame()[3]
    fields, y, areas = _values(kind)
    reg = _regions(R)
    per_clip = [restated_extent([f[b] for f in fields[:S]], y[b], counted[b], reg, areas, THR, R) for b in range(B)]
    return tuple(np.stack([c[k] for c in per_clip], axis=1) for k in range(2))


def _operands(kind, S):
    """(outs, meshes, y, kw) on the device, as tests/test_gpu_verify_rule.py builds them: hand-made labels, a mask, step STALE with
    a smaller node count; outputs of B * P rows and 4 columns (column 0 carries the values, the others a decoy)."""
    from qtmpnn.mesh import build_pixel_mesh
    labels, n_stale, mask, counted = _frame()
    fields, y, areas = _values(kind)
    mesh = copy.copy(build_pixel_mesh(B, N_, M_, None, dev()))
    mesh.labels = _t(labels.reshape(B, N_, M_))
    mesh.loss_mask = _t(mask.astype(np.uint8))
    stale = copy.copy(mesh)
    stale.n_dev = torch.tensor([n_stale], dtype=torch.int32, device=dev())
    meshes = [mesh] * T
    meshes[STALE] = stale
    outs, node = [], labels >= 0
    for z in range(T):
        o = torch.full((B * P, 4), 0.87, device=dev())
        o[_t(labels[node].astype(np.int64)), 0] = _t(fields[0][:, z].reshape(B, P)[node])
        outs.append(o)
    kw = dict(persistence=_t(fields[1][:, 0]), climatology=_t(fields[2])) if S == 3 else {}
    return outs, meshes, _t(y), kw


def _maps(kind, R):
    from qtmpnn import ops
    region, area, R_map = ops.check_regions('test', _regions(R), _values(kind)[2], (N_, M_))
    assert R_map == R
    return _t(region).view(-1), None if area is None else _t(area).view(-1)


def _close(got, want, absterms, what, exact=()):
    """n equal, the (row, slot) pairs of `exact` equal, everything else within EPS * sum |term|; -> worst err / bound."""
    np.testing.assert_array_equal(got[..., 0, 0], want[..., 0, 0], err_msg=f'{what}: n')
    for row, slot in exact:
        np.testing.assert_array_equal(got[..., row, slot], want[..., row, slot], err_msg=f'{what}: row {row} slot {slot}')
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(EPS * absterms, 1e-300)))
    print(f'{what}: n per region {got[..., 0, 0].sum(axis=tuple(range(got.ndim - 3))).tolist()} | max err / bound {worst:.3f}')
    assert (err <= EPS * absterms).all(), (what, worst)
    return worst


def _count_slots(S):
    return [(0, k) for k in ROW0_COUNTS] + [(1 + s, k) for s in range(S) for k in SRC_COUNTS]


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('R', [1, 5, 32])
def test_op_unit_areas_counts_are_exact(R, S):
    """Unit areas: n, A, E_o, E_s, O_s and U_s are integers and equal the restatement's; the two SIA slots are within the bound.
    A second call gives the same bits, and the fp32 partials of the three tiles add up to the result."""
    from qtmpnn import ops
    outs, meshes, y, kw = _operands('random', S)
    region, area = _maps('random', R)
    assert area is None
    want, absterms = _restated('random', S, R)
    got = ops.rollout_extent(outs, meshes, y, THR, region, None, R, **kw)
    tiles = ops.rollout_extent(outs, meshes, y, THR, region, None, R, per_tile=True, **kw)
    assert got.shape == (T, B, R, 1 + S, 4) and got.dtype == torch.float64 and got.is_cuda and not got.requires_grad
    assert tiles.shape == (T, B, 3, R, 1 + S, 4) and tiles.dtype == torch.float32
    assert torch.equal(got, tiles.double().sum(2))
    assert torch.equal(got, ops.rollout_extent(outs, meshes, y, THR, region, None, R, **kw))
    got = got.cpu().numpy()
    for row, slot in _count_slots(S):
        assert (got[..., row, slot] == np.floor(got[..., row, slot])).all(), (row, slot)
    _close(got, want, absterms, f'unit R={R} S={S}', exact=_count_slots(S))
    counted = _frame()[3]
    reg = _regions(R)
    assert (got[..., 0, 0].sum(axis=2) == (counted & (reg >= 0)).sum(axis=(2, 3)).T).all()
    if R > 1:
        assert (got[:, :, 1] == 0).all() and (got[:, :, 0, 0, 0] > 0).all()      # the region under the mask adds nothing
    if R == 32:
        assert (got[:, :, 31, 0, :2] == 1).all()                                  # one pixel of area 1
    if R == 5:
        # labels at and above R are no region: the same map read with R = 3 gives the first three regions, bit for bit
        fewer = ops.rollout_extent(outs, meshes, y, THR, region, None, 3, **kw).cpu().numpy()
        assert np.array_equal(fewer, got[:, :, :3])


@pytest.mark.parametrize('S', [1, 3])
def test_no_maps_equals_rollout_scores_exactly(S):
    from qtmpnn import ops
    outs, meshes, y, kw = _operands('random', S)
    ext = ops.rollout_extent(outs, meshes, y, THR, **kw).cpu().numpy()
    sc = ops.rollout_scores(outs, meshes, y, THR, **kw).cpu().numpy()
    assert ext.shape == (T, B, 1, 1 + S, 4) and sc.shape == (T, B, S, 8)
    n, hits, over, under = (sc[..., k] for k in (0, 4, 5, 6))
    assert (n > 0).all() and (over > 0).all() and (under > 0).all()
    for s in range(S):
        np.testing.assert_array_equal(ext[:, :, 0, 0, 0], n[..., s], err_msg='n')
        np.testing.assert_array_equal(ext[:, :, 0, 0, 1], n[..., s], err_msg='A under unit areas')
        np.testing.assert_array_equal(ext[:, :, 0, 0, 2], (hits + under)[..., s], err_msg='E_o = hits + under')
        np.testing.assert_array_equal(ext[:, :, 0, 1 + s, 0], (hits + over)[..., s], err_msg='E_s = hits + over')
        np.testing.assert_array_equal(ext[:, :, 0, 1 + s, 2], over[..., s], err_msg='O_s = over')
        np.testing.assert_array_equal(ext[:, :, 0, 1 + s, 3], under[..., s], err_msg='U_s = under')


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('R', [1, 5, 32])
def test_op_cosine_areas_within_the_bound(R, S):
    from qtmpnn import ops
    outs, meshes, y, kw = _operands('cosine', S)
    region, area = _maps('cosine', R)
    want, absterms = _restated('cosine', S, R)
    got = ops.rollout_extent(outs, meshes, y, THR, region, area, R, **kw).cpu().numpy()
    assert np.isfinite(got).all()
    _close(got, want, absterms, f'cosine R={R} S={S}')
    # the same counts as under unit areas
    np.testing.assert_array_equal(got[..., 0, 0], _restated('random', S, R)[0][..., 0, 0])


def test_op_exact_case_is_equal_in_every_slot():
    """Areas in eighths up to 4 and fields in 1/256: every product and every partial sum is exact in fp32 (checked here for the
    largest tile sum), so all slots equal the float64 restatement."""
    from qtmpnn import ops
    S, R = 3, 5
    outs, meshes, y, kw = _operands('exact', S)
    region, area = _maps('exact', R)
    want, absterms = _restated('exact', S, R)
    assert absterms.max() * 2048 < 2 ** 24 and (absterms * 2048 == np.floor(absterms * 2048)).all()
    tiles = ops.rollout_extent(outs, meshes, y, THR, region, area, R, per_tile=True, **kw).cpu().numpy()
    assert (np.abs(tiles) * 2048 < 2 ** 24).all()
    got = ops.rollout_extent(outs, meshes, y, THR, region, area, R, **kw).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert (got[:, :, [0, 2, 3, 4], 1:, 1] > 0).all()


def test_nan_forecast_touches_its_own_sia_only():
    """A NaN node value in one region of one clip and step: that region's SIA of the model is NaN, its counts are what they were
    without the pixel's ice, and every other region, source, clip and step has the bits of the run without the NaN."""
    from qtmpnn import ops
    S, R, b0, z0, r0, c0 = 3, 5, 1, 2, 20, 40
    labels, n_stale, mask, counted = _frame()
    fields, yv, areas = _values('cosine')
    reg = _regions(R)
    r_nan = int(reg[r0, c0])
    assert counted[b0, z0, r0, c0] and r_nan >= 0 and r_nan != 1
    outs, meshes, y, kw = _operands('cosine', S)
    region, area = _maps('cosine', R)
    clean = ops.rollout_extent(outs, meshes, y, THR, region, area, R, **kw).cpu().numpy()
    outs[z0][int(labels[b0, r0 * M_ + c0]), 0] = float('nan')
    got = ops.rollout_extent(outs, meshes, y, THR, region, area, R, **kw).cpu().numpy()
    assert np.isnan(got).sum() == 1 and np.isnan(got[z0, b0, r_nan, 1, 1])
    # not ice: the pixel's area leaves E_model (and O_model or joins U_model) exactly as the restatement says
    f = [x[b0].copy() for x in fields[:S]]
    f[0][z0, r0, c0] = np.nan
    want, absterms = restated_extent(f, yv[b0], counted[b0], reg, areas, THR, R)
    keep = np.isfinite(want)
    assert (~keep).sum() == 1
    assert (np.abs(got[:, b0] - want)[keep] <= (EPS * absterms)[keep]).all()
    np.testing.assert_array_equal(got[:, b0, :, 0, 0], want[:, :, 0, 0])
    was_ice = fields[0][b0, z0, r0, c0] > np.float32(THR)
    assert (got[z0, b0, r_nan, 1, 0] < clean[z0, b0, r_nan, 1, 0]) == bool(was_ice)
    # everything but the model row of that (step, clip, region) is bit-identical
    same = np.ones(got.shape, bool)
    same[z0, b0, r_nan, 1] = False
    assert np.array_equal(got[same], clean[same])


# ---------------------------------------------------------------------------------------------------------------- predictor

NAMES = ('hudson', 'foxe', 'strait')


def _maps64(mask):
    """Three named regions of a 64 x 64 frame (bands of columns; the last row in none), cell areas of a latitude-longitude grid."""
    from model.utils import cell_area_weights
    reg = np.digitize(np.arange(64), [20, 45])[None].repeat(64, axis=0)
    reg[63] = -1
    return reg, cell_area_weights(np.linspace(52.0, 67.75, 64), 64)


@functools.lru_cache(maxsize=None)
def _reference(with_clim):
    """(predictor, loader, climatology, kwargs, per-clip fields from eager predict()): made once per case, not modified.  The
    64 x 64 quadtree model with a land mask: batches of 2, 2 and 1 clips, or with a climatology its first three clips one by one."""
    nfp, loader, clim, extra = _case('quadtree_masked_64')
    nfp.model.eval()
    if with_clim:
        x = np.concatenate([item[0].numpy() for item in loader])[:3]
        y = np.concatenate([item[1].numpy() for item in loader])[:3]
        loader = _loader(x, y, [1, 1, 1], (64, 64))
        base = np.random.default_rng(11).random((64, 64), dtype=np.float32)
        clim = torch.from_numpy(climatology_from_base(base)).to(dev())
    return nfp, loader, clim, extra, _fields(nfp, loader, clim, extra)


def _check(ex, fields, loader, mask, regions, areas, thr, what, exact=()):
    clips = _clips(loader)
    R = int(regions.max()) + 1 if regions is not None else 1
    assert ex.sums.shape == (len(clips), fields[0]['model'].shape[0], R, 1 + len(ex.sources), 4) and ex.sums.dtype == np.float64
    assert ex.sources == tuple(fields[0])
    for c, (x, y, launch) in enumerate(clips):
        want, absterms = restated_extent([fields[c][name].astype(np.float32) for name in ex.sources], y.astype(np.float32),
                                         ~mask, regions, areas, thr, R)
        _close(ex.sums[c], want, absterms, f'{what} clip {c}', exact)


@pytest.mark.parametrize('with_clim', [False, True])
def test_extent_equals_restatement(with_clim):
    nfp, loader, clim, extra, fields = _reference(with_clim)
    regions, areas = _maps64(extra['mask'])
    ex = nfp.extent(loader, clim, regions=regions, areas=areas, region_names=NAMES, **extra)
    S = 3 if with_clim else 2
    assert ex.sources == ('model', 'persistence') + (('climatology',) if with_clim else ()) and ex.region_names == NAMES
    assert ex.threshold == 0.15 and nfp.model.static_shapes is False
    _check(ex, fields, loader, extra['mask'], regions, areas, 0.15, f'areas clim={with_clim}')
    unit = nfp.extent(loader, clim, regions=regions, region_names=NAMES, **extra)
    _check(unit, fields, loader, extra['mask'], regions, None, 0.15, f'unit clim={with_clim}', exact=_count_slots(S))
    # every unmasked pixel that is in a region is counted, at every lead time
    want_n = [int((~extra['mask'] & (regions == r)).sum()) for r in range(3)]
    assert (ex.n() == np.array(want_n)).all() and (unit.total_area() == unit.n()).all()
    np.testing.assert_array_equal(ex.n(), unit.n())
    # the derived numbers hang together on real sums
    for s in ex.sources:
        np.testing.assert_allclose(ex.iiee(s), ex.aee(s) + ex.me(s), rtol=0, atol=1e-9)
        # E_s - E_o = O_s - U_s in exact arithmetic; the four are separate fp32 sums, each within EPS of its own size
        slack = EPS * (ex.extent(s) + ex.extent('observed') + ex.over(s) + ex.under(s))
        assert (np.abs(ex.aee(s) - np.abs(ex.error(s))) <= slack).all(), s
        assert np.array_equal(unit.aee(s), np.abs(unit.error(s)))             # counts: exact
    lead = ex.by_lead('model', 'foxe')
    assert np.array_equal(lead['iiee'], ex.iiee('model')[:, :, 1].mean(axis=0)) and lead['n_clips'][0] == len(_clips(loader))
    assert ex.skill('model', 'persistence').shape == (ex.sums.shape[1],)


def test_graphed_extent_equals_eager_bit_for_bit():
    """Batches of 2, 2 and 1 clips: two captured shapes, one replay."""
    nfp, loader, clim, extra, _ = _reference(False)
    regions, areas = _maps64(extra['mask'])
    kw = dict(regions=regions, areas=areas, region_names=NAMES, **extra)
    assert len({tuple(item[0].shape) for item in loader}) == 2
    nfp.model.static_shapes = True
    static = nfp.extent(loader, clim, **kw)
    nfp.model.static_shapes = False
    graphed = nfp.extent(loader, clim, use_graph=True, **kw)
    assert nfp.model.static_shapes is False
    assert graphed.sources == static.sources and graphed.sums.shape == static.sums.shape
    assert np.array_equal(graphed.sums, static.sums), float(np.abs(graphed.sums - static.sums).max())
    assert graphed.sums[..., 0, 0].sum() > 0 and graphed.region_names == NAMES
    again = nfp.extent(loader, clim, use_graph=True, **kw)
    assert np.array_equal(again.sums, graphed.sums)


def test_extent_without_maps_agrees_with_score_exactly():
    nfp, loader, clim, extra, _ = _reference(True)
    ex = nfp.extent(loader, clim, **extra)
    sc = nfp.score(loader, clim, **extra)
    assert ex.sources == sc.sources and len(ex.sources) == 3 and ex.region_names == ('region0',)
    assert ex.sums.shape == sc.sums.shape[:2] + (1, 4, 4)
    n, hits, over, under = (sc.sums[..., k] for k in (0, 4, 5, 6))           # (clips, T, S)
    for s, name in enumerate(ex.sources):
        np.testing.assert_array_equal(ex.n()[..., 0], n[..., s])
        np.testing.assert_array_equal(ex.total_area()[..., 0], n[..., s])
        np.testing.assert_array_equal(ex.extent('observed')[..., 0], (hits + under)[..., s])
        np.testing.assert_array_equal(ex.extent(name)[..., 0], (hits + over)[..., s])
        np.testing.assert_array_equal(ex.over(name)[..., 0], over[..., s])
        np.testing.assert_array_equal(ex.under(name)[..., 0], under[..., s])
        np.testing.assert_array_equal(ex.iiee(name)[..., 0], (over + under)[..., s])
    assert over.sum() > 0 and under.sum() > 0


def test_extent_refuses_bad_maps_before_any_launch(monkeypatch):
    from qtmpnn import _lib
    nfp, loader, clim, extra, _ = _reference(False)
    regions, areas = _maps64(extra['mask'])
    x, y, _ = loader[0]
    x, y = x.to(dev()), y.to(dev())
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    negative = areas.copy()
    negative[5, 5] = -0.5
    with pytest.raises(ValueError, match='extent: regions of shape .64, 32. for frames of .64, 64.'):
        nfp.extent(loader, clim, regions=regions[:, :32], areas=areas, **extra)
    with pytest.raises(ValueError, match='extent: areas must not be negative'):
        nfp.extent(loader, clim, regions=regions, areas=negative, **extra)
    with pytest.raises(ValueError, match='extent: region_names must be 3 distinct names'):
        nfp.extent(loader, clim, regions=regions, areas=areas, region_names=('a', 'b'), **extra)
    with pytest.raises(ValueError, match='make_graphed_extent: regions of shape'):
        nfp.make_graphed_extent(x, y, regions=regions.T[:32], **extra)
    with pytest.raises(ValueError, match='make_graphed_extent: areas must not be negative'):
        nfp.make_graphed_extent(x, y, areas=negative, **extra)
    assert launched == [] and nfp.model.static_shapes is False
