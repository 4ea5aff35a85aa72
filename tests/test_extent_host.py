"""CPU-side checks of the regional extent verification (no GPU): the numpy restatement of tests/extent_restated.py on a frame
worked out by hand, qtmpnn.extent.Extent on synthetic sums (the IIEE identities, regions against their total, names, skill,
refusals), ops.check_regions, and the qt_extent_rollout entry with its argument checks."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from extent_restated import restated_extent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_frame():
    """4 x 6: columns 0-1 are region 0, columns 2-4 region 1, column 5 none; row i has area (i + 1) / 2; pixel (1, 3) is masked.
    Truth: 1 (ice) in columns 0-2, 0.25 elsewhere; forecast: 0.75 (ice) in columns 1-3, 0 elsewhere; thr 0.5."""
    regions = np.array([[0, 0, 1, 1, 1, -1]] * 4)
    areas = np.repeat(np.array([0.5, 1.0, 1.5, 2.0], np.float32)[:, None], 6, axis=1)
    counted = np.ones((4, 6), bool)
    counted[1, 3] = False
    y = np.full((1, 4, 6), 0.25, np.float32)
    y[:, :, :3] = 1.0
    f = np.zeros((1, 4, 6), np.float32)
    f[:, :, 1:4] = 0.75
    return f, y, counted, regions, areas


def test_restatement_on_a_frame_worked_out_by_hand():
    f, y, counted, regions, areas = _hand_frame()
    sums, absterms = restated_extent([f], y, counted, regions, areas, 0.5, 2)
    assert sums.shape == absterms.shape == (1, 2, 2, 4) and sums.dtype == np.float64
    # region 0: 8 pixels of area 2 * 5; all ice in the truth; the forecast has column 1 only (area 5): U = column 0
    assert sums[0, 0].tolist() == [[8, 10, 10, 10], [5, 3.75, 0, 5]]
    # region 1: 11 pixels of area 15 - 1; truth ice in column 2 (5), forecast in columns 2 and 3 (5 + 4): O = column 3
    assert sums[0, 1].tolist() == [[11, 14, 5, 5 + 0.25 * 4 + 0.25 * 5], [9, 0.75 * 9, 4, 0]]
    assert np.array_equal(absterms, sums)                      # no negative term
    # the regionless column and the masked pixel add nothing: giving them wild values changes no slot
    f2, y2 = f.copy(), y.copy()
    f2[:, :, 5], y2[:, :, 5], f2[0, 1, 3], y2[0, 1, 3] = 9.0, np.nan, np.nan, 7.0
    again, _ = restated_extent([f2], y2, counted, regions, areas, 0.5, 2)
    assert np.array_equal(again, sums)
    # defaults: no map is one region of every counted pixel with unit areas
    unit, _ = restated_extent([f], y, counted, None, None, 0.5, 1)
    assert unit[0, 0].tolist() == [[23, 23, 12, 12 + 0.25 * 11], [11, 0.75 * 11, 3, 4]]
    # a label beyond R is no region
    one, _ = restated_extent([f], y, counted, regions, areas, 0.5, 1)
    assert np.array_equal(one[0, 0], sums[0, 0])
    # strict >: the threshold itself is not ice; a NaN is not ice and makes its own SIA NaN only
    edge = f.copy()
    edge[0, 0, 1], edge[0, 2, 2] = 0.5, np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got, _ = restated_extent([edge], y, counted, regions, areas, 0.5, 2)
    assert got[0, 0, 1].tolist() == [4.5, 3.75 - 0.5 * 0.25, 0, 5.5] and np.array_equal(got[0, :, 0], sums[0, :, 0])
    assert np.isnan(got[0, 1, 1, 1]) and got[0, 1, 1, [0, 2, 3]].tolist() == [9 - 1.5, 4, 1.5]


def _extent(clips, sources=('model',), names=None, **kw):
    """Extent from clips[c] = (fields [S x (T, W, H)], truth (T, W, H)) through the restatement."""
    from qtmpnn.extent import Extent
    R = kw.pop('R')
    sums = np.stack([restated_extent(f, y, kw.get('counted', np.ones(y.shape[1:], bool)), kw.get('regions'), kw.get('areas'),
                                     0.5, R)[0] for f, y in clips])
    return Extent(sums, sources, 0.5, names)


def _blob(r0, r1, c0, c1, shape=(12, 16)):
    a = np.zeros((1, *shape), np.float32)
    a[:, r0:r1, c0:c1] = 1.0
    return a


def test_extent_identities_on_synthetic_sums():
    areas = np.repeat(np.linspace(0.5, 2.0, 12, dtype=np.float32)[:, None], 16, axis=1)
    regions = np.where(np.arange(16) < 8, 0, 1)[None].repeat(12, axis=0)
    regions[:, 15] = -1
    truth = _blob(3, 8, 1, 5) + _blob(2, 9, 9, 13)
    shifted = _blob(3, 8, 2, 6) + _blob(2, 9, 9, 13)          # region 0's blob moved one column, inside the region
    grown = _blob(2, 9, 0, 6) + _blob(1, 10, 8, 14)            # both blobs with a ring of one pixel around them
    rng = np.random.default_rng(3)
    noise = [rng.random((1, 12, 16), dtype=np.float32) for _ in range(3)]
    mixed = _blob(2, 9, 0, 6) + _blob(3, 8, 10, 12)            # west grown, east shrunk: errors of opposite sign
    ex = _extent([([shifted, grown], truth), ([noise[0], noise[1]], noise[2]), ([mixed, noise[1]], truth)],
                 ('model', 'persistence'), ('west', 'east'), regions=regions, areas=areas, R=2)
    assert ex.sums.shape == (3, 1, 2, 3, 4) and ex.region_names == ('west', 'east') and ex.threshold == 0.5
    for s in ('observed', 'model', 'persistence'):
        np.testing.assert_allclose(ex.iiee(s), ex.aee(s) + ex.me(s), rtol=0, atol=1e-12)
        np.testing.assert_allclose(ex.error(s), ex.over(s) - ex.under(s), rtol=0, atol=1e-12)
        np.testing.assert_allclose(ex.aee(s), np.abs(ex.error(s)), rtol=0, atol=1e-12)
        assert ex.extent(s).shape == ex.area(s).shape == ex.total_area().shape == (3, 1, 2)
    assert (ex.iiee('observed') == 0).all() and (ex.error('observed', 'area') == 0).all()
    assert np.array_equal(ex.extent('observed'), ex.sums[:, :, :, 0, 2]) and np.array_equal(ex.area('observed'), ex.sums[:, :, :, 0, 3])
    # a shift inside the region keeps its extent: all of its error is misplacement
    assert ex.aee('model')[0, 0, 0] == 0 and ex.me('model')[0, 0, 0] == ex.iiee('model')[0, 0, 0] > 0
    assert ex.iiee('model')[0, 0, 1] == 0                      # the east blob is where it was
    # growth only over-forecasts: no misplacement
    assert (ex.me('persistence')[0, 0] == 0).all() and (ex.under('persistence')[0, 0] == 0).all()
    assert (ex.aee('persistence')[0, 0] == ex.iiee('persistence')[0, 0]).all() and (ex.iiee('persistence')[0, 0] > 0).all()
    # the regions add up to the total, and AEE of the total cannot exceed the regions' AEE added
    tot = ex.total()
    assert tot.sums.shape == (3, 1, 1, 3, 4) and tot.region_names == ('total',) and tot.sources == ex.sources
    for s in ('observed', 'model', 'persistence'):
        np.testing.assert_allclose(tot.extent(s)[..., 0], ex.extent(s).sum(axis=-1), rtol=0, atol=1e-12)
        np.testing.assert_allclose(tot.area(s)[..., 0], ex.area(s).sum(axis=-1), rtol=0, atol=1e-12)
        assert (tot.aee(s)[..., 0] <= ex.aee(s).sum(axis=-1) + 1e-12).all()
        np.testing.assert_allclose(tot.iiee(s)[..., 0], ex.iiee(s).sum(axis=-1), rtol=0, atol=1e-12)
    assert 0 < tot.aee('model')[2, 0, 0] < ex.aee('model')[2].sum()      # opposite signs: the regions' errors partly cancel
    np.testing.assert_allclose(tot.total_area()[..., 0], ex.total_area().sum(axis=-1))
    # by_lead: a name is its index; None is the total
    for s in ('model', 'persistence'):
        by_name, by_index, all_regions = ex.by_lead(s, region='east'), ex.by_lead(s, region=1), ex.by_lead(s)
        assert list(by_name) == list(by_index) == list(all_regions)
        for k in by_name:
            assert np.array_equal(by_name[k], by_index[k]) and by_name[k].shape == (1,), k
            assert np.array_equal(all_regions[k], tot.by_lead(s, region=0)[k]), k
    lead = ex.by_lead('model', 'west')
    assert lead['n_clips'].tolist() == [3]
    err = ex.error('model')[:, 0, 0]
    assert lead['extent_bias'][0] == err.mean() and lead['extent_mae'][0] == np.abs(err).mean()
    assert lead['extent_rmse'][0] == np.sqrt((err * err).mean())
    assert lead['observed_extent'][0] == ex.extent('observed')[:, 0, 0].mean()
    assert lead['forecast_area'][0] == ex.area('model')[:, 0, 0].mean()
    assert lead['iiee'][0] == ex.iiee('model')[:, 0, 0].mean() and lead['me'][0] == ex.me('model')[:, 0, 0].mean()
    assert set(lead) == {'n_clips', 'observed_extent', 'forecast_extent', 'extent_bias', 'extent_mae', 'extent_rmse',
                         'observed_area', 'forecast_area', 'area_bias', 'area_mae', 'area_rmse', 'iiee', 'aee', 'me'}
    # skill: a source against itself is 0; against another it is 1 - the ratio of the means
    for metric in ('iiee', 'aee', 'me'):
        assert ex.skill('model', 'model', metric).tolist() == [0.0]
    assert ex.skill('model').tolist() == [1 - tot.iiee('model')[:, 0, 0].mean() / tot.iiee('persistence')[:, 0, 0].mean()]


def test_extent_refuses_by_name_and_empty_regions_are_quiet():
    from qtmpnn.extent import Extent
    s = np.zeros((2, 3, 2, 3, 4))
    src = ('model', 'persistence')
    for bad in (s[0], s[..., :3], s[:, :, :, :2], s[..., None]):
        with pytest.raises(ValueError, match='Extent: sums of shape'):
            Extent(bad, src, 0.15)
    with pytest.raises(ValueError, match='Extent: sources'):
        Extent(s, ('model', 'model'), 0.15)
    with pytest.raises(ValueError, match='Extent: sources'):
        Extent(s, ('model', 'observed'), 0.15)
    for names in (('a',), ('a', 'a'), ('a', 'b', 'c')):
        with pytest.raises(ValueError, match='Extent: region_names'):
            Extent(s, src, 0.15, names)
    ex = Extent(s.astype(np.float32), src, 0.15)
    assert ex.sums.dtype == np.float64 and ex.region_names == ('region0', 'region1') and ex.sources == src
    for fn in (ex.extent, ex.area, ex.iiee, ex.aee, ex.me, ex.error, ex.by_lead, ex.over, ex.under):
        with pytest.raises(KeyError, match='climatology'):
            fn('climatology')
    with pytest.raises(KeyError, match='skill: no source .climatology.'):
        ex.skill(reference='climatology')
    for bad in ('north', 2, -1, 1.0, True):
        with pytest.raises(KeyError, match='no region'):
            ex.by_lead('model', region=bad)
    with pytest.raises(ValueError, match='what must be'):
        ex.error('model', 'volume')
    with pytest.raises(ValueError, match='metric must be'):
        ex.skill(metric='rmse')
    # regions without a counted pixel: zeros, and NaN where a ratio has nothing below it -- no warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert (ex.extent() == 0).all() and (ex.iiee() == 0).all() and (ex.total_area() == 0).all()
        assert np.isnan(ex.concentration()).all() and np.isnan(ex.skill()).all()
        assert ex.by_lead('model', 'region1')['extent_rmse'].tolist() == [0, 0, 0]


def test_check_regions():
    from qtmpnn import ops
    shape = (4, 6)
    assert ops.check_regions('w', None, None, shape) == (None, None, 1)
    regions = np.array([[0, 0, 1, 1, 4, -1]] * 4)
    regions[2, 0] = -7
    region, area, R = ops.check_regions('w', regions, np.full(shape, 2.5), shape)
    assert R == 5 and region.dtype == np.int8 and region.shape == shape and region.flags.c_contiguous
    assert region[2, 0] == -1 and region[0, 5] == -1 and np.array_equal(region >= 0, regions >= 0)
    assert np.array_equal(region[regions >= 0], regions[regions >= 0])
    assert area.dtype == np.float32 and area.shape == shape and (area == 2.5).all()
    # a float map of whole numbers, an unsigned one, and a map without any region
    assert ops.check_regions('w', regions.astype(np.float64), None, shape)[2] == 5
    assert ops.check_regions('w', np.full(shape, 31, np.uint8), None, shape)[2] == 32
    none, _, R = ops.check_regions('w', np.full(shape, -3), None, shape)
    assert R == 1 and (none == -1).all()
    # labels far below int8 stay "no region"
    assert (ops.check_regions('w', np.full(shape, -300), None, shape)[0] == -1).all()
    import torch
    r_t, a_t, R = ops.check_regions('w', torch.from_numpy(regions), torch.full(shape, 0.0), shape)
    assert R == 5 and np.array_equal(r_t, region) and (a_t == 0).all()
    with pytest.raises(ValueError, match='extent: regions of shape .6, 4. for frames of .4, 6.'):
        ops.check_regions('extent', regions.T, None, shape)
    with pytest.raises(ValueError, match='extent: areas of shape'):
        ops.check_regions('extent', None, np.ones(24), shape)
    with pytest.raises(ValueError, match='extent: regions must hold integers'):
        ops.check_regions('extent', regions + 0.5, None, shape)
    with pytest.raises(ValueError, match='extent: regions must hold integers'):
        ops.check_regions('extent', np.where(regions > 0, np.nan, 0.0), None, shape)
    with pytest.raises(ValueError, match='extent: regions must hold integers'):
        ops.check_regions('extent', regions > 0, None, shape)
    with pytest.raises(ValueError, match='extent: regions name 33 regions'):
        ops.check_regions('extent', np.full(shape, 32), None, shape)
    for bad in (np.nan, np.inf, -np.inf):
        a = np.ones(shape)
        a[1, 1] = bad
        with pytest.raises(ValueError, match='extent: areas must be finite'):
            ops.check_regions('extent', None, a, shape)
    with pytest.raises(ValueError, match='extent: areas must be finite'):
        ops.check_regions('extent', None, np.full(shape, 1e300), shape)
    a = np.ones(shape)
    a[3, 5] = -1e-9
    with pytest.raises(ValueError, match='make_graphed_extent: areas must not be negative'):
        ops.check_regions('make_graphed_extent', None, a, shape)


def test_extent_entry_is_declared_exported_and_bound():
    from helpers import HEADER, binding_kinds, header_decls
    from qtmpnn import _lib
    name = 'qt_extent_rollout'
    decls = header_decls()
    decl = decls[name]
    assert re.match(r'int\s+qt_extent_rollout\s*\(', decl.text)
    ext = _lib._SIGNATURES[name]
    assert decl.kinds == binding_kinds(ext)
    # the 20 leading arguments are qt_score_rollout's, unchanged
    assert decl.params[:20] == decls['qt_score_rollout'].params[:20]
    assert ext[:20] == _lib._SIGNATURES['qt_score_rollout'][:20] == _lib._SIGNATURES['qt_reliability_rollout'][:20]
    assert re.search(r'int\s+m\s*,\s*const\s+int8_t\s*\*\s*region\s*,\s*const\s+float\s*\*\s*area\s*,\s*int\s+R\s*,\s*'
                     r'float\s*\*\s*partial\s*,\s*void\s*\*\s*stream\s*\)', decl.text)
    assert ext[20:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # declared once in the one header, bound in the one table
    assert decl.times == 1
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names()
    assert _lib.load().qt_extent_rollout.argtypes == ext and _lib.load().qt_extent_rollout.restype is ctypes.c_int
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert len(_lib.exported_names()) == 91 and '(91 entry points)' in readme and not re.search(r'qtmpnn_\w+\.h', readme)
    # the slot table and the NaN rule are stated where the entry is declared: in the comment that ends at the declaration
    header = open(HEADER).read()
    doc = header[:header.index(decl.text)].rsplit('/*', 1)[1]
    assert doc.startswith(' qt_extent_rollout:') and doc.rstrip().endswith('*/')
    for word in ('E_o', 'SIA_o', 'O_s', 'U_s', 'NaN'):
        assert word in doc, word


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_extent_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.5, B=1, n=8, m=8, region=x, area=x, R=2, partial=x):
        rc = lib.qt_extent_rollout(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm, thr,
                                   B, n, m, region, area, R, partial, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(outs=None), dict(strides=None), dict(labels=None), dict(Ns=None),
           dict(n_devs=None), dict(y=None), dict(partial=None), dict(R=0), dict(R=33), dict(R=-1),
           dict(R=33, region=None, area=None), dict(B=0), dict(B=-3), dict(B=65536), dict(n=0), dict(m=0), dict(m=-8),
           dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1), dict(b1=x, b1ss=-1), dict(b2=x, b2cs=-1), dict(b2=x, b2ss=-1),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_extent_rollout' in err, (kw, rc, err)
    assert b'qt_extent_rollout: nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(b2=x, b2ss=-1)[1]
    assert b'bad segment' in call(strides=(ctypes.c_int * 16)())[1]
    assert b'R must be 1..32' in call(R=0)[1] and b'R must be 1..32' in call(R=33)[1]
    assert b'null partial' in call(partial=None)[1]
    assert b'bad sizes' in call(B=0)[1]
    # the shared checks come first, as in qt_reliability_rollout
    assert b'nseg' in call(nseg=0, R=0)[1] and b'null pointer' in call(y=None, R=0)[1]
    assert lib.qt_extent_rollout(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.5, 1, 8, 8, None,
                                 None, 1, None, None) == -1
    assert b'qt_extent_rollout' in lib.qt_last_error()


def test_extent_is_a_method_beside_score():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    from qtmpnn.extent import Extent
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    ext = inspect.signature(NextFramePredictorS2S.extent).parameters
    assert list(ext) == list(score) + ['regions', 'areas', 'region_names']
    for name, p in score.items():
        assert ext[name].default == p.default, name
    assert all(ext[k].default is None for k in ('regions', 'areas', 'region_names'))
    scores = inspect.signature(NextFramePredictorS2S.make_graphed_scores).parameters
    graphed = inspect.signature(NextFramePredictorS2S.make_graphed_extent).parameters
    assert list(graphed) == [k for k in scores if k != 'maps'] + ['regions', 'areas']
    for name in graphed:
        if name in scores and name not in ('self', 'x', 'y'):
            assert graphed[name].default == scores[name].default, name
    params = inspect.signature(ops.rollout_extent).parameters
    assert list(params) == ['outputs', 'meshes', 'y', 'threshold', 'regions', 'areas', 'R', 'persistence', 'climatology', 'per_tile']
    assert params['threshold'].default == 0.15 and params['R'].default == 1 and params['per_tile'].default is False
    assert list(inspect.signature(ops.check_regions).parameters) == ['who', 'regions', 'areas', 'shape']
    assert list(inspect.signature(mpnnlstm.extent_product).parameters) == ['threshold', 'region_dev', 'area_dev', 'R']
    assert list(inspect.signature(Extent.__init__).parameters) == ['self', 'sums', 'sources', 'threshold', 'region_names']


class _Mesh:
    def __init__(self, n, m, B=1):
        self.n, self.m, self.B, self.P = n, m, B, n * m


def test_rollout_extent_refuses_before_any_launch(monkeypatch):
    """No GPU here: every refusal comes before the library is touched."""
    import torch
    from qtmpnn import _lib, ops
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    with pytest.raises(ValueError, match='rollout_extent: 0 output steps for'):
        ops.rollout_extent([], [], None)
    with pytest.raises(ValueError, match='rollout_extent: 1 output steps for 2 meshes'):
        ops.rollout_extent([torch.zeros(4, 1)], [_Mesh(2, 2)] * 2, torch.zeros(4))
    with pytest.raises(ValueError, match='rollout_extent: outputs must be fp32'):
        ops.rollout_extent([torch.zeros(4, 1)], [_Mesh(2, 2)], torch.zeros(4))
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match='rollout_extent: R must be an integer in 1..32'):
            ops.rollout_extent([torch.zeros(4, 1)], [_Mesh(2, 2)], torch.zeros(4), R=bad)
    assert launched == [] and ops.EXTENT_MAX_REGIONS == 32
