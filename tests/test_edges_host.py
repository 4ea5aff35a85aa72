"""CPU-side checks of the ice-edge verification (no GPU): the numpy restatement of tests/edges_restated.py against fields worked
out by hand, qtmpnn.edges.EdgeDistance on hand numbers (perfect forecast, pooling, empty sets, pixel_km, skill, refusals), and the
qt_edge_rollout entry with its argument checks."""
import ctypes
import inspect
import math
import os
import re
import warnings

import numpy as np
import pytest

from edges_restated import edge_set, ice, restated_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ('n_f', 'n_o', 'sum_q_fo', 'sum_q_of', 'sum_d2_fo', 'sum_d2_of', 'max_d2_fo', 'max_d2_of')


def _f(a):
    return np.asarray(a, dtype=np.float32)[None]


def test_straight_edge_shifted_three_columns():
    """Ice in columns < 5 (truth) and < 8 (forecast) of a 6 x 12 frame: the edges are columns 4 and 7, every d2 = 9, q = 768."""
    y, f = np.zeros((6, 12), np.float32), np.zeros((6, 12), np.float32)
    y[:, :5], f[:, :8] = 1, 1
    keep = np.ones((6, 12), bool)
    ey, ef = edge_set(ice(y, keep, 0.5), keep), edge_set(ice(f, keep, 0.5), keep)
    assert np.argwhere(ey).tolist() == [[r, 4] for r in range(6)] and np.argwhere(ef).tolist() == [[r, 7] for r in range(6)]
    s = restated_edges(_f(f), _f(y), None, 0.5)
    assert s.dtype == np.int64 and s.shape == (1, 8)
    assert s[0].tolist() == [6, 6, 6 * 768, 6 * 768, 6 * 9, 6 * 9, 9, 9] and math.isqrt(65536 * 9) == 768


def test_single_pixels_at_opposite_corners():
    y, f = np.zeros((5, 9), np.float32), np.zeros((5, 9), np.float32)
    y[0, 0], f[4, 8] = 1, 1
    s = restated_edges(_f(f), _f(y), None, 0.5)[0]
    d2 = 4 * 4 + 8 * 8
    q = math.isqrt(65536 * d2)
    assert s.tolist() == [1, 1, q, q, d2, d2, d2, d2]
    assert q == 2289 and q * q <= 65536 * d2 < (q + 1) ** 2         # 256 * sqrt(80) = 2289.73..., rounded down


def test_all_ice_no_ice_borders_and_masked_pixels_make_no_edge():
    keep = np.ones((4, 6), bool)
    full, none = np.ones((4, 6), np.float32), np.zeros((4, 6), np.float32)
    half = none.copy()
    half[:, :3] = 1
    assert not edge_set(ice(full, keep, 0.5), keep).any() and not edge_set(ice(none, keep, 0.5), keep).any()
    # an empty set on either side: its own count is 0, and both directions' sums and maxima are 0
    assert restated_edges(_f(full), _f(half), None, 0.5)[0].tolist() == [0, 4, 0, 0, 0, 0, 0, 0]
    assert restated_edges(_f(half), _f(none), None, 0.5)[0].tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
    assert restated_edges(_f(none), _f(full), None, 0.5)[0].tolist() == [0] * 8
    # ice against the frame border only: no edge
    rim = none.copy()
    rim[0, :] = 1
    assert np.argwhere(edge_set(ice(rim, keep, 0.5), keep)).tolist() == [[0, c] for c in range(6)]          # open water below
    assert not edge_set(ice(full, keep, 0.5), keep).any()
    # ice whose only non-ice neighbours are masked: no edge; the mask neither forms nor blocks one
    mask = np.zeros((4, 6), bool)
    mask[:, 3] = True
    blocked = none.copy()
    blocked[:, :3] = 1                                       # ice in columns 0-2, column 3 is land, columns 4-5 open water
    assert not edge_set(ice(blocked, ~mask, 0.5), ~mask).any()
    assert restated_edges(_f(blocked), _f(blocked), mask, 0.5)[0].tolist() == [0] * 8
    # a masked pixel that would be ice is not ice, and is no open water either
    inner = full.copy()
    inner[1, 1] = 0
    assert edge_set(ice(inner, keep, 0.5), keep).sum() == 4
    hole = np.zeros((4, 6), bool)
    hole[1, 1] = True
    assert not edge_set(ice(inner, ~hole, 0.5), ~hole).any()
    # per-step counted (pixels without a node) act as the mask does
    counted = np.ones((1, 4, 6), bool)
    counted[0, :, 3] = False
    assert restated_edges(_f(blocked), _f(blocked), None, 0.5, counted)[0].tolist() == [0] * 8


def test_special_values_around_the_threshold():
    """thr itself and its lower fp32 neighbour, NaN and -inf are not ice; the upper neighbour and +inf are."""
    t = np.float32(0.15)
    vals = np.array([t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(1)), np.nan, np.inf, -np.inf], np.float32)
    keep = np.ones((1, 6), bool)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = ice(vals[None], keep, 0.15)
    assert got.tolist() == [[False, False, True, False, True, False]]
    # the threshold is rounded to fp32 once: compared with the float64 0.15, fp32(0.15) itself would be ice
    assert np.float64(t) > 0.15
    assert edge_set(got, keep).tolist() == [[False, False, True, False, True, False]]
    f = np.zeros((3, 6), np.float32)
    f[1] = vals
    s = restated_edges(_f(f), _f(f), None, 0.15)[0]
    assert s.tolist() == [2, 2, 0, 0, 0, 0, 0, 0]


def _ed(rows, sources=('model',)):
    """EdgeDistance from rows[clip][lead][source] of 8 integers."""
    from qtmpnn.edges import EdgeDistance
    return EdgeDistance(np.array(rows, dtype=np.int64), sources, 0.15)


def test_edge_distance_on_hand_numbers():
    from qtmpnn import edges
    assert edges.SLOTS == SLOTS
    # a perfect forecast through the restatement
    y = np.zeros((1, 6, 12), np.float32)
    y[:, :, :5] = 1
    s = restated_edges(y, y, None, 0.5)
    perfect = _ed(s[None, :, None])
    for fn in (perfect.displacement, perfect.modified_hausdorff, perfect.hausdorff, perfect.rms):
        assert fn().tolist() == [[0.0]]
    # one clip, one lead: n_f = 4, n_o = 2, directed means 2 and 5 pixels
    one = _ed([[[[4, 2, 4 * 2 * 256, 2 * 5 * 256, 20, 58, 9, 49]]]])
    assert one.displacement().tolist() == [[3.5]] and one.modified_hausdorff().tolist() == [[5.0]]
    assert one.hausdorff().tolist() == [[7.0]] and one.rms().tolist() == [[math.sqrt(78 / 6)]]
    # pooling: clip 0 means 1 and 1, clip 1 means 4 and 2 -> pooled fo (256 + 3 * 4 * 256) / 4 / 256 = 3.25, of (256 + 2 * 2 * 256)
    # / 3 / 256 = 5 / 3; the mean of the clips' displacements is (1 + 3) / 2 = 2
    two = _ed([[[[1, 1, 256, 256, 1, 1, 1, 1]]], [[[3, 2, 3 * 4 * 256, 2 * 2 * 256, 48, 8, 16, 4]]]])
    assert two.displacement()[:, 0].tolist() == [1.0, 3.0]
    lead = two.by_lead()
    assert lead['n_defined'].tolist() == [2] and lead['edge_length'].tolist() == [1.5]
    assert lead['displacement'].tolist() == [(3.25 + 5 / 3) / 2] and lead['displacement'][0] != two.displacement().mean()
    assert lead['modified_hausdorff'].tolist() == [3.25] and lead['hausdorff'].tolist() == [4.0]
    assert lead['rms'].tolist() == [math.sqrt(58 / 7)]
    km = two.by_lead(pixel_km=25)
    for k in ('displacement', 'modified_hausdorff', 'hausdorff', 'rms'):
        assert km[k].tolist() == (lead[k] * 25).tolist()
    assert km['n_defined'].tolist() == [2] and km['edge_length'].tolist() == [1.5]


def test_pairs_with_an_empty_set_are_nan_and_left_out_of_the_pool():
    # lead 0: clip 1 has no forecast edge (its n_o must not enter edge_length); lead 1: no clip is defined
    r = _ed([[[[2, 2, 2 * 256, 2 * 256 * 3, 2, 18, 1, 9]], [[0, 3, 0, 0, 0, 0, 0, 0]]],
             [[[0, 40, 0, 0, 0, 0, 0, 0]], [[5, 0, 0, 0, 0, 0, 0, 0]]]])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for fn in (r.displacement, r.modified_hausdorff, r.hausdorff, r.rms):
            v = fn()
            assert v.shape == (2, 2) and np.isnan(v).tolist() == [[False, True], [True, True]]
        lead = r.by_lead()
    assert lead['n_defined'].tolist() == [1, 0] and lead['edge_length'][0] == 2.0 and np.isnan(lead['edge_length'][1])
    assert lead['displacement'][0] == 2.0 and lead['hausdorff'][0] == 3.0
    for k in ('displacement', 'modified_hausdorff', 'hausdorff', 'rms'):
        assert np.isnan(lead[k][1])


def test_skill_against_a_reference():
    row = lambda mean: [2, 2, 2 * mean * 256, 2 * mean * 256, 0, 0, 0, 0]
    r = _ed([[[row(1), row(4)], [row(6), row(4)], [row(3), [0] * 8]]], ('model', 'persistence'))
    assert r.skill().tolist()[:2] == [0.75, -0.5] and np.isnan(r.skill()[2])
    assert r.skill('model', 'model')[:2].tolist() == [0.0, 0.0] and r.skill().shape == (3,)
    with pytest.raises(KeyError, match='skill: no source .climatology.'):
        r.skill(reference='climatology')


def test_edge_distance_refuses_by_name():
    from qtmpnn.edges import EdgeDistance
    s = np.zeros((2, 3, 2, 8), dtype=np.int64)
    src = ('model', 'persistence')
    for bad in (s[0], s[..., :7], s[:, :, :1], s.reshape(2, 3, 16), s[..., None]):
        with pytest.raises(ValueError, match='EdgeDistance: sums of shape'):
            EdgeDistance(bad, src, 0.15)
    with pytest.raises(ValueError, match='EdgeDistance: sums must be integers'):
        EdgeDistance(s.astype(np.float64), src, 0.15)
    with pytest.raises(ValueError, match='EdgeDistance: sources'):
        EdgeDistance(s, ('model', 'model'), 0.15)
    r = EdgeDistance(s.astype(np.int32), src, 0.15)
    assert r.sums.dtype == np.int64 and r.threshold == 0.15 and r.sources == src
    for fn in (r.displacement, r.modified_hausdorff, r.hausdorff, r.rms, r.by_lead):
        with pytest.raises(KeyError, match='climatology'):
            fn('climatology')


def test_edge_entry_is_declared_exported_and_bound():
    from helpers import binding_kinds, header_decls
    from qtmpnn import _lib
    name = 'qt_edge_rollout'
    decls = header_decls()
    decl = decls[name]
    assert re.match(r'int\s+qt_edge_rollout\s*\(', decl.text) and decl.times == 1
    # header and table hold each other (tests/test_host_cpu.py does so for every entry): per argument a pointer, an int, an
    # int64 or a float in the same place
    edge = _lib._SIGNATURES[name]
    assert decl.kinds == binding_kinds(edge)
    assert re.search(r'int\s+m\s*,\s*uint64_t\s*\*\s*planes\s*,\s*int32_t\s*\*\s*partial\s*,\s*void\s*\*\s*stream\s*\)', decl.text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.exported_names()
    assert _lib.load().qt_edge_rollout.argtypes == edge and _lib.load().qt_edge_rollout.restype is ctypes.c_int
    # the 20 leading arguments are qt_score_rollout's, in the binding and in the header's text
    assert edge[:20] == _lib._SIGNATURES['qt_score_rollout'][:20] == _lib._SIGNATURES['qt_fss_rollout'][:20]
    assert decl.params[:20] == decls['qt_score_rollout'].params[:20]
    assert edge[20:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.qt_abi_version() == 1
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert f'({len(_lib.exported_names())} entry points)' in readme and not re.search(r'qtmpnn_\w+\.h', readme)


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_void_p * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_edge_entry_refuses_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    one = (ctypes.c_int * 17)(*([1] * 17))
    ptrs = (ctypes.c_void_p * 17)(*([x] * 17))

    def call(nseg=1, outs=ptrs, strides=one, labels=ptrs, Ns=one, n_devs=ptrs, y=x, ycs=64, yss=64, b1=None, b1cs=0, b1ss=0,
             b2=None, b2cs=0, b2ss=0, pm=None, thr=0.5, B=1, n=8, m=8, planes=x, partial=x):
        rc = lib.qt_edge_rollout(nseg, outs, strides, labels, Ns, n_devs, y, ycs, yss, b1, b1cs, b1ss, b2, b2cs, b2ss, pm, thr, B,
                                 n, m, planes, partial, None)
        return rc, lib.qt_last_error()

    bad = [dict(nseg=0), dict(nseg=17), dict(nseg=-1), dict(outs=None), dict(strides=None), dict(labels=None), dict(Ns=None),
           dict(n_devs=None), dict(y=None), dict(partial=None), dict(planes=None),
           dict(B=0), dict(B=-3), dict(B=65536), dict(n=0), dict(m=0), dict(m=-8),
           dict(n=257), dict(m=257), dict(n=257, m=257), dict(n=1 << 20, m=1 << 20),
           dict(ycs=-1), dict(yss=-64), dict(b1=x, b1cs=-1), dict(b1=x, b1ss=-1), dict(b2=x, b2cs=-1), dict(b2=x, b2ss=-1),
           dict(labels=(ctypes.c_void_p * 16)()), dict(strides=(ctypes.c_int * 16)())]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1 and b'qt_edge_rollout' in err, (kw, rc, err)
    assert b'qt_edge_rollout: nseg' in call(nseg=17)[1]
    assert b'negative stride' in call(b2=x, b2ss=-1)[1]
    assert b'bad segment' in call(strides=(ctypes.c_int * 16)())[1]
    assert b'null planes / partial' in call(partial=None)[1] and b'null planes / partial' in call(planes=None)[1]
    assert b'bad sizes' in call(B=0)[1]
    assert b'larger than 256 x 256' in call(n=257)[1] and b'larger than 256 x 256' in call(n=8, m=300)[1]
    assert lib.qt_edge_rollout(17, None, None, None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0.5, 1, 8, 8, None,
                               None, None) == -1
    assert b'qt_edge_rollout' in lib.qt_last_error()


def test_edge_distance_is_a_method_beside_score():
    from model import mpnnlstm
    from model.mpnnlstm import NextFramePredictorS2S
    from qtmpnn import ops
    from qtmpnn.edges import EdgeDistance
    score = inspect.signature(NextFramePredictorS2S.score).parameters
    edge = inspect.signature(NextFramePredictorS2S.edge_distance).parameters
    assert list(edge) == list(score)
    for name, p in score.items():
        assert edge[name].default == p.default, name
    graphed = inspect.signature(NextFramePredictorS2S.make_graphed_edges).parameters
    assert list(graphed) == ['self', 'x', 'y', 'concat_layers', 'mask', 'high_interest_region', 'graph_structure', 'threshold']
    assert graphed['threshold'].default == 0.15 and graphed['concat_layers'].default is None
    params = inspect.signature(ops.rollout_edges).parameters
    assert list(params) == ['outputs', 'meshes', 'y', 'threshold', 'persistence', 'climatology', 'per_tile']
    assert params['threshold'].default == 0.15 and params['per_tile'].default is False
    assert list(inspect.signature(mpnnlstm.edge_product).parameters) == ['threshold']
    assert list(inspect.signature(EdgeDistance.__init__).parameters) == ['self', 'sums', 'sources', 'threshold']


class _Mesh:
    def __init__(self, n, m, B=1):
        self.n, self.m, self.B, self.P = n, m, B, n * m


def test_rollout_edges_refuses_before_any_launch(monkeypatch):
    """No GPU here: every refusal comes before the library is touched."""
    import torch
    from qtmpnn import _lib, ops
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]))
    with pytest.raises(ValueError, match='rollout_edges: 0 output steps for'):
        ops.rollout_edges([], [], None)
    with pytest.raises(ValueError, match='rollout_edges: 1 output steps for 2 meshes'):
        ops.rollout_edges([torch.zeros(4, 1)], [_Mesh(2, 2)] * 2, torch.zeros(4))
    with pytest.raises(ValueError, match='rollout_edges: outputs must be fp32'):
        ops.rollout_edges([torch.zeros(4, 1)], [_Mesh(2, 2)], torch.zeros(4))
    assert launched == [] and ops.EDGE_MAX == 256
