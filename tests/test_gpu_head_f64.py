"""The decoder head's input -- qt_head_fwd / qt_head_bwd (csrc/lstm.hip: k_head_fwd<LPN>, k_head_bwd<LPN>, LPN = 2 .. 32) with
qt_colsum over their slabs, through the C ABI and through ops.head_input (GradAcc included) -- against the float64 model
tests/head_f64.py.

Every comparison is kernel against model, never kernel against kernel.  Bounds are derived beside the model (twice a count of
float32 roundings times 2^-24 times the majorant, propagated through the LayerNorm); data movement (Zb, gconcat, zero pad columns)
has bound 0.  Outputs and slabs of the raw calls are pre-filled with the sentinel -7.25; capacity rows of inputs are NaN, and O
also comes as the column view gates[:, 3h:4h] of a matrix whose other columns are NaN.  Entries whose float64 pre-activation lies
within the forward bound of the ReLU kink carry no cotangent and are compared against both branches (at most 0.1 % of a case:
tests/test_head_f64_host.py).  Every case prints its worst error / bound before it asserts (pytest -s; a recorded run:
profiles/head_pack_f64.txt).  tests/test_head_f64_host.py names, per mutation, the case here that sees it."""
import numpy as np
import pytest
import torch

import head_f64 as M
from helpers import dev
from test_gpu_cheb_f64 import compare

pytestmark = pytest.mark.gpu

SENT = -7.25
WORST = {}
ENTRIES = []
_INPUTS = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


def check(family, name, got, ref, bound=0.0):
    ratio = compare(got, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f'  [{family}] {name}: {ratio:.3g}')
    assert ratio <= 1.0, f'{family} {name}: worst error / bound = {ratio:.4g}'


def call(name, *args):
    from qtmpnn import _lib
    ENTRIES.append(name)
    _lib.call(name, *args)


def p(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def filled(*shape):
    return torch.full(shape, SENT, device=dev())


def pad_rows(a, cap):
    a = np.asarray(a, np.float32)
    if cap > a.shape[0]:
        a = np.concatenate([a, np.full((cap - a.shape[0], a.shape[1]), np.nan, np.float32)])
    return _t(a)


def inputs(c):
    """The case's inputs, built once and left unchanged."""
    if c['name'] not in _INPUTS:
        _INPUTS.clear()                                   # (one case at a time: the largest is 70001 x 128)
        _INPUTS[c['name']] = M.inputs(c)
    return _INPUTS[c['name']]


def device_O(c, O):
    """(tensor that owns the storage, pointer offset in floats, ld_o): O dense (cap, h), or the column view [:, 3h:4h] of a
    (cap, 4h) matrix of NaN."""
    cap, h = c['cap'] or c['N'], c['h']
    if not c['view']:
        return pad_rows(O, cap), 0, h
    wide = np.full((cap, 4 * h), np.nan, np.float32)
    wide[:c['N'], 3 * h:] = O
    return _t(wide), 3 * h, 4 * h


def za_error(got, Za, pre, near):
    """|got - model|; at a near-kink entry the distance to the nearer of the two branches 0 and pre."""
    got = np.asarray(got, np.float64)
    return np.where(near, np.minimum(np.abs(got), np.abs(got - pre)), np.abs(got - Za))


def head_fwd(c, x):
    """qt_head_fwd on the case: (Za (cap, h), Zb (cap, hp - h)) as numpy, from the two-matrix or the single-matrix form."""
    N, h, hp, cap = c['N'], c['h'], c['hp'], c['cap'] or c['N']
    Od, off, ld = device_O(c, x['O'])
    ln, cc = _t(x['ln']), (pad_rows(x['concat'], cap) if x['concat'] is not None else None)
    nd = torch.tensor([N], dtype=torch.int32, device=dev()) if c['cap'] else None
    if c['single']:
        Z = filled(cap, hp)
        call('qt_head_fwd', p(Od, off), ld, p(ln), p(cc), cap, p(nd), h, hp, p(Z), None)
        Z = _np(Z)
        return Z[:, :h], Z[:, h:]
    Za, Zb = filled(cap, h), filled(cap, hp - h)
    call('qt_head_fwd', p(Od, off), ld, p(ln), p(cc), cap, p(nd), h, hp, p(Za), p(Zb))
    return _np(Za), _np(Zb)


def head_bwd(c, x, gZa, part=None, accumulate=0):
    """qt_head_bwd on the case with the cotangent gZa (N, h): (gO (cap, h), gconcat (cap,), slabs (nblk, 2h)) as numpy; `part`: the
    slab tensor to launch into (default: a fresh one holding the sentinel)."""
    N, h, hp, cap = c['N'], c['h'], c['hp'], c['cap'] or c['N']
    Od, off, ld = device_O(c, x['O'])
    ln = _t(x['ln'])
    nd = torch.tensor([N], dtype=torch.int32, device=dev()) if c['cap'] else None
    from qtmpnn import _lib
    nblk = _lib.value('qt_lstm_bwd_blocks', cap, h)
    assert nblk == M.bwd_blocks(cap, h)
    part = filled(nblk, 2 * h) if part is None else part
    gO, gcat = filled(cap, h), filled(cap)
    if c['single']:
        g = pad_rows(np.concatenate([gZa, x['gZb']], axis=1), cap)
        call('qt_head_bwd', p(g), None, p(Od, off), ld, p(ln), cap, p(nd), h, hp, p(gO), p(gcat), p(part), accumulate)
    else:
        ga, gb = pad_rows(gZa, cap), pad_rows(x['gZb'], cap)
        call('qt_head_bwd', p(ga), p(gb), p(Od, off), ld, p(ln), cap, p(nd), h, hp, p(gO), p(gcat), p(part), accumulate)
    return _np(gO), _np(gcat), part


# ------------------------------------------------------------------------------------------------------- 1. the C ABI
@pytest.mark.parametrize('name', [c['name'] for c in M.CASES])
def test_head_abi(name):
    """Forward, backward, slabs and their qt_colsum of one case of head_f64.CASES; capacity rows keep the sentinel bit for bit and
    their NaN inputs reach no parameter sum; wherever the kernel's own Za is 0, a cotangent placed only there gives gO == 0."""
    c = M.BY_NAME[name]
    x = inputs(c)
    N, h, hp, cap, fam = c['N'], c['h'], c['hp'], c['cap'] or c['N'], c['family']
    Zr, Zbr, pre = M.forward(x['O'], x['ln'], x['concat'], hp)
    Za, Zb = head_fwd(c, x)
    print(f'  [{fam}] {name}: {int(x["near"].sum())} of {x["near"].size} entries left out at the kink')
    check(f'fwd {fam}', name + ' Za', za_error(Za[:N], Zr, pre, x['near']), np.zeros_like(Zr), M.forward_bound(x['O'], x['ln']))
    check('data movement', name + ' Zb', Zb[:N], Zbr)
    assert (Za[N:] == SENT).all() and (Zb[N:] == SENT).all(), f'{name}: a capacity row of Za / Zb was written'
    if fam == 'const':                                    # xhat = 0 exactly: Za = relu(beta) bit for bit
        assert np.array_equal(Za[:N], np.broadcast_to(np.maximum(x['ln'][1], 0), (N, h)))
    # backward
    gOr, gcr, _ = M.backward(x['gZa'], x['gZb'], x['O'], x['ln'])
    gO, gcat, part = head_bwd(c, x, x['gZa'])
    check(f'bwd {fam}', name + ' gO', gO[:N], gOr, M.backward_bound(x['gZa'], x['O'], x['ln']))
    check('data movement', name + ' gconcat', gcat[:N], gcr)
    assert (gO[N:] == SENT).all() and (gcat[N:] == SENT).all(), f'{name}: a capacity row of gO / gconcat was written'
    slabs, mag, inh, cnt = M.part_slabs(x['gZa'], x['O'], x['ln'], part.shape[0], h // 4)
    check(f'slabs {fam}', name, part, slabs, M.slab_bound(mag, inh, cnt))          # (every slab written: none holds the sentinel)
    psum = filled(2 * h)
    call('qt_colsum', p(part), part.shape[0], 2 * h, p(psum))
    check(f'psum {fam}', name, psum, slabs.sum(axis=0), M.psum_bound(mag, inh, cnt))
    # independent of the model: the backward recomputes the forward's mask with the same bits
    dead = (Za[:N] == 0)
    g0 = np.where(dead, np.float32(1.5), np.float32(0.0)).astype(np.float32)
    gO0, _, part0 = head_bwd(c, x, g0)
    assert (gO0[:N] == 0).all() and (_np(part0) == 0).all(), f'{name}: a cotangent where Za == 0 reached gO or the sums'


# --------------------------------------------------------------------------------------------------------- 2. accumulate
@pytest.mark.parametrize('name', ['h8-N777-randn-dense-exact-cat', 'h128-N777-randn-dense-exact-cat', 'h16-N70001-randn-view-cap70400-cat',
                                  'h32-N777-offset-view-cap1100-cat'])
def test_head_accumulate(name):
    """accumulate = 1: two launches into slabs pre-filled with 3.0 give 3 + both models' slabs -- added to, not overwritten."""
    c = M.BY_NAME[name]
    x = inputs(c)
    h, cap = c['h'], c['cap'] or c['N']
    g2 = np.random.default_rng(c['seed'] + 1).standard_normal(x['gZa'].shape).astype(np.float32)
    g2[x['near']] = 0.0
    nblk = M.bwd_blocks(cap, h)
    part = torch.full((nblk, 2 * h), 3.0, device=dev())
    head_bwd(c, x, x['gZa'], part, 1)
    s1, m1, i1, cnt = M.part_slabs(x['gZa'], x['O'], x['ln'], nblk, h // 4)
    bound1 = M.slab_bound(m1, i1, cnt) + 2.0 * M.U * np.abs(3.0 + s1)
    check('slabs accumulate', name + ' first', part, 3.0 + s1, bound1)
    head_bwd(c, x, g2, part, 1)
    s2, m2, i2, _ = M.part_slabs(g2, x['O'], x['ln'], nblk, h // 4)
    check('slabs accumulate', name + ' second', part, 3.0 + s1 + s2, bound1 + M.slab_bound(m2, i2, cnt) + 2.0 * M.U * np.abs(3.0 + s1 + s2))


# ------------------------------------------------------------------------------------------------------ 3. ops.head_input
@pytest.fixture
def recording(monkeypatch):
    from qtmpnn import _lib
    names, inner = [], _lib.call

    def rec(name, *a):
        names.append(name)
        ENTRIES.append(name)
        return inner(name, *a)
    monkeypatch.setattr(_lib, 'call', rec)
    return names


def _mesh(c):
    from qtmpnn.mesh import Mesh
    mesh = Mesh()
    mesh.B, mesh.n, mesh.m, mesh.N = 1, c['cap'] or c['N'], 1, c['cap'] or c['N']
    if c['cap']:
        mesh.n_dev = torch.tensor([c['N']], dtype=torch.int32, device=dev())
    return mesh


def _leaf_O(c, O):
    Od, off, _ = device_O(c, O)
    return (Od[:, off:off + c['h']] if c['view'] else Od).detach().requires_grad_(True)


OPS_CASES = [c['name'] for c in M.CASES if c['N'] <= 777 and not c['single']] + ['h16-N70001-randn-view-cap70400-cat', 'h64-N70001-randn-view-exact-cat']


@pytest.mark.parametrize('name', OPS_CASES)
def test_head_input_autograd(recording, name):
    """ops.head_input and its backward: O dense or a column view, static capacity through mesh.n_dev, concat given or None."""
    from qtmpnn import ops
    c = M.BY_NAME[name]
    x = inputs(c)
    N, h, hp, cap, fam = c['N'], c['h'], c['hp'], c['cap'] or c['N'], c['family']
    mesh = _mesh(c)
    O, ln = _leaf_O(c, x['O']), _t(x['ln']).requires_grad_(True)
    cc = pad_rows(x['concat'], cap).requires_grad_(True) if x['concat'] is not None else None
    Za, Zb = ops.head_input(O, ln, cc, hp, mesh)
    wrt = [O, ln] + ([cc] if cc is not None else [])
    gs = torch.autograd.grad([Za, Zb], wrt, [pad_rows(x['gZa'], cap), pad_rows(x['gZb'], cap)])
    Zr, Zbr, pre = M.forward(x['O'], x['ln'], x['concat'], hp)
    check(f'fwd {fam}', name + ' ops Za', za_error(_np(Za)[:N], Zr, pre, x['near']), np.zeros_like(Zr), M.forward_bound(x['O'], x['ln']))
    check('data movement', name + ' ops Zb', Zb[:N], Zbr)
    gOr, gcr, _ = M.backward(x['gZa'], x['gZb'], x['O'], x['ln'])
    check(f'bwd {fam}', name + ' ops gO', gs[0][:N], gOr, M.backward_bound(x['gZa'], x['O'], x['ln']))
    slabs, mag, inh, cnt = M.part_slabs(x['gZa'], x['O'], x['ln'], M.bwd_blocks(cap, h), h // 4)
    check(f'psum {fam}', name + ' ops gln', gs[1].reshape(-1), slabs.sum(axis=0), M.psum_bound(mag, inh, cnt))
    if cc is not None:
        check('data movement', name + ' ops gconcat', gs[2][:N, 0], gcr)
    assert recording == ['qt_head_fwd', 'qt_head_bwd', 'qt_colsum'], recording


@pytest.mark.parametrize('name', ['h8-N777-randn-dense-exact-cat', 'h16-N777-randn-view-cap1100-nocat', 'h128-N777-offset-view-cap1100-cat'])
def test_head_input_gradacc(recording, name):
    """Two uses of one ln_o under a GradAcc (acc.slab: accumulate = 1, one qt_colsum at the first use's backward): the parameter
    gradient equals the sum of the two models."""
    from qtmpnn import ops
    c = M.BY_NAME[name]
    x = inputs(c)
    N, h, hp, cap = c['N'], c['h'], c['hp'], c['cap'] or c['N']
    mesh, acc = _mesh(c), ops.GradAcc()
    rng = np.random.default_rng(c['seed'] + 2)
    O2 = M.draw_rows(rng, c['family'], N, h)
    g2 = rng.standard_normal((N, h)).astype(np.float32)
    g2[M.near_kink(O2, x['ln'])] = 0.0
    ln = _t(x['ln']).requires_grad_(True)
    cc = pad_rows(x['concat'], cap) if x['concat'] is not None else None
    Za1, Zb1 = ops.head_input(_leaf_O(c, x['O']), ln, cc, hp, mesh, acc)
    O2d = _leaf_O(c, O2) * 1.0                             # the second use hangs on the first, as the recurrent state chains them
    O2d[:1, :1] = O2d[:1, :1] + 0.0 * Za1[:1, :1]          # (through a valid row only: capacity rows of a gradient hold anything)
    Za2, Zb2 = ops.head_input(O2d, ln, cc, hp, mesh, acc)
    (gln,) = torch.autograd.grad([Za1, Za2], [ln], [pad_rows(x['gZa'], cap), pad_rows(g2, cap)])
    nblk = M.bwd_blocks(cap, h)
    s1, m1, i1, cnt = M.part_slabs(x['gZa'], x['O'], x['ln'], nblk, h // 4)
    s2, m2, i2, _ = M.part_slabs(g2, O2, x['ln'], nblk, h // 4)
    # per slab both launches' bounds and the second add's rounding; then the column sum of the summed majorants
    bound = (M.slab_bound(m1, i1, cnt) + M.slab_bound(m2, i2, cnt) + 2.0 * M.U * np.abs(s1 + s2)).sum(axis=0) \
        + 2.0 * M.colsum_count(nblk) * M.U * (m1 + m2).sum(axis=0)
    check('psum GradAcc', name, gln.reshape(-1), (s1 + s2).sum(axis=0), bound)
    assert recording == ['qt_head_fwd', 'qt_head_fwd', 'qt_head_bwd', 'qt_head_bwd', 'qt_colsum'], recording


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per family of this session (the figures of profiles/head_pack_f64.txt) and the entry points
    that ran; when the whole file ran, every entry point of the family was called."""
    for fam in sorted(WORST):
        print(f'  worst [{fam}]: {WORST[fam]:.3g}')
    print('  entry points:', ', '.join(f'{n} x{ENTRIES.count(n)}' for n in sorted(set(ENTRIES))))
    assert all(v <= 1.0 for v in WORST.values())
    assert WORST.get('data movement', 0.0) == 0.0
    want = {f'{k} {f}' for k in ('fwd', 'bwd', 'slabs', 'psum') for f in M.FAMILIES} | {'data movement', 'slabs accumulate', 'psum GradAcc'}
    if not want <= set(WORST):
        return                                         # (a selection of the file ran: nothing to say about what it covers)
    assert {'qt_head_fwd', 'qt_head_bwd', 'qt_colsum'} <= set(ENTRIES)
