"""The dense half of ops.cheb_poly -- qt_dense2 with its six kernels (k_gemm_skinny<256>, k_gemm_row16, k_gemm_skinny<64>,
k_gemm_fwd<2|3|4>), qt_head_dgrad, qt_act_bwd, qt_wgrad, qt_wgrad_group and qt_colsum (csrc/gemm.hip, csrc/lstm.hip), and the
Python side that chains them (ops._cheb_backward, GradAcc, ops._wgrad_group) -- against the float64 model tests/gemm_f64.py.

Every comparison is kernel against model, never kernel against kernel.  Exact cases draw every operand from {-2, -1, 1, 2} (dropout
factors from {0, 2}): every partial sum is an integer below 2^24, the bound is 0 and got == model entry for entry at any N, so one
dropped, doubled or misplaced row or quad fails with certainty.  Real-valued cases draw sign * (0.5 + U[0, 1)) and use the bounds
derived beside the model (twice a count of float32 roundings times 2^-24 times the majorant).  Outputs and slabs are pre-filled
with the sentinel -7.25; capacity rows of inputs are NaN.  Every case prints its worst error / bound before it asserts
(pytest -s; a recorded run: profiles/gemm_f64.txt).  tests/test_gemm_f64_host.py names, per mutation, the case here that sees it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cheb_f64 as CM
import gemm_f64 as M
from helpers import dev
from test_gpu_cheb_f64 import compare, get, pad

pytestmark = pytest.mark.gpu

SENT = -7.25
WORST = {}
KERNELS = set()          # kernels qt_dense2 was asked for, by shape (gemm_f64.dispatch)
ENTRIES = []             # entry points called through _lib.call while `recording`


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


def n_dev(nv):
    return None if nv is None else torch.tensor([nv], dtype=torch.int32, device=dev())


def p(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


class Operand:
    """A model operand (K, nv, Ca + Cab) on the device in the C ABI's layout (gemm_f64.pack_operand), and its argument tuple
    (a0, lda0, a_rest, a0b, lda0b, a_restb)."""

    def __init__(self, planes, Ca, cap=None, lda=(0, 0), sm=False, rng=None):
        nv = planes.shape[1]
        junk = None if rng is None else M.ints(rng, nv, 96)
        self.parts = M.pack_operand(planes, Ca, cap, lda, sm=sm, junk=junk)
        self.dev = [(_t(q['wide']), q['off'], None if q['rest'] is None else _t(q['rest'])) for q in self.parts]
        self.args = []
        for wide, off, rest in self.dev:
            self.args += [p(wide, off), wide.shape[1], p(rest)]
        if len(self.dev) == 1:
            self.args += [None, 0, None]


def filled(*shape):
    return torch.full(shape, SENT, device=dev())


def dense2(planes, S, W, Kb, Cb, Cbb, nv, cap=None, Ca=None, lda=(0, 0), in_sm=False, out_sm=False, use_wt=False, act=M.ACT_NONE,
           res=None, res_view=None, drop=None, W2=None, rng=None):
    """One qt_dense2 launch on the model's arrays; returns (Y (Kb, cap, Cb + Cbb) as the model lays it out, U (cap, 4) or None)."""
    Ka, _, C = planes.shape
    Ca = C if Ca is None else Ca
    cap = nv if cap is None else cap
    op = Operand(planes, Ca, cap, lda, in_sm, rng)
    Ks = 0 if S is None else S.shape[1]
    Sd = None if S is None else pad_rows(S, cap)
    Wd = _t(W)
    WTd = _t(W.T) if use_wt else None
    NB = Kb * (Cb + Cbb)
    out, outb = filled(Kb, cap, Cb), filled(Kb, cap, Cbb) if Cbb else None
    Ud = filled(cap, 4) if W2 is not None else None
    resd, rs = None, 0
    if res is not None:
        resd = pad_rows(res, cap)
        rs = resd.shape[1]
        if res_view is not None:                       # one column of a wider matrix
            resd = resd[:, res_view:res_view + 1]
    dropd = None if drop is None else pad_rows(drop[:, None], cap)
    KERNELS.add(M.dispatch(Ka * C + Ks, NB, Kb, Cbb, act, not use_wt))
    nd, W2d = n_dev(None if cap == nv else nv), (_t(W2) if W2 is not None else None)       # (every operand stays referenced until the results are read)
    call('qt_dense2', *op.args, Ka, Ca, C - Ca, None if use_wt else p(Wd), p(WTd), p(Sd), Ks,
         p(Wd, Ka * C * NB) if (Ks and not use_wt) else None, Kb, Cb, Cbb, cap, p(nd), act, p(resd), rs,
         p(dropd), p(out), p(outb), int(in_sm) | 2 * int(out_sm), p(W2d), p(Ud))
    Y = M.unpack_planes(_np(out), None if outb is None else _np(outb), out_sm)
    return Y, None if Ud is None else _np(Ud)


def pad_rows(a, cap):
    """Device copy of the (nv, w) array a with NaN rows up to cap."""
    a = np.asarray(a, np.float32)
    if cap > a.shape[0]:
        a = np.concatenate([a, np.full((cap - a.shape[0], a.shape[1]), np.nan, np.float32)])
    return _t(a)


def exact_forward(name, Kred, nb, N, cap=None, seed=0, **kw):
    """An exact qt_dense2 case: operands of {-2, -1, 1, 2}, got == model entry for entry, capacity rows untouched."""
    Ka, Ca, Cab, Ks = M.split_kred(Kred) if isinstance(Kred, int) else Kred
    Kb, Cb, Cbb = nb
    rng = np.random.default_rng(seed + 7 * N)
    planes = M.ints(rng, Ka, N, Ca + Cab)
    S = M.ints(rng, N, Ks) if Ks else None
    W = M.ints(rng, Ka * (Ca + Cab) + Ks, Kb * (Cb + Cbb))
    mk = {k: kw.pop(k) for k in ('act', 'res', 'drop', 'W2') if k in kw}
    Yr, Ur, _ = M.forward(planes, S, W, Kb, Cb, Cbb, **mk)
    Y, Ug = dense2(planes, S, W, Kb, Cb, Cbb, N, cap, Ca=Ca, rng=rng, **mk, **kw)
    check('dense2 exact', name, Y[:, :N], Yr)
    assert (Y[:, N:] == SENT).all(), f'{name}: a capacity row was written'
    if Ur is not None:
        check('dense2 exact', name + ' U', Ug[:N], Ur)
        assert (Ug[N:] == SENT).all()


# ------------------------------------------------------------------------------------------------------- 1. forward dispatch
@pytest.mark.parametrize('Kred,NB,nb,kernel', M.DISPATCH)
def test_forward_dispatch_exact(Kred, NB, nb, kernel):
    """Every kernel of qt_dense2 by shape, at the row counts around its row tile; with W, and where NB > 16 also with WT."""
    nb = nb or M.split_nb(NB)
    assert M.dispatch(Kred, NB, nb[0], nb[2]) == kernel
    for N in M.ROWS.get(kernel, M.ROWS_MFMA):
        exact_forward(f'({Kred}, {NB}) {nb} N={N} W', Kred, nb, N, seed=Kred + NB)
        if NB > 16:
            exact_forward(f'({Kred}, {NB}) {nb} N={N} WT', Kred, nb, N, seed=Kred + NB, use_wt=True)


# ---------------------------------------------------------------------------------------------------------- 2. operand forms
@pytest.mark.parametrize('Ks', [0, 4, 8])
@pytest.mark.parametrize('shape', [(5, 64), (3, 16)])
def test_operand_forms_exact(shape, Ks):
    """One part and two parts, plane 0 dense and as a column view (lda 24 / 36), planes 1.. row-major and slice-major.
    (Swapping lda0 / lda0b in build_quad_table fails the two-part column-view cases; so does reading part b with part a's stride.)"""
    Ka, NB = shape
    nb = M.split_nb(NB)
    for N in (129, 257):
        for Ca, Cab in ((4, 16), (20, 0)):
            for lda in ((0, 0), (24, 36)):
                for sm in (False, True):
                    lda_ = lda if Cab else (lda[1], 0)
                    exact_forward(f'Ka={Ka} ({Ca}, {Cab}) Ks={Ks} NB={NB} N={N} lda={lda_} sm={int(sm)}', (Ka, Ca, Cab, Ks), nb, N,
                                  seed=Ks, lda=lda_, in_sm=sm, use_wt=NB > 16 and sm)


# ----------------------------------------------------------------------------------------------------------- 3. output forms
@pytest.mark.parametrize('widths', [(16, 0), (4, 16)])
@pytest.mark.parametrize('Kb', [1, 3, 5])
def test_output_forms_exact(Kb, widths):
    """Output planes row-major and slice-major (plane 0 stays row-major), one and two column parts, and n_dev: 0, 1 and 130 valid
    rows of 384 (the last 128-row block wholly invalid).  (Dropping the `sm && pl > 0` test in plane_piece fails sm=1 here.)"""
    Cb, Cbb = widths
    for out_sm in (False, True):
        for N, cap in ((129, None), (257, None), (0, 384), (1, 384), (130, 384)):
            exact_forward(f'Kb={Kb} {widths} out_sm={int(out_sm)} N={N} cap={cap}', 64, (Kb, Cb, Cbb), N, cap, seed=Kb,
                          out_sm=out_sm, in_sm=out_sm)


# -------------------------------------------------------------------------------------------------------------- 4. epilogues
@pytest.mark.parametrize('Kred,NB', [(20, 4), (64, 16), (260, 16), (64, 8), (104, 64), (104, 96), (68, 128)])
def test_relu_and_dropout_exact(Kred, NB):
    for N in (65, 257):
        rng = np.random.default_rng(N)
        drop = rng.choice([0.0, 2.0], size=N).astype(np.float32)
        exact_forward(f'relu ({Kred}, {NB}) N={N}', Kred, (1, NB, 0), N, act=M.ACT_RELU)
        exact_forward(f'relu + drop ({Kred}, {NB}) N={N}', Kred, (1, NB, 0), N, act=M.ACT_RELU, drop=drop)
        exact_forward(f'relu + drop ({Kred}, {NB}) N={N} of 320', Kred, (1, NB, 0), N, 320,
                      act=M.ACT_RELU, drop=drop)


@pytest.mark.parametrize('Kred', [64, 256, 260])
@pytest.mark.parametrize('act', [M.ACT_NONE, M.ACT_RELU])
def test_post_product_exact(Kred, act):
    """post_W on k_gemm_row16 (Kred <= 256) and on k_gemm_skinny<64> (Kred = 260): U = [act(Y) | 1 0 0 0] W2."""
    assert M.dispatch(Kred, 16) == ('k_gemm_row16' if Kred <= 256 else 'k_gemm_skinny<64>')
    for N, cap in ((1, None), (63, None), (65, None), (130, None), (70, 192)):
        W2 = M.ints(np.random.default_rng(N), 20, 4)
        exact_forward(f'post Kred={Kred} act={act} N={N} cap={cap}', Kred, (1, 16, 0), N, cap, act=act, W2=W2)


@pytest.mark.parametrize('NB,stride', [(16, 16), (16, 20), (8, 8), (12, 20)])
def test_relu_bwd_epilogue_exact(NB, stride):
    """QT_ACT_RELU_BWD: the product masked by res = the forward output Y (N, stride) > 0; Kred = 4 (the head's gU @ Wb2)."""
    for N, cap in ((1, None), (64, None), (65, None), (200, None), (70, 192)):
        rng = np.random.default_rng(N + stride)
        Yf = M.ints(rng, N, stride)
        exact_forward(f'relu_bwd NB={NB} stride={stride} N={N} cap={cap}', 4, (1, NB, 0), N, cap, act=M.ACT_RELU_BWD, res=Yf)


@pytest.mark.parametrize('Kred,NB,N', M.REAL_TANH + M.REAL_TANH_WIDE)
@pytest.mark.parametrize('view', [None, 0, 1])
def test_tanh_res_real(Kred, NB, N, view):
    """QT_ACT_TANH_RES, real-valued: res as a one-column view of an (N, 4) matrix (column `view`) and of full width (N, NB), with a dropout
    mask of {0, 1.25}; the default fp32 path within gemm_f64.forward_bound.  A bf16 operand is >= 10 bounds away (host test)."""
    Ka, Ca, Cab, Ks = M.split_kred(Kred)
    rng = np.random.default_rng(Kred + NB + N)
    planes, S = M.draw(rng, Ka, N, Ca + Cab), M.draw(rng, N, Ks)
    W = M.draw(rng, Kred, NB) * np.float32(4.0 / Kred)
    res = M.draw(rng, N, 4 if view is not None else NB)
    drop = ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
    Yr, _, maj = M.forward(planes, S, W, 1, NB, 0, M.ACT_TANH_RES, res if view is None else res[:, view:], drop)
    for cap in (None, N + 130):
        Y, _ = dense2(planes, S, W, 1, NB, 0, N, cap, Ca=Ca, act=M.ACT_TANH_RES, res=res, res_view=view, drop=drop, in_sm=Ka > 1)
        check('dense2 tanh', f'({Kred}, {NB}) N={N} cap={cap} view={view}', Y[0, :N], Yr[0], M.forward_bound(maj, M.ACT_TANH_RES, Yr[0]))
        assert (Y[:, N:] == SENT).all()


@pytest.mark.parametrize('Kred,NB', M.REAL_FORWARD)
def test_forward_real(Kred, NB):
    """The plain product, real-valued, on row16, skinny<64> and the three MFMA tiles: Kred fused multiply-adds per entry."""
    Ka, Ca, Cab, Ks = M.split_kred(Kred)
    Kb, Cb, Cbb = M.split_nb(NB)
    N = 129
    rng = np.random.default_rng(Kred + NB)
    planes, S, W = M.draw(rng, Ka, N, Ca + Cab), M.draw(rng, N, Ks), M.draw(rng, Kred, NB)
    Yr, _, maj = M.forward(planes, S, W, Kb, Cb, Cbb)
    bound = M.product_bound(maj['mag'], Kred).reshape(N, Kb, Cb + Cbb).transpose(1, 0, 2)
    for wt in ((False, True) if NB > 16 else (False,)):
        Y, _ = dense2(planes, S, W, Kb, Cb, Cbb, N, Ca=Ca, use_wt=wt)
        check('dense2 real', f'({Kred}, {NB}) WT={int(wt)}', Y, Yr, bound)


# ---------------------------------------------------------------------------------------------------------- 5. qt_head_dgrad
def head_dgrad(gU, W2, Y, W1, K, Cb, Cbb, nv, cap, out_sm):
    Wb2, Wb1 = _t(W2[:16].T), _t(W1[:K * (Cb + Cbb)])
    G, out, outb = filled(cap, 16), filled(K, cap, Cb), filled(K, cap, Cbb) if Cbb else None
    gUd, Yd, nd = pad_rows(gU, cap), pad_rows(Y, cap), n_dev(None if cap == nv else nv)
    call('qt_head_dgrad', p(gUd), p(Wb2), p(Yd), p(Wb1), K, Cb, Cbb, cap, p(nd), p(G), p(out), p(outb), int(out_sm))
    return _np(G), M.unpack_planes(_np(out), None if outb is None else _np(outb), out_sm)


@pytest.mark.parametrize('widths', [(4, 16), (20, 0)])
@pytest.mark.parametrize('real', [False, True])
def test_head_dgrad(widths, real):
    """G = relu'(Y) (.) (gU W2[:16]^T) and both plane sets = G W1^T, K = 3; exact at every N, real-valued at gemm_f64.REAL_HEAD's."""
    Cb, Cbb = widths
    K, C = 3, Cb + Cbb
    rows = [(N, None) for N in (1, 63, 64, 65, 200)] + [(70, 192)]
    if real:
        rows = [(N, None) for w, N in M.REAL_HEAD if w == widths] + [(70, 192)]
    gen = M.draw if real else M.ints
    for N, cap in rows:
        rng = np.random.default_rng(N + Cb)
        gU, W2, Y, W1 = gen(rng, N, 4), gen(rng, 20, 4), gen(rng, N, 16), gen(rng, K * C + 4, 16)
        Gr, Pr, parts = M.head_bwd(gU, W2, Y, W1, K, C)
        eG, eP = M.head_bounds(parts) if real else (0.0, 0.0)
        for out_sm in (False, True):
            G, P = head_dgrad(gU, W2, Y, W1, K, Cb, Cbb, N, cap or N, out_sm)
            fam = 'head_dgrad real' if real else 'head_dgrad exact'
            check(fam, f'{widths} N={N} cap={cap} sm={int(out_sm)} G', G[:N], Gr, eG)
            check(fam, f'{widths} N={N} cap={cap} sm={int(out_sm)} planes', P[:, :N], Pr, eP)
            assert (G[N:] == SENT).all() and (P[:, N:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------- 6. qt_act_bwd
def act_bwd(gY, Y, act, res, drop, gY2, nv, cap, want_gres):
    Co = Y.shape[1]
    G = filled(cap, Co)
    gres = filled(cap, res.shape[1]) if want_gres else None
    gYd, Yd, resd = pad_rows(gY, cap), pad_rows(Y, cap), (None if res is None else pad_rows(res, cap))
    dropd, g2d, nd = (None if drop is None else pad_rows(drop[:, None], cap)), (None if gY2 is None else pad_rows(gY2, cap)), n_dev(None if cap == nv else nv)
    call('qt_act_bwd', p(gYd), p(Yd), p(resd), 0 if res is None else res.shape[1], p(dropd), act, cap, p(nd), Co, p(G), p(gres), p(g2d))
    return _np(G), None if gres is None else _np(gres)


@pytest.mark.parametrize('Co', [4, 16])
def test_act_bwd_relu_exact(Co):
    for N, cap in ((1, None), (65, None), (257, None), (70, 192)):
        rng = np.random.default_rng(N + Co)
        gY, gY2, Y = M.ints(rng, N, Co), M.ints(rng, N, Co), M.ints(rng, N, Co)
        drop = rng.choice([0.0, 2.0], size=N).astype(np.float32)
        for d, g2 in ((None, None), (drop, None), (drop, gY2)):
            G, _ = act_bwd(gY, Y, M.ACT_RELU, None, d, g2, N, cap or N, False)
            check('act_bwd exact', f'relu Co={Co} N={N} cap={cap} drop={d is not None} gY2={g2 is not None}', G[:N],
                  M.act_bwd(gY, Y, M.ACT_RELU, None, d, g2)[0])
            assert (G[N:] == SENT).all()


@pytest.mark.parametrize('Co,rs,N', M.REAL_ACT)
def test_act_bwd_tanh_real(Co, rs, N):
    """Tanh + residual (narrower than Co), with gres and with the second gradient gY2."""
    rng = np.random.default_rng(Co + N)
    res, drop = M.draw(rng, N, rs), ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
    Y = (np.tanh(M.draw(rng, N, Co)) + res[:, :1]).astype(np.float32)
    gY, gY2 = M.draw(rng, N, Co), M.draw(rng, N, Co)
    for cap in (N, N + 130):
        for g2 in (None, gY2):
            Gr, gres_r, parts = M.act_bwd(gY, Y, M.ACT_TANH_RES, res, drop, g2)
            G, gres = act_bwd(gY, Y, M.ACT_TANH_RES, res, drop, g2, N, cap, True)
            check('act_bwd tanh', f'Co={Co} rs={rs} N={N} cap={cap} gY2={g2 is not None}', G[:N], Gr, M.act_bwd_bound(parts, Gr))
            # gres column 0 = gY + gY2 (one rounding), the rest 0
            check('act_bwd tanh', f'Co={Co} rs={rs} N={N} cap={cap} gres', gres[:N], gres_r, 2.0 * M.U * np.abs(gres_r) * (g2 is not None))
            assert (G[N:] == SENT).all() and (gres[N:] == SENT).all()


# ------------------------------------------------------------------------------------------------- 7. qt_wgrad + qt_colsum
def colsum(part, nblk, length):
    out = filled(length)
    call('qt_colsum', p(part), nblk, length, p(out))
    return _np(out)


def wgrad(planes, S, G, nv, cap, Ca, sm=False, lda=(0, 0), prefill=None, rng=None):
    """qt_wgrad on the model's arrays: (slabs (nblk, M, Co), their qt_colsum)."""
    from qtmpnn import _lib
    Ka, _, C = planes.shape
    Ks = 0 if S is None else S.shape[1]
    Mw, Co = Ka * C + Ks, G.shape[1]
    op = Operand(planes, Ca, cap, lda, sm, rng)
    nblk = _lib.value('qt_wgrad_blocks', cap)
    assert nblk == -(-cap // M.WGRAD_ROWS)
    part = filled(nblk, Mw, Co) if prefill is None else _t(prefill)
    Sd, Gd, nd = (None if S is None else pad_rows(S, cap)), pad_rows(G, cap), n_dev(None if cap == nv else nv)
    call('qt_wgrad', *op.args, Ka, Ca, C - Ca, p(Sd), Ks, p(Gd), Co, cap, p(nd), int(prefill is not None), p(part), int(sm))
    return _np(part), colsum(part, nblk, Mw * Co).reshape(Mw, Co)


def exact_wgrad(name, Mw, Co, N, cap=None, **kw):
    Ka, Ca, Cab, Ks = M.split_kred(Mw)
    rng = np.random.default_rng(Mw + Co + N)
    planes, G = M.ints(rng, Ka, N, Ca + Cab), M.ints(rng, N, Co)
    S = M.ints(rng, N, Ks) if Ks else None
    cap = cap or N
    ref = M.wgrad_blocks(planes, S, G, N, cap)
    pre = None
    if kw.pop('accumulate', False):
        pre = rng.integers(-3, 4, size=ref.shape).astype(np.float32)
        ref = ref + pre
    part, total = wgrad(planes, S, G, N, cap, Ca, prefill=pre, rng=rng, **kw)
    check('wgrad exact', name + ' slabs', part, ref)          # a block beyond the valid rows: exactly 0, not the sentinel
    check('wgrad exact', name + ' colsum', total, ref.sum(axis=0))


@pytest.mark.parametrize('Mw,Co', M.wgrad_pairs())
def test_wgrad_exact(Mw, Co):
    """Feature tiles FW = 1 / 2 / 4, column tiles CT = 1 / 2 with a second blockIdx.y tile at Co = 128, the 2 x 32-row pipeline
    and its zero-loading tail, z-blocks of 512 rows.  (`rend` one short in k_gemm_wgrad fails every N here.)"""
    for N in M.WGRAD_N:
        exact_wgrad(f'M={Mw} Co={Co} N={N}', Mw, Co, N)


@pytest.mark.parametrize('Mw,Co', [(20, 16), (64, 36), (104, 128), (512, 16)])
def test_wgrad_forms_exact(Mw, Co):
    """n_dev valid {0, 1, 513} of 1536 (slabs of blocks beyond the valid rows exactly 0), accumulate = 1 on pre-filled slabs,
    slice-major planes, two-part operands with strided plane 0."""
    for nv in (0, 1, 513):
        exact_wgrad(f'M={Mw} Co={Co} n_dev {nv} of 1536', Mw, Co, nv, 1536)
        exact_wgrad(f'M={Mw} Co={Co} n_dev {nv} of 1536 accumulate', Mw, Co, nv, 1536, accumulate=True)
    for N in (65, 513):
        exact_wgrad(f'M={Mw} Co={Co} N={N} accumulate', Mw, Co, N, accumulate=True)
        exact_wgrad(f'M={Mw} Co={Co} N={N} sm', Mw, Co, N, sm=True)
        _, Ca, Cab, _ = M.split_kred(Mw)
        lda = (Ca + 20, Cab + 20 if Cab else 0)               # (4, 16): 24 and 36
        exact_wgrad(f'M={Mw} Co={Co} N={N} strided', Mw, Co, N, lda=lda)
        exact_wgrad(f'M={Mw} Co={Co} N={N} strided sm 600', Mw, Co, N, 600, sm=True, lda=lda)


@pytest.mark.parametrize('Mw,Co,N', M.REAL_WGRAD)
def test_wgrad_real(Mw, Co, N):
    Ka, Ca, Cab, Ks = M.split_kred(Mw)
    rng = np.random.default_rng(Mw + Co + N)
    planes, S, G = M.draw(rng, Ka, N, Ca + Cab), M.draw(rng, N, Ks), M.draw(rng, N, Co)
    ref, mag = M.wgrad(planes, S, G)
    _, total = wgrad(planes, S, G, N, N, Ca, sm=Ka > 1)
    check('wgrad real', f'M={Mw} Co={Co} N={N} ({M.wgrad_count(N, Mw)} roundings)', total, ref, M.wgrad_bound(mag, N, Mw))


# ----------------------------------------------------------------------------------------------------------- 8. qt_wgrad_group
@pytest.mark.parametrize('sm', [False, True])
@pytest.mark.parametrize('Ns', [(70,), (70, 0, 513), tuple(40 + 37 * t for t in range(16))])
def test_wgrad_group_exact(Ns, sm):
    """1, 3 (one use of no rows: skipped) and 16 uses per launch, every other use with a capacity and n_dev; the slabs and their
    qt_colsum against the sum of the model's per-use gradients."""
    from qtmpnn import _lib
    Ka, Ca, Cab, Ks, Co = 3, 4, 16, 4, 16
    Mw = Ka * (Ca + Cab) + Ks
    rng = np.random.default_rng(len(Ns))
    keep, slabs, caps = [], [], []
    cols = {k: [] for k in ('a0', 'lda0', 'ar', 'a0b', 'lda0b', 'arb', 'S', 'G', 'nd')}
    for t, nv in enumerate(Ns):
        cap = nv + 100 if (t % 2 and nv) else nv
        caps.append(cap)
        planes, S, G = M.ints(rng, Ka, nv, Ca + Cab), M.ints(rng, nv, Ks), M.ints(rng, nv, Co)
        if cap:
            slabs.append(M.wgrad_blocks(planes, S, G, nv, cap))
        op = Operand(planes, Ca, max(cap, 1), (24, 36) if t % 3 == 1 else (0, 0), sm, rng)
        Sd, Gd, nd = pad_rows(S, max(cap, 1)), pad_rows(G, max(cap, 1)), n_dev(None if cap == nv else nv)
        keep += [op, Sd, Gd, nd]
        for k, v in zip(('a0', 'lda0', 'ar', 'a0b', 'lda0b', 'arb'), op.args):
            cols[k].append(v)
        cols['S'].append(p(Sd)), cols['G'].append(p(Gd)), cols['nd'].append(p(nd))
    n = len(Ns)
    vp, ip = (lambda k: (ctypes.c_void_p * n)(*cols[k])), (lambda v: (ctypes.c_int * n)(*v))
    Nc = ip(caps)
    nblk = _lib.value('qt_wgrad_group_blocks', n, Nc)
    ref = np.concatenate(slabs)
    assert nblk == ref.shape[0]
    part = filled(nblk, Mw, Co)
    call('qt_wgrad_group', n, vp('a0'), ip(cols['lda0']), vp('ar'), vp('a0b'), ip(cols['lda0b']), vp('arb'), vp('S'), vp('G'), Nc, vp('nd'),
         Ka, Ca, Cab, Ks, Co, p(part), int(sm))
    check('wgrad_group exact', f'{n} uses sm={int(sm)} slabs', _np(part), ref)
    check('wgrad_group exact', f'{n} uses sm={int(sm)} colsum', colsum(part, nblk, Mw * Co).reshape(Mw, Co), ref.sum(axis=0))


# --------------------------------------------------------------------------------------------------------------- 9. qt_colsum
@pytest.mark.parametrize('length', [1, 31, 32, 33, 1000])
def test_colsum_exact(length):
    """Four slabs in flight per thread in steps of 128 / 32; nblk = 0 gives zeros."""
    for nblk in (0, 1, 31, 32, 33, 127, 128, 129, 200):
        part = np.random.default_rng(nblk + length).integers(-2, 3, size=(max(nblk, 1), length)).astype(np.float32)
        check('colsum exact', f'nblk={nblk} len={length}', colsum(_t(part), nblk, length), part[:nblk].sum(axis=0))


# ------------------------------------------------------------------------------------------------ 10. ops.cheb_poly end to end
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


def _model_poly(L, Z, W, K, Ks, act, res, drop, W2):
    """The model of ops.cheb_poly on the model's L^: (Y, U, planes T, S, majorants incl. the inherited plane errors through |W|)."""
    T, A = CM.planes(L, Z, K)
    S = Sm = None
    if Ks:
        ksp = -(-Ks // 4) * 4
        S, Sm = np.zeros((L.N, ksp)), np.zeros((L.N, ksp))
        S[:, :Ks], Sm[:, :Ks] = CM.ones(L, Ks)
    Y, Um, maj = M.forward(T, S, W, 1, W.shape[1], 0, act, res, drop, W2)
    # what the planes and the bias columns carry in: plane k is k hops (cheb_f64.plane_bound), through |W|'s rows of that plane
    eA = [CM.plane_bound(L, k, A[k]) for k in range(K)]
    if Ks:
        eS = np.zeros_like(Sm)
        for k in range(Ks):
            eS[:, k] = CM.plane_bound(L, k, Sm[:, k])
        eA.append(eS)
    maj['eA'] = np.concatenate(eA, axis=1)
    maj['inherit'] = maj['eA'] @ np.abs(np.asarray(W, np.float64))
    return Y[0], Um, T, S, maj


def _y_bound(maj, act, Y):
    d = maj['drop'][:, None]
    return M.forward_bound(maj, act, Y) + d * maj['inherit']


E2E = [  # tag, K, widths, Ks, act, drop, post, live, Y of a post + ReLU case has a cotangent of its own
    ('S', 1, (16,), 0, M.ACT_NONE, False, False, None, False),
    ('S', 2, (4, 16), 1, M.ACT_RELU, False, False, None, False),
    ('D', 3, (4, 16), 3, M.ACT_RELU, False, True, None, False),            # the head: qt_head_dgrad
    ('D', 3, (4, 16), 1, M.ACT_NONE, False, True, None, False),            # post without ReLU: two launches backwards
    ('D', 5, (16,), 1, M.ACT_TANH_RES, True, False, None, False),
    ('D', 3, (4, 16), 1, M.ACT_NONE, False, False, (False, True), False),  # Za is data, Zb wants a gradient
    ('T', 3, (4, 16), 1, M.ACT_RELU, True, False, None, False),            # static: n_dev
    ('T', 5, (4, 16), 3, M.ACT_NONE, False, True, None, False),
    ('Z', 2, (16,), 1, M.ACT_TANH_RES, False, False, None, False),
    ('Z', 3, (4, 16), 0, M.ACT_RELU, False, True, None, False),
    ('D', 3, (4, 16), 1, M.ACT_RELU, False, True, (False, True), False),   # the head with a live subset: gU @ Wb2 with QT_ACT_RELU_BWD
    ('D', 3, (4, 16), 1, M.ACT_RELU, False, True, None, True),             # the head with a gradient at Y too: G + gY, then qt_act_bwd
    ('T', 3, (4, 16), 1, M.ACT_RELU, True, True, None, False),             # the head under a dropout mask: no fused launch knows it
]


@pytest.mark.parametrize('tag,K,widths,Ks,act,with_drop,post,live,y_cot', E2E)
def test_cheb_poly_end_to_end(recording, tag, K, widths, Ks, act, with_drop, post, live, y_cot):
    """Y, U and the gradients of ops.cheb_poly under random cotangents against cheb_f64.planes / clenshaw composed with gemm_f64.
    Bounds: the product's own roundings + the planes' errors through |W| (cheb_f64.plane_bound); an entry of a ReLU whose
    pre-activation lies inside its own bound may fall either way and is allowed its whole gradient."""
    from qtmpnn import ops
    mesh, L = get(tag)
    nv, C, Co = L.N, sum(widths), 16
    rng = np.random.default_rng(K + 10 * Ks + C)
    Z = M.draw(rng, nv, C)
    ksp = -(-Ks // 4) * 4
    W = M.draw(rng, K * C + ksp, Co) * np.float32(2.0 / (K * C))
    W[K * C + Ks:] = 0
    res = M.draw(rng, nv, 4) if act == M.ACT_TANH_RES else None
    drop = ((rng.random(nv) > 0.2) * 1.25).astype(np.float32) if with_drop else None
    W2 = M.draw(rng, 20, 4) if post else None
    if post:
        W2[17:] = 0
    gY, gU = M.draw(rng, nv, Co), M.draw(rng, nv, 4)
    live = live or (True,) * len(widths)
    # device
    Zd, o = [], 0
    for w, f in zip(widths, live):
        Zd.append(pad(mesh, Z[:, o:o + w]).requires_grad_(f))
        o += w
    Wd, W2d = _t(W).requires_grad_(True), (_t(W2).requires_grad_(True) if post else None)
    resd = pad(mesh, res).requires_grad_(True) if res is not None else None
    dropd = pad(mesh, drop) if drop is not None else None
    out = ops.cheb_poly(Zd[0] if len(Zd) == 1 else tuple(Zd), Wd, mesh, K, Ks, act, res=resd, drop=dropd,
                        post=(W2d, None) if post else None)
    Yd, Ud = out if post else (out, None)
    wrt = [z for z, f in zip(Zd, live) if f] + [Wd] + ([resd] if resd is not None else []) + ([W2d] if post else [])
    outs, cots = [Yd] + ([Ud] if post else []), [pad(mesh, gY, 0.0)] + ([pad(mesh, gU, 0.0)] if post else [])
    if post and act == M.ACT_RELU and not y_cot:
        outs, cots = [Ud], cots[1:]            # the head as the model runs it: Y has no other consumer (gY is None)
        gY = np.zeros_like(gY)
    grads = list(torch.autograd.grad(outs, wrt, cots))
    # model
    Yr, Ur, T, S, maj = _model_poly(L, Z, W, K, Ks, act, res, drop, W2)
    yb = _y_bound(maj, act, Yr)
    name = f'{tag} K={K} {widths} Ks={Ks} act={act} drop={int(with_drop)} post={int(post)} live={live} y_cot={int(y_cot)}'
    check('cheb_poly Y', name, Yd[:nv], Yr, yb)
    d = maj['drop'][:, None]
    g = gY.astype(np.float64)
    eg = np.zeros_like(g)
    if post:
        check('cheb_poly U', name, Ud[:nv], Ur, M.post_bound(maj, yb))
        Wb2 = np.asarray(W2, np.float64)[:16].T
        g = g + gU.astype(np.float64) @ Wb2
        mgu = np.abs(gU.astype(np.float64)) @ np.abs(Wb2)
        eg = M.product_bound(mgu, 4) + 2.0 * M.U * (np.abs(gY) + mgu)          # four fused multiply-adds, then the add of gY
        one = np.zeros((nv, 4))
        one[:, 0] = 1.0
        Y1, eY1 = np.concatenate([Yr, one], axis=1), np.concatenate([yb, 0.0 * one], axis=1)
    if act == M.ACT_RELU:
        G = np.where(Yr > 0, g * d, 0.0)
        # the device masks by its own Y = max(d acc, 0), |d acc - d pre| <= yb: only where the model's d pre lies inside that bound
        # may the entry fall either way
        near = np.abs(d * maj['pre']) <= yb
        print(f'  [cheb_poly] {name}: {int(near.sum())} of {near.size} pre-activations inside their bound')
        eG = np.where(near, np.abs(g * d) + eg * d, np.where(Yr > 0, eg * d + 2.0 * M.U * np.abs(G), 0.0))
    elif act == M.ACT_TANH_RES:
        t = Yr - res[:, :1].astype(np.float64)
        G = g * (1.0 - t * t) * d
        eG = np.abs(g) * d * (2.0 * np.abs(t) * (yb + 2.0 * M.U * np.abs(t)) + 2.0 * M.U * (t * t + np.abs(1.0 - t * t))) + 4.0 * M.U * np.abs(G)
    else:
        G, eG = g, eg
    i = 0
    Pr, Pm = M.dgrad(G, W, K, C)
    eP = M.product_bound(Pm, Co) + M.dgrad(eG, np.abs(W), K, C)[0]
    o = 0
    for w, f in zip(widths, live):
        if f:
            ref, mag = CM.clenshaw(L, Pr[:, :, o:o + w], K)
            _, emag = CM.clenshaw(L, eP[:, :, o:o + w], K)
            check('cheb_poly dZ', f'{name} part at {o}', grads[i][:nv], ref, CM.plane_bound(L, K - 1, mag) + emag)
            i += 1
        o += w
    A = M.design(T, S)
    gWr, gWm = A.T @ G, np.abs(A).T @ np.abs(G)
    # dW: the summation tree's own roundings, G's error through |A|, and the planes' errors (inherited, per column of A) through |G|
    nb = -(-mesh.N // M.WGRAD_ROWS)
    bW = M.wgrad_bound(gWm, max(nv, 1), A.shape[1], nb) + np.abs(A).T @ eG + maj['eA'].T @ np.abs(G)
    check('cheb_poly dW', name, grads[i], gWr, bW)
    i += 1
    if resd is not None:
        gr = np.zeros((nv, 4))
        gr[:, 0] = g[:, 0]
        check('cheb_poly dres', name, grads[i][:nv], gr)
        i += 1
    if post:
        check('cheb_poly dW2', name, grads[i], Y1.T @ gU, M.wgrad_bound(np.abs(Y1).T @ np.abs(gU), max(nv, 1), 20, nb) + eY1.T @ np.abs(gU))
    # which branch of _ChebPoly.backward ran
    fuse = post and act == M.ACT_RELU and not y_cot and not with_drop      # the ReLU gradient rides on the gU @ Wb2 launch
    head = fuse and all(live)                                              # ... and that launch is qt_head_dgrad
    assert ('qt_head_dgrad' in recording) == bool(head and nv > 0), recording
    assert ('qt_act_bwd' in recording) == (act != M.ACT_NONE and not fuse), recording
    assert recording.count('qt_wgrad') == 1 + int(post) and 'qt_wgrad_group' not in recording
    if post:
        assert recording.count('qt_dense2') == (1 if head else 3)          # forward; gU @ Wb2 and the data gradient
    if live != (True,) * len(widths):
        assert grads[0].shape[1] == widths[1]


@pytest.mark.parametrize('tag,uses', [('D', 3), ('S', 17), ('T', 3)])
def test_gradacc_chain(recording, tag, uses):
    """Y_t = cheb_poly((X_t, H_t), W, K = 3, Ks = 1, acc), H_{t+1} = Y_t: the deferred weight gradient of all uses -- one
    qt_wgrad_group launch per 16 uses (17 uses: a second chunk) and one qt_colsum -- against the sum of the model's per-use A^T G."""
    from qtmpnn import ops
    mesh, L = get(tag)
    nv, K, Co = L.N, 3, 16
    rng = np.random.default_rng(uses)
    W = M.draw(rng, K * 20 + 4, Co) * np.float32(0.005)        # (|W| small enough that the error majorants of 17 chained uses do not grow)
    W[K * 20 + 1:] = 0
    Xs = [M.draw(rng, nv, 4) for _ in range(uses)]
    H0, gTs = M.draw(rng, nv, Co), [M.draw(rng, nv, Co) for _ in range(uses)]       # every Y_t has a cotangent of its own
    Wd, acc = _t(W).requires_grad_(True), ops.GradAcc()
    H, Ys = pad(mesh, H0), []
    for X in Xs:
        H = ops.cheb_poly((pad(mesh, X), H), Wd, mesh, K, 1, acc=acc)
        Ys.append(H)
    (gW,) = torch.autograd.grad(Ys, [Wd], [pad(mesh, g, 0.0) for g in gTs])
    # model: forward chain, then backwards; every bound carries the inherited errors through the same majorants
    S = np.zeros((nv, 4))
    S[:, 0] = 1.0
    Hs, Ts, eHs = [H0.astype(np.float64)], [], [np.zeros((nv, Co))]
    Wf, c = np.asarray(W, np.float64), CM.hop_factor(L)
    for X in Xs:
        Zt = np.concatenate([X.astype(np.float64), Hs[-1]], axis=1)
        T, Am = CM.planes(L, Zt, K)
        _, eIn = CM.planes(L, np.concatenate([np.zeros((nv, 4)), eHs[-1]], axis=1), K)        # H's error through the recurrence
        Yr, _, maj = M.forward(T, S, Wf)
        eT = np.stack([CM.plane_bound(L, k, Am[k]) + eIn[k] for k in range(K)])
        Ts.append((T, eT))
        Hs.append(Yr[0])
        eHs.append(M.product_bound(maj['mag'], K * 20 + 4) + M.design(eT, np.zeros((nv, 4))) @ np.abs(Wf))
    check('GradAcc chain', f'{tag} {uses} uses H', H[:nv], Hs[-1], eHs[-1])
    G, eG = np.zeros((nv, Co)), np.zeros((nv, Co))
    ref, bnd = np.zeros_like(Wf), np.zeros_like(Wf)
    nb = -(-mesh.N // M.WGRAD_ROWS) * uses
    per_use = []
    for (T, eT), gT in zip(reversed(Ts), reversed(gTs)):
        # dL/dY_t = its own cotangent + what the next use hands back (one add)
        eG = eG + 2.0 * M.U * (np.abs(gT) + np.abs(G)) * bool(np.any(G))
        G = gT.astype(np.float64) + G
        A = M.design(T, S)
        per_use.append(np.abs(A.T @ G).max())
        ref += A.T @ G
        bnd += M.wgrad_bound(np.abs(A).T @ np.abs(G), max(nv, 1), A.shape[1], nb) + np.abs(A).T @ eG + M.design(eT, np.zeros((nv, 4))).T @ np.abs(G)
        Pr, Pm = M.dgrad(G, Wf, K, 20)
        eP = M.product_bound(Pm, Co) + M.dgrad(eG, np.abs(Wf), K, 20)[0]
        gz, mag = CM.clenshaw(L, Pr[:, :, 4:], K)
        _, emag = CM.clenshaw(L, eP[:, :, 4:], K)
        G, eG = gz, CM.plane_bound(L, K - 1, mag) + emag
    check('GradAcc chain', f'{tag} {uses} uses dW', gW, ref, bnd)
    # every use weighs in: leaving out any one of them (the 17th sits alone in the second chunk of _wgrad_group) is >= 10 bounds away
    print(f'  [GradAcc chain] {tag} {uses} uses: largest entry per use {min(per_use):.3g} .. {max(per_use):.3g}, largest bound {bnd.max():.3g}')
    assert min(per_use) >= 10.0 * bnd.max()
    assert recording.count('qt_wgrad_group') == -(-uses // 16) and recording.count('qt_colsum') == 1 and 'qt_wgrad' not in recording


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per family of this session (the figures of profiles/gemm_f64.txt) and what ran: every kernel
    of qt_dense2 by shape and every entry point of the dense half at least once."""
    for fam in sorted(WORST):
        print(f'  worst [{fam}]: {WORST[fam]:.3g}')
    print('  kernels of qt_dense2 by shape:', ', '.join(sorted(KERNELS)))
    print('  entry points:', ', '.join(f'{n} x{ENTRIES.count(n)}' for n in sorted(set(ENTRIES))))
    assert all(v <= 1.0 for v in WORST.values())
    if not {'dense2 exact', 'head_dgrad exact', 'act_bwd exact', 'wgrad exact', 'wgrad_group exact', 'colsum exact', 'GradAcc chain'} <= set(WORST):
        return                                         # (a selection of the file ran: nothing to say about what it covers)
    if 'QT_GEMM_NO_ROW16' in os.environ or 'QT_GEMM_BF16X3' in os.environ:
        return                                         # (the library's switches change what a shape launches: gemm_f64.dispatch is the default's)
    assert KERNELS >= {'k_gemm_skinny<256>', 'k_gemm_row16', 'k_gemm_skinny<64>', 'k_gemm_fwd<2>', 'k_gemm_fwd<3>', 'k_gemm_fwd<4>'}
    assert {'qt_dense2', 'qt_head_dgrad', 'qt_act_bwd', 'qt_wgrad', 'qt_wgrad_group', 'qt_colsum'} <= set(ENTRIES)
