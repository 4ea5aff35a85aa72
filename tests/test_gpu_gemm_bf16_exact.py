"""The two bf16 kernels that share the fp32 kernels' staged epilogue (csrc/qt_gemm.h: stage_and_store) -- k_gemm_sb behind
qt_dense_sb and k_gemm_fwd3 behind qt_dense2 under QT_GEMM_BF16X3=1 -- against the float64 model tests/gemm_f64.py, entry for entry.

Operands come from {-2, -1, 1, 2} and dropout factors from {0, 2}: exact in bf16, so the mid and lo terms of both splits are zero,
every partial sum is an integer below 2^24 (test_exact_sums_stay_below_2_24 checks that on the model alone) and the bound is 0:
one dropped, doubled or misplaced float4 piece of an output row fails with certainty.  The tolerances of tests/test_gpu_ops.py
(2e-5 / 2e-6 of the largest entry) would not see one.  Every case has 133 valid rows in a capacity of 140 with the device-side
count -- two 128-row tiles, the second ragged -- outputs pre-filled with the sentinel and NaN capacity rows, as in
tests/test_gpu_gemm_f64.py, whose helpers run the cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_f64 as M

N, CAP = 133, 140
K_SB = 80                                    # one full 64-row pass of W plus a 16-row tail
# (Kb, Cb, Cbb): NB = 280, NT = 4, three column blocks, the last 24 columns wide, both parts | NT = 2, one pass | NB = 48, ragged
SB_SHAPES = [(7, 8, 32), (1, 64, 0), (3, 16, 0)]
KRED_X3 = 104                                # 5 x 20 + 4: no multiple of 16, the zeroed k tail is used
# name, (Kb, Cb, Cbb), activation, dropout column, slice-major planes
X3_CASES = [('relu + drop NB=64', (1, 64, 0), M.ACT_RELU, True, False),
            ('tanh + res NB=32', (1, 32, 0), M.ACT_TANH_RES, True, False),
            ('NB=280 slice-major', (7, 8, 32), M.ACT_NONE, False, True),
            ('NB=280 row-major', (7, 8, 32), M.ACT_NONE, False, False)]


def test_exact_sums_stay_below_2_24():
    """The model alone: the majorant |A| |W| of every shape, times the dropout factor 2, bounds every partial sum; and the
    operand values are their own bf16 roundings."""
    rng = np.random.default_rng(0)
    for Kred, shapes in ((K_SB, SB_SHAPES), (KRED_X3, [c[1] for c in X3_CASES])):
        for Kb, Cb, Cbb in shapes:
            _, _, maj = M.forward(M.ints(rng, 1, N, Kred), None, M.ints(rng, Kred, Kb * (Cb + Cbb)), Kb, Cb, Cbb)
            assert 2.0 * maj['mag'].max() < 2.0 ** 24
    vals = np.array([-2.0, -1.0, 0.0, 1.0, 2.0], np.float32)
    assert (M.bf16(vals) == vals).all()


@pytest.mark.gpu
@pytest.mark.parametrize('Kb,Cb,Cbb', SB_SHAPES)
def test_dense_sb_exact(Kb, Cb, Cbb):
    """qt_dense_sb == A W entry for entry; W^T's hi term is W^T itself, its lo term 0."""
    import torch
    import test_gpu_gemm_f64 as T
    rng = np.random.default_rng(Kb + Cb)
    A, W = M.ints(rng, N, K_SB), M.ints(rng, K_SB, Kb * (Cb + Cbb))
    Yr, _, maj = M.forward(A[None], None, W, Kb, Cb, Cbb)
    assert maj['mag'].max() < 2.0 ** 24
    Ad, hi = T.pad_rows(A, CAP), T._t(W.T).to(torch.bfloat16)
    lo, nd = torch.zeros_like(hi), T.n_dev(N)
    out, outb = T.filled(Kb, CAP, Cb), T.filled(Kb, CAP, Cbb) if Cbb else None
    T.call('qt_dense_sb', T.p(Ad), 0, K_SB, hi.data_ptr(), lo.data_ptr(), Kb, Cb, Cbb, CAP, T.p(nd), T.p(out), T.p(outb))
    Y = M.unpack_planes(T._np(out), None if outb is None else T._np(outb))
    T.check('dense_sb exact', f'({Kb}, {Cb}, {Cbb})', Y[:, :N], Yr)
    assert (Y[:, N:] == T.SENT).all(), 'a row past the device-side count was written'


def bf16x3_cases():
    """The k_gemm_fwd3 cases (the child process of test_bf16x3_exact: QT_GEMM_BF16X3 is latched per process)."""
    import test_gpu_gemm_f64 as T
    assert os.environ.get('QT_GEMM_BF16X3') == '1'
    for name, nb, act, with_drop, sm in X3_CASES:
        rng = np.random.default_rng(len(name))
        drop = rng.choice([0.0, 2.0], size=N).astype(np.float32) if with_drop else None
        if act != M.ACT_TANH_RES:
            kw = dict(act=act, drop=drop) if act != M.ACT_NONE else {}
            T.exact_forward(name, KRED_X3, nb, N, CAP, out_sm=sm, in_sm=sm, **kw)
            continue
        # the pre-activation is exact; tanhf and the two roundings around it are held to the model's bound of the fp32 case
        Ka, Ca, Cab, Ks = M.split_kred(KRED_X3)
        planes, S, W, res = M.ints(rng, Ka, N, Ca + Cab), M.ints(rng, N, Ks), M.ints(rng, KRED_X3, nb[1]), M.ints(rng, N, 4)
        Yr, _, maj = M.forward(planes, S, W, 1, nb[1], 0, act, res, drop)
        Y, _ = T.dense2(planes, S, W, 1, nb[1], 0, N, CAP, Ca=Ca, act=act, res=res, res_view=0, drop=drop)
        T.check('dense2 bf16x3', name, Y[0, :N], Yr[0], M.forward_bound(maj, act, Yr[0]))
        assert (Y[:, N:] == T.SENT).all()


@pytest.mark.gpu
def test_bf16x3_exact():
    """k_gemm_fwd3<2, 128> (NB = 64, 32) and <4, 64> (NB = 280) through qt_dense2, in one child process with the switch set."""
    env = dict(os.environ, QT_GEMM_BF16X3='1')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count('[dense2') == len(X3_CASES), out.stdout          # every case ran and printed its ratio


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), 'quadtree-mpnnlstm_amd')]
    bf16x3_cases()
