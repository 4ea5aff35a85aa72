"""Host checks of the float64 model of the dense products (tests/gemm_f64.py) on its own: it agrees with float64 torch autograd
of the same expression, its layout helpers round-trip, a float32 emulation of every real-valued case of
tests/test_gpu_gemm_f64.py stays within its bound whatever the order of its sums -- and single mutations of the model's output
land at >= 10 bounds at those shapes, so the GPU comparison would see them.  No GPU, nothing of qtmpnn.

Mutation -> the GPU case that sees the same fault in a kernel:
  one node row dropped / counted twice   test_wgrad_exact, test_wgrad_real       (`rend` one short in k_gemm_wgrad)
  last k-quad dropped                    test_forward_dispatch_exact, test_forward_real
  two weight rows swapped, W as W^T      test_forward_real, test_head_dgrad
  part b read with part a's stride       test_operand_forms_exact                (lda0 / lda0b swapped in build_quad_table)
  slice-major read as row-major          test_output_forms_exact, test_operand_forms_exact   (`sm && pl > 0` in plane_piece)
  one operand rounded to bf16            test_forward_real, test_tanh_res_real, test_head_dgrad[real], test_wgrad_real
  bias rows skipped                      test_forward_real, test_wgrad_real
  res column off by one                  test_tanh_res_real, test_act_bwd_tanh_real
"""
import numpy as np
import pytest
import torch

import gemm_f64 as M

REAL_FORWARD = M.REAL_FORWARD         # test_forward_real, N = 129


def operands(Kred, NB, N, seed, scale=1.0):
    Ka, Ca, Cab, Ks = M.split_kred(Kred)
    rng = np.random.default_rng(seed)
    return (M.draw(rng, Ka, N, Ca + Cab), M.draw(rng, N, Ks) if Ks else None, M.draw(rng, Kred, NB) * np.float32(scale), rng, Ca)


def worst(got, ref, bound):
    bound = np.broadcast_to(bound, np.shape(ref))
    err = np.abs(np.asarray(got, np.float64) - ref)
    pos = bound > 0
    if (err[~pos] != 0).any():
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# --------------------------------------------------------------------------------------------------- model against autograd
@pytest.mark.parametrize('Kred,NB,N', [(20, 4, 9), (64, 16, 33), (104, 64, 17)])
def test_model_equals_float64_autograd(Kred, NB, N):
    Ka, Ca, Cab, Ks = M.split_kred(Kred)
    planes, S, W, rng, _ = operands(Kred, NB, N, Kred, 4.0 / Kred)
    res, drop = M.draw(rng, N, 4), ((rng.random(N) > 0.3) * 1.25).astype(np.float32)
    gY, gY2 = M.draw(rng, N, NB), M.draw(rng, N, NB)
    tp, tS, tW, tr = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (planes, S, W, res))
    A = torch.cat([tp[k] for k in range(Ka)] + [tS], dim=1)
    d = torch.from_numpy(drop.astype(np.float64))[:, None]
    for act in (M.ACT_NONE, M.ACT_RELU, M.ACT_TANH_RES):
        pre = A @ tW
        y = pre if act == M.ACT_NONE else (torch.relu(d * pre) if act == M.ACT_RELU else torch.tanh(d * pre) + tr[:, :1])
        gp, gS, gW, gr = torch.autograd.grad(y, [tp, tS, tW, tr], torch.from_numpy(M.f64(gY) + M.f64(gY2)), allow_unused=True)
        kw = {} if act == M.ACT_NONE else dict(drop=drop)
        Y, _, _ = M.forward(planes, S, W, 1, NB, 0, act, res if act == M.ACT_TANH_RES else None, **kw)
        np.testing.assert_allclose(Y[0], y.detach().numpy(), rtol=1e-13, atol=1e-13)
        G = gY.astype(np.float64) + gY2
        if act != M.ACT_NONE:
            G, gres, _ = M.act_bwd(gY, Y[0], act, res if act == M.ACT_TANH_RES else None, drop, gY2)
            if act == M.ACT_TANH_RES:
                # (gres is the kernel's contract, not autograd's: only column 0 of Y is consumed, so column 0 of gres = g[:, 0])
                assert (gres[:, 1:] == 0).all() and np.allclose(gres[:, 0], (M.f64(gY) + M.f64(gY2))[:, 0])
        P, _ = M.dgrad(G, W, Ka, Ca + Cab)
        np.testing.assert_allclose(P, gp.numpy(), rtol=1e-12, atol=1e-12)
        gWm, _ = M.wgrad(planes, S, G)
        np.testing.assert_allclose(gWm, gW.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(G @ M.f64(W)[Ka * (Ca + Cab):].T, gS.numpy(), rtol=1e-12, atol=1e-12)      # the bias block's own gradient


def test_head_model_equals_float64_autograd():
    rng = np.random.default_rng(5)
    N, K, C = 21, 3, 20
    Z, W1, W2, gU = M.draw(rng, K, N, C), M.draw(rng, K * C + 4, 16) * np.float32(0.1), M.draw(rng, 20, 4), M.draw(rng, N, 4)
    S = np.zeros((N, 4), np.float32)
    S[:, 0] = 1
    Y, Um, _ = M.forward(Z, S, W1, 1, 16, 0, M.ACT_RELU, W2=W2)
    tZ, tW1, tW2 = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (Z, W1, W2))
    tS = torch.from_numpy(S.astype(np.float64))
    y = torch.relu(torch.cat([tZ[k] for k in range(K)] + [tS], dim=1) @ tW1)
    u = torch.cat([y, tS], dim=1) @ tW2
    np.testing.assert_allclose(Um, u.detach().numpy(), rtol=1e-13, atol=1e-13)
    gZ, = torch.autograd.grad(u, [tZ], torch.from_numpy(gU.astype(np.float64)))
    G, P, _ = M.head_bwd(gU, W2, Y[0], W1, K, C)
    np.testing.assert_allclose(P, gZ.numpy(), rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('sm', [False, True])
@pytest.mark.parametrize('lda', [(0, 0), (24, 36)])
@pytest.mark.parametrize('K,Ca,Cab', [(1, 4, 16), (3, 4, 16), (5, 20, 0)])
def test_layouts_round_trip(K, Ca, Cab, lda, sm):
    rng = np.random.default_rng(K)
    N, cap = 37, 50
    planes = M.draw(rng, K, N, Ca + Cab)
    lda = lda if Cab else (lda[1], 0)
    parts = M.pack_operand(planes, Ca, cap, lda, sm=sm)
    assert len(parts) == 1 + (Cab > 0) and all(np.isnan(q['wide'][N:]).all() for q in parts)
    assert np.array_equal(M.unpack_operand(parts, N, sm), planes)
    if K > 1:
        rest = parts[0]['rest']
        assert rest.shape == (K - 1, cap, Ca)
        # slice-major: quad q of row i of plane k sits at ((k (Ca / 4) + q) cap + i) 4, as build_quad_table addresses it
        flat, k, q, i = rest.reshape(-1), K - 2, Ca // 4 - 1, N - 1
        at = ((k * (Ca // 4) + q) * cap + i) * 4 if sm else (k * cap + i) * Ca + 4 * q
        assert np.array_equal(flat[at:at + 4], planes[k + 1, i, 4 * q:4 * q + 4])
    out = M.draw(rng, K, cap, Ca + Cab)
    a, b = out[:, :, :Ca].copy(), (out[:, :, Ca:].copy() if Cab else None)
    if sm and K > 1:
        a[1:] = M.slice_major(a[1:])
        if Cab:
            b[1:] = M.slice_major(b[1:])
    assert np.array_equal(M.unpack_planes(a, b, sm), out)
    assert np.array_equal(M.row_major(M.slice_major(out)), out)


def test_dispatch_names_every_kernel():
    assert {k for *_, k in M.DISPATCH} == {'k_gemm_skinny<256>', 'k_gemm_row16', 'k_gemm_skinny<64>', 'k_gemm_fwd<2>', 'k_gemm_fwd<3>', 'k_gemm_fwd<4>'}
    for Kred, NB, nb, kernel in M.DISPATCH:
        Kb, _, Cbb = nb or M.split_nb(NB)
        assert M.dispatch(Kred, NB, Kb, Cbb) == kernel and Kred // 4 <= M.MAXQ
    assert M.gemm_nt(100) == 4 and M.gemm_nt(280) == 3 and M.gemm_nt(96) == 3 and M.gemm_nt(64) == 2
    assert M.dispatch(64, 16, act=M.ACT_TANH_RES) == 'k_gemm_skinny<64>' and M.dispatch(64, 16, has_W=False) == 'k_gemm_fwd<2>'


# ---------------------------------------------------------------------------------------------- emulation within the bounds
def orders(n, rng):
    return [rng.permutation(n), np.arange(n)[::-1]]


@pytest.mark.parametrize('Kred,NB', REAL_FORWARD)
def test_emulated_forward_within_bound(Kred, NB):
    planes, S, W, rng, _ = operands(Kred, NB, 129, Kred + NB)
    Y, _, maj = M.forward(planes, S, W, 1, NB, 0)
    for order in orders(Kred, rng):
        r = worst(M.emulate_product(M.design(planes, S), W, order), Y[0], M.product_bound(maj['mag'], Kred))
        print(f'  forward ({Kred}, {NB}): {r:.3g}')
        assert r <= 1.0


@pytest.mark.parametrize('Kred,NB,N', M.REAL_TANH + M.REAL_TANH_WIDE)
def test_emulated_tanh_within_bound(Kred, NB, N):
    planes, S, W, rng, _ = operands(Kred, NB, N, Kred + NB + N, 4.0 / Kred)
    res, drop = M.draw(rng, N, 4), ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
    Y, _, maj = M.forward(planes, S, W, 1, NB, 0, M.ACT_TANH_RES, res, drop)
    for order in orders(Kred, rng):
        pre = M.emulate_product(M.design(planes, S), W, order)
        got = (np.tanh((drop[:, None] * pre).astype(np.float32)).astype(np.float32) + res[:, :1]).astype(np.float32)
        r = worst(got, Y[0], M.forward_bound(maj, M.ACT_TANH_RES, Y[0]))
        print(f'  tanh ({Kred}, {NB}) N={N}: {r:.3g}')
        assert r <= 1.0


@pytest.mark.parametrize('Mw,Co,N', M.REAL_WGRAD)
def test_emulated_wgrad_within_bound(Mw, Co, N):
    """The kernels' tree with any order inside its chains: per z-block of 512 rows the RG = 4 / FW row groups sum their rows of every
    32-row pass, the groups are added, then the blocks."""
    planes, S, _, rng, _ = operands(Mw, 4, N, Mw + Co + N)
    G = M.draw(rng, N, Co)
    ref, mag = M.wgrad(planes, S, G)
    A = M.design(planes, S).astype(np.float32)
    RG = 4 // M.wgrad_fw(Mw)
    for rev in (False, True):
        slabs = []
        for z in range(-(-N // M.WGRAD_ROWS)):
            rows = np.arange(z * M.WGRAD_ROWS, min(N, (z + 1) * M.WGRAD_ROWS))
            groups = []
            for rg in range(RG):
                mine = rows[((rows - rows[0]) % 32) // (32 // RG) == rg]
                assert len(mine) <= M.wgrad_count(N, Mw) - (RG - 1) - 3 - min(-(-N // M.WGRAD_ROWS), 32)
                groups.append(M.emulate_product(A.T, G, mine[::-1] if rev else rng.permutation(mine)))
            slabs.append(M.emulate_sum(np.stack(groups)))
        got = M.emulate_sum(np.stack(slabs), range(len(slabs) - 1, -1, -1) if rev else None)
        r = worst(got, ref, M.wgrad_bound(mag, N, Mw))
        print(f'  wgrad M={Mw} Co={Co} N={N}: {r:.3g}')
        assert r <= 1.0


@pytest.mark.parametrize('widths,N', M.REAL_HEAD)
def test_emulated_head_within_bound(widths, N):
    rng = np.random.default_rng(N)
    K, C = 3, sum(widths)
    gU, W2, Y, W1 = M.draw(rng, N, 4), M.draw(rng, 20, 4), M.draw(rng, N, 16), M.draw(rng, K * C + 4, 16)
    Gr, Pr, parts = M.head_bwd(gU, W2, Y, W1, K, C)
    eG, eP = M.head_bounds(parts)
    for order in orders(4, rng):
        G = np.where(Y > 0, M.emulate_product(gU, W2[:16].T, order), np.float32(0))
        P = M.emulate_product(G, W1[:K * C].T, np.arange(16)[::-1]).reshape(N, K, C).transpose(1, 0, 2)
        assert worst(G, Gr, eG) <= 1.0 and worst(P, Pr, eP) <= 1.0


@pytest.mark.parametrize('Co,rs,N', M.REAL_ACT)
def test_emulated_act_bwd_within_bound(Co, rs, N):
    rng = np.random.default_rng(Co + N)
    res, drop = M.draw(rng, N, rs), ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
    Y = (np.tanh(M.draw(rng, N, Co)) + res[:, :1]).astype(np.float32)
    gY, gY2 = M.draw(rng, N, Co), M.draw(rng, N, Co)
    Gr, _, parts = M.act_bwd(gY, Y, M.ACT_TANH_RES, res, drop, gY2)
    f = np.float32
    t = (Y - res[:, :1]).astype(f)
    got = (((gY + gY2).astype(f) * (f(1) - (t * t).astype(f)).astype(f)).astype(f) * drop[:, None]).astype(f)
    assert worst(got, Gr, M.act_bwd_bound(parts, Gr)) <= 1.0


# --------------------------------------------------------------------------------------------------------------- mutations
def test_mutations_of_the_forward_product_are_ten_bounds_away():
    """Every mutation at every shape of test_forward_real.  (Kred = 512 is not among them: twice 512 roundings at their worst and
    of one sign lie above the random walk of bf16's 2^-9 errors, ~5 bounds; (512, 128) runs as an exact case only.)"""
    for Kred, NB in REAL_FORWARD:
        planes, S, W, rng, Ca = operands(Kred, NB, 129, Kred + NB)
        Ka, _, Cab, Ks = M.split_kred(Kred)
        Y, _, maj = M.forward(planes, S, W, 1, NB, 0)
        bound = M.product_bound(maj['mag'], Kred)
        A = M.design(planes, S)
        Wd = M.f64(W)
        muts = {}
        muts['last k-quad dropped'] = A[:, :-4] @ Wd[:-4]
        sw = Wd.copy()
        sw[[1, 2]] = sw[[2, 1]]
        muts['two weight rows swapped'] = A @ sw
        if Kred == NB:
            muts['W read as W^T'] = A @ Wd.T
        muts['operand rounded to bf16'] = M.f64(M.bf16(A.astype(np.float32))) @ Wd
        muts['weight rounded to bf16'] = A @ M.f64(M.bf16(W))
        if Ks:
            muts['bias rows skipped'] = A[:, :-Ks] @ Wd[:-Ks]
        if Ka > 1:
            wrong = planes.copy()
            wrong[1:] = M.slice_major(planes[1:])
            muts['slice-major read as row-major'] = M.design(wrong, S) @ Wd
        if (Ca, Cab) == (4, 16):
            # plane 0 of part b as a column view (ld 36) read with part a's stride (24): row i starts 24 i floats into the matrix
            parts = M.pack_operand(planes, Ca, lda=(24, 36), junk=M.draw(rng, 129, 40))
            flat = np.concatenate([parts[1]['wide'].reshape(-1), np.zeros(64, np.float32)])
            wrong = planes.copy()
            wrong[0, :, Ca:] = np.stack([flat[24 * i + 8:24 * i + 8 + Cab] for i in range(129)])
            muts["part b read with part a's stride"] = M.design(wrong, S) @ Wd
        for name, got in muts.items():
            r = worst(got, Y[0], bound)
            print(f'  forward ({Kred}, {NB}) {name}: {r:.3g}')
            assert r >= 10.0, (Kred, NB, name, r)


def test_mutations_of_the_tanh_epilogue_are_ten_bounds_away():
    for Kred, NB, N in M.REAL_TANH + M.REAL_TANH_WIDE:
        planes, S, W, rng, _ = operands(Kred, NB, N, Kred + NB + N, 4.0 / Kred)
        res, drop = M.draw(rng, N, 4), ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
        Y, _, maj = M.forward(planes, S, W, 1, NB, 0, M.ACT_TANH_RES, res, drop)
        bound = M.forward_bound(maj, M.ACT_TANH_RES, Y[0])
        muts = {'res column off by one': M.forward(planes, S, W, 1, NB, 0, M.ACT_TANH_RES, res[:, 1:], drop)[0],
                'dropout mask ignored': M.forward(planes, S, W, 1, NB, 0, M.ACT_TANH_RES, res, None)[0],
                'operand rounded to bf16': M.forward(M.bf16(planes), S, W, 1, NB, 0, M.ACT_TANH_RES, res, drop)[0],
                'bias rows skipped': M.forward(planes, 0 * S, W, 1, NB, 0, M.ACT_TANH_RES, res, drop)[0]}
        for name, got in muts.items():
            r = worst(got[0], Y[0], bound)
            print(f'  tanh ({Kred}, {NB}) N={N} {name}: {r:.3g}')
            assert r >= 10.0, (Kred, NB, N, name, r)


def test_mutations_of_the_weight_gradient_are_ten_bounds_away():
    """One node row dropped or counted twice, skipped bias rows and a bf16 operand at every shape of test_wgrad_real."""
    for Mw, Co, N in M.REAL_WGRAD:
        planes, S, _, rng, _ = operands(Mw, 4, N, Mw + Co + N)
        Ks = M.split_kred(Mw)[3]
        G = M.draw(rng, N, Co)
        ref, mag = M.wgrad(planes, S, G)
        bound = M.wgrad_bound(mag, N, Mw)
        A = M.design(planes, S)
        last = np.arange(N) != N - 1
        muts = {'one node row dropped': A[last].T @ M.f64(G)[last],
                'one row counted twice': ref + np.outer(A[N // 2], M.f64(G)[N // 2]),
                'operand rounded to bf16': M.f64(M.bf16(A.astype(np.float32))).T @ M.f64(G),
                'gradient rounded to bf16': A.T @ M.f64(M.bf16(G))}
        if Ks:
            muts['bias rows skipped'] = np.concatenate([ref[:-Ks], np.zeros((Ks, Co))])
        for name, got in muts.items():
            r = worst(got, ref, bound)
            print(f'  wgrad M={Mw} Co={Co} N={N} {name}: {r:.3g}')
            assert r >= 10.0, (Mw, Co, N, name, r)


def test_mutations_of_the_head_and_activation_backward_are_ten_bounds_away():
    for widths, N in M.REAL_HEAD:
        rng = np.random.default_rng(N)
        K, C = 3, sum(widths)
        gU, W2, Y, W1 = M.draw(rng, N, 4), M.draw(rng, 20, 4), M.draw(rng, N, 16), M.draw(rng, K * C + 4, 16)
        Gr, Pr, parts = M.head_bwd(gU, W2, Y, W1, K, C)
        eG, eP = M.head_bounds(parts)
        sw = W1.copy()
        sw[[0, 1]] = sw[[1, 0]]
        sq = W2.copy()
        sq[:4] = W2[:4].T
        muts = {'two weight rows swapped': M.head_bwd(gU, W2, Y, sw, K, C), 'G rounded to bf16': M.head_bwd(M.bf16(gU), W2, Y, W1, K, C),
                'W2 quad read as its transpose': M.head_bwd(gU, sq, Y, W1, K, C), 'relu mask dropped': M.head_bwd(gU, W2, np.abs(Y), W1, K, C)}
        for name, (G, P, _) in muts.items():
            r = max(worst(G, Gr, eG), worst(P, Pr, eP))
            print(f'  head {widths} N={N} {name}: {r:.3g}')
            assert r >= 10.0, (widths, N, name, r)
    for Co, rs, N in M.REAL_ACT:
        rng = np.random.default_rng(Co + N)
        res, drop = M.draw(rng, N, max(rs, 2)), ((rng.random(N) > 0.2) * 1.25).astype(np.float32)
        Y = (np.tanh(M.draw(rng, N, Co)) + res[:, :1]).astype(np.float32)
        gY, gY2 = M.draw(rng, N, Co), M.draw(rng, N, Co)
        Gr, _, parts = M.act_bwd(gY, Y, M.ACT_TANH_RES, res, drop, gY2)
        bound = M.act_bwd_bound(parts, Gr)
        muts = {'res column off by one': M.act_bwd(gY, Y, M.ACT_TANH_RES, res[:, 1:], drop, gY2)[0],
                'second gradient dropped': M.act_bwd(gY, Y, M.ACT_TANH_RES, res, drop, None)[0],
                'Y rounded to bf16': M.act_bwd(gY, M.bf16(Y), M.ACT_TANH_RES, res, drop, gY2)[0]}
        for name, got in muts.items():
            r = worst(got, Gr, bound)
            print(f'  act_bwd Co={Co} rs={rs} N={N} {name}: {r:.3g}')
            assert r >= 10.0, (Co, rs, N, name, r)
