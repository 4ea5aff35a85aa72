"""Host checks of the float64 model of the decoder head's input (tests/head_f64.py) on its own: it agrees with float64 torch
autograd of relu(layer_norm(O)) | concat, a float32 emulation of k_head_fwd / k_head_bwd with the kernels' reduction trees stays
within one bound on the cases of tests/test_gpu_head_f64.py, single mutations of that emulation land at >= 10 bounds on a named
case of that file, and no case leaves more than 0.1 % of its entries out at the ReLU kink.  No GPU, nothing of qtmpnn.

Mutation -> the GPU case (head_f64.BY_NAME) whose comparison sees it:
  eps 1e-6                                   h16-N777-small-view-exact-cat          Za, gO
  variance / (h - 1)                         h8-N777-randn-dense-exact-cat          Za, gO
  ReLU mask from gamma xhat, without beta    h32-N777-randn-dense-exact-cat         gO, slabs
  LayerNorm backward without xhat mean(g xhat)   h64-N777-randn-dense-exact-cat     gO
  gamma / beta sums count capacity rows      h16-N777-randn-view-cap1100-nocat      slabs (NaN rows reach them)
  gamma / beta sums drop the last ragged group   h128-N777-randn-dense-exact-cat, h8-N70001-randn-view-exact-cat    slabs
  accumulate overwrites                      h8-N777-randn-dense-exact-cat          slabs of the second launch
  gconcat read from column 1                 h16-N777-randn-dense-exact-cat         gconcat (bound 0)
"""
import numpy as np
import pytest
import torch

import head_f64 as M


def worst(got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(bound, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    pos = bound > 0
    if (err[~pos] != 0).any():
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def ratios(case, second=False, **mut):
    """Worst error / bound per output of the (mutated) emulation against the model on a case of the GPU file."""
    c = M.BY_NAME[case] if isinstance(case, str) else case
    x = M.inputs(c)
    h, N, cap = c['h'], c['N'], c['cap'] or c['N']
    nblk = M.bwd_blocks(cap, h)
    O, gZa, gZb = (np.concatenate([a, np.full((cap - N, a.shape[1]), np.nan, np.float32)]) for a in (x['O'], x['gZa'], x['gZb']))
    Za, Zb, pre = M.forward(x['O'], x['ln'], x['concat'], c['hp'])
    gO, gcat, _ = M.backward(x['gZa'], x['gZb'], x['O'], x['ln'])
    slabs, mag, inh, cnt = M.part_slabs(x['gZa'], x['O'], x['ln'], nblk, h // 4)
    prev = None
    if second:          # the second of two launches into the same slabs (accumulate = 1)
        prev = M.emulate(O, x['ln'], x['concat'], c['hp'], gZa, gZb, nblk, N)['slabs']
        slabs = 2.0 * slabs
    e = M.emulate(O, x['ln'], x['concat'], c['hp'], gZa, gZb, nblk, N, prev=prev, **mut)
    fb = M.forward_bound(x['O'], x['ln'])
    za_err = np.where(x['near'], np.minimum(np.abs(e['Za']), np.abs(e['Za'] - pre)), np.abs(e['Za'] - Za))
    sb = M.slab_bound(mag, inh, cnt) * (2 if second else 1) + (2.0 * M.U * np.abs(slabs) if second else 0.0)
    return dict(Za=worst(za_err, 0.0 * za_err, fb), Zb=worst(e['Zb'], Zb, 0.0), gO=worst(e['gO'], gO, M.backward_bound(x['gZa'], x['O'], x['ln'])),
                gconcat=worst(e['gconcat'], gcat, 0.0), slabs=worst(e['slabs'], slabs, sb))


# -------------------------------------------------------------------------------------------------- model against autograd
@pytest.mark.parametrize('h,N,family', [(8, 5, 'randn'), (16, 33, 'small'), (64, 9, 'offset'), (128, 3, 'randn')])
def test_model_equals_float64_autograd(h, N, family):
    rng = np.random.default_rng(h + N)
    O, ln = M.draw_rows(rng, family, N, h), rng.standard_normal((2, h))
    cc, gZa, gZb = rng.standard_normal((N, 1)), rng.standard_normal((N, h)), rng.standard_normal((N, 4))
    tO, tl, tc = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (O, ln, cc))
    z = torch.cat([torch.relu(torch.nn.functional.layer_norm(tO, (h,), tl[0], tl[1], 1e-5)), tc, torch.zeros(N, 3, dtype=torch.float64)], dim=1)
    Za, Zb, _ = M.forward(O, ln, cc, h + 4)
    tol = 1e-6 if family == 'offset' else 1e-10           # (float64 itself loses 1000 / sigma of its digits to the offset)
    np.testing.assert_allclose(np.concatenate([Za, Zb], axis=1), z.detach().numpy(), rtol=tol, atol=tol)
    gO, gl, gc = torch.autograd.grad(z, [tO, tl, tc], torch.from_numpy(np.concatenate([gZa, gZb], axis=1)))
    mO, mc, mp = M.backward(gZa, gZb, O, ln)
    np.testing.assert_allclose(mO, gO.numpy(), rtol=tol, atol=tol * np.abs(gO.numpy()).max())
    np.testing.assert_allclose(mp, gl.numpy().reshape(-1), rtol=tol, atol=tol)
    np.testing.assert_array_equal(mc, gc.numpy()[:, 0])
    assert M.forward(O, ln, None, h + 4)[1].any() == False                      # noqa: E712  (concat None: zeros)


@pytest.mark.parametrize('h', M.HIDDEN)
def test_part_slabs_partition_the_rows(h):
    """Every valid row lands in exactly one slab, in the grid-stride order of k_head_bwd; the slabs sum to the model's psum."""
    lpn, R = h // 4, 256 // (h // 4)
    for N, nv in ((1, 1), (777, 777), (1100, 777), (70001, 70001)):
        nblk = M.bwd_blocks(N, h)
        assert nblk == min(-(-N // R), 512)
        rng = np.random.default_rng(N)
        O, ln, g = M.draw_rows(rng, 'randn', nv, h), rng.standard_normal((2, h)), rng.standard_normal((nv, h))
        slabs, mag, _, cnt = M.part_slabs(g, O, ln, nblk, lpn)
        np.testing.assert_allclose(slabs.sum(axis=0), M.backward(g, None, O, ln)[2], rtol=1e-10, atol=1e-10)
        owner = (np.arange(nv) // R) % nblk                   # node = b R + r + j nblk R
        ones = np.ones((nv, h))
        rows = M._by_block(ones, nblk, R).sum(axis=(0, 2))[:, 0]
        np.testing.assert_array_equal(rows, np.bincount(owner, minlength=nblk))
        assert cnt.max() == -(-nv // (nblk * R)) + 1 + M.log2i(64 // lpn) + 4
    assert -(-70001 // (512 * R)) >= 2                        # 70001 rows exceed one sweep of the 512-block grid at every LPN


# ------------------------------------------------------------------------------------------------------ the kink share
def test_no_case_leaves_more_than_a_thousandth_out_at_the_kink():
    for c in M.CASES:
        near = M.inputs(c)['near']
        assert near.mean() <= M.KINK_SHARE, (c['name'], int(near.sum()), near.size)
        if c['family'] == 'const':
            assert not near.any()             # (xhat = 0 exactly on both sides: pre = beta, nothing is left out)


def test_case_table_covers_what_the_gpu_file_promises():
    cs = M.CASES
    assert {(c['h'], c['N']) for c in cs} >= {(h, N) for h in M.HIDDEN for N in M.ROWS}
    for h in M.HIDDEN:
        mine = [c for c in cs if c['h'] == h]
        assert {c['family'] for c in mine} == set(M.FAMILIES)
        assert {c['view'] for c in mine} == {False, True} and any(c['cap'] for c in mine) and {c['concat'] for c in mine} == {False, True}
    assert any(c['single'] for c in cs)


# -------------------------------------------------------------------------------------------------------- the emulation
SMALL = [c['name'] for c in M.CASES if c['N'] <= 777]


@pytest.mark.parametrize('name', SMALL + ['h8-N70001-randn-view-exact-cat', 'h128-N70001-randn-view-exact-cat'])
def test_float32_emulation_within_one_bound(name):
    r = ratios(name)
    print(f'  {name}: ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert r['Zb'] == 0 and r['gconcat'] == 0


def test_float32_emulation_of_two_accumulated_launches_within_bound():
    for name in ('h8-N777-randn-dense-exact-cat', 'h128-N777-randn-dense-exact-cat'):
        assert ratios(name, second=True)['slabs'] <= 1.0


def test_constant_rows_are_exact():
    c = M.BY_NAME['h16-N37-const-view-exact-nocat']
    x = M.inputs(c)
    e = M.emulate(x['O'], x['ln'], None, c['hp'])
    assert np.array_equal(e['Za'], np.broadcast_to(np.maximum(x['ln'][1], 0), e['Za'].shape))


MUTATIONS = [
    ('eps 1e-6', 'h16-N777-small-view-exact-cat', dict(eps=1e-6), ('Za', 'gO'), False),
    ('variance / (h - 1)', 'h8-N777-randn-dense-exact-cat', dict(ddof=1), ('Za', 'gO'), False),
    ('mask without beta', 'h32-N777-randn-dense-exact-cat', dict(mask_no_beta=True), ('gO', 'slabs'), False),
    ('no xhat term', 'h64-N777-randn-dense-exact-cat', dict(no_xhat_term=True), ('gO',), False),
    ('capacity rows counted', 'h16-N777-randn-view-cap1100-nocat', dict(count_capacity=True), ('slabs',), False),
    ('ragged group dropped', 'h128-N777-randn-dense-exact-cat', dict(drop_ragged=True), ('slabs',), False),
    ('ragged group dropped', 'h8-N70001-randn-view-exact-cat', dict(drop_ragged=True), ('slabs',), False),
    ('accumulate overwrites', 'h8-N777-randn-dense-exact-cat', dict(overwrite=True), ('slabs',), True),
    ('gconcat from column 1', 'h16-N777-randn-dense-exact-cat', dict(gconcat_col=1), ('gconcat',), False),
]


@pytest.mark.parametrize('what,name,mut,outputs,second', MUTATIONS)
def test_mutations_are_ten_bounds_away(what, name, mut, outputs, second):
    assert name in M.BY_NAME
    r = ratios(name, second=second, **mut)
    print(f'  {what} on {name}: ' + ', '.join(f'{k} {r[k]:.3g}' for k in outputs))
    for k in outputs:
        assert r[k] >= 10.0, (what, k, r[k])
