"""Host checks of the float64 model of MHTransformerConv (tests/mh_f64.py) on its own: it equals the restatement of PyG's
TransformerConv (tests/mh_restated.py, heads = H, concat) followed by a float64 Linear(H C, C) for H = 1 .. 4; its float32 form passes
every checker; and every tampered float32 form -- one subtly wrong kernel each -- fails its checker.  No GPU, nothing of qtmpnn."""
import functools

import numpy as np
import pytest
import torch

import mh_f64 as M
from test_attn_f64_host import _random_symmetric_graph


@pytest.mark.parametrize('heads', [1, 2, 3, 4])
def test_model_equals_pyg_restatement_and_linear(heads):
    """keep = 1: y and the gradients of proj, We, Wt and blin equal mh_restated.TransformerConv(heads=H, concat=True, edge_dim=2)
    (its linears select the q / k / v / skip blocks of x = proj) followed by Linear(H C, C), in float64, to 1e-12 relative."""
    import mh_restated
    N, C, H = 37, 5, heads
    rowptr, col, eattr, selfpair = _random_symmetric_graph(N, 20 + heads)
    assert (selfpair > 0).any() and (selfpair == 0).any() and (np.diff(rowptr) > 0).all()
    rng = np.random.default_rng(7 + heads)
    proj, We = rng.standard_normal((N, H * 4 * C)), rng.standard_normal((H, C, 2))
    Wt, blin, g = rng.standard_normal((H * C, C)), rng.standard_normal(C), rng.standard_normal((N, C))
    ref = M.model(rowptr, col, selfpair, eattr, proj, We, Wt, blin, C, H, 1.0, 0, 0)
    gr = M.gradients(ref, g)

    conv = mh_restated.TransformerConv(H * 4 * C, C, heads=H, concat=True, edge_dim=2).double()
    lin = torch.nn.Linear(H * C, C).double()
    P = np.arange(H * 4 * C).reshape(H, 4, C)
    with torch.no_grad():
        for sel, blk in ((conv.lin_query, 0), (conv.lin_key, 1), (conv.lin_value, 2), (conv.lin_skip, 3)):
            sel.weight.zero_()
            sel.bias.zero_()
            sel.weight[torch.arange(H * C), torch.from_numpy(P[:, blk].reshape(-1))] = 1.0
        conv.lin_edge.weight.copy_(torch.from_numpy(We.reshape(H * C, 2)))
        lin.weight.copy_(torch.from_numpy(Wt.T))
        lin.bias.copy_(torch.from_numpy(blin))
    own = np.nonzero(selfpair > 0)[0]
    tgt = np.concatenate([np.repeat(np.arange(N), np.diff(rowptr)), own])
    src = np.concatenate([col, own])
    ea = np.concatenate([eattr, np.zeros((len(own), 2))])
    perm = np.random.default_rng(5).permutation(len(tgt))
    x = torch.from_numpy(proj).requires_grad_(True)
    cat = conv(x, torch.from_numpy(np.stack([src, tgt])[:, perm]), torch.from_numpy(ea[perm]))
    y = lin(cat)
    gx, gwe, gwl, gbl, gc = torch.autograd.grad(y, [x, conv.lin_edge.weight, lin.weight, lin.bias, cat], torch.from_numpy(g))

    def same(a, b, what):
        a, b = a.detach().numpy(), b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (what, np.abs(a - b).max(), np.abs(b).max())
    same(ref.cat, cat, 'cat')
    same(ref.y, y, 'y')
    same(gr.proj, gx, 'd proj')
    same(gr.We.reshape(H * C, 2), gwe, 'd We')
    same(gr.Wt, gwl.T, 'd Wt')
    same(gr.blin, gbl, 'd blin')
    same(gr.gcat, gc, 'gcat')
    assert all(float(gr.proj.view(N, H, 4, C)[:, h, b].abs().max()) > 0 for b in range(4) for h in range(H))
    # the majorants dominate what they bound, and the coefficients sum to one per target and head
    assert bool((ref.y.detach().abs() <= ref.ybound * (1 + 1e-12)).all()) and bool((gr.gcat.abs() <= gr.gcat_bound * (1 + 1e-12)).all())
    assert bool((ref.s.abs() <= ref.smaj * (1 + 1e-12)).all())
    rev = _rev(rowptr, col)
    ae, as_ = M.coefficients(ref, rev)
    total = np.zeros((H, N))
    np.add.at(total, (slice(None), col), ae)                  # alpha_e follows the CSR order of the pairs (src = row, dst = col)
    np.testing.assert_allclose(total + as_, 1.0, rtol=0, atol=1e-12)
    assert not as_[:, selfpair == 0].any() and (as_[:, selfpair > 0] > 0).all()


def _rev(rowptr, col):
    """Position of every stored edge's transpose in a CSR whose rows are sorted by column."""
    N = len(rowptr) - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    key = row * N + col.astype(np.int64)
    assert (np.diff(key) > 0).all()
    rev = np.searchsorted(key, col.astype(np.int64) * N + row)
    assert np.array_equal(key[rev], col.astype(np.int64) * N + row)
    return rev


def _grid_graph(n, m, seed):
    """CSR of the 4-neighbour n x m grid, rows sorted by column; attr(j -> i) = [angle + 1/2 mod 1, dist] of attr(i -> j); self
    pairs on about half of the nodes."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n * m, dtype=np.int64).reshape(n, m)
    a = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel()])
    b = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel()])
    ang, dist = rng.random(len(a)), 0.25 + 3 * rng.random(len(a))
    tgt, src = np.concatenate([a, b]), np.concatenate([b, a])
    attr = np.stack([np.concatenate([ang, (ang + 0.5) % 1.0]), np.concatenate([dist, dist])], axis=1)
    order = np.argsort(tgt * (n * m) + src)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n * m))]).astype(np.int32)
    return rowptr, src[order].astype(np.int32), attr[order], (rng.random(n * m) < 0.5).astype(np.float32)


# One case for the clean form and every tamper: H = 3, C = 8, keep = 0.5, more rows than one sweep of the merge backward's grid.
H, C, KEEP, SEED, EPOCH = 3, 8, 0.5, 0xDEADBEEF, 5


@functools.lru_cache(maxsize=None)
def _big():
    rowptr, col, eattr, selfpair = _grid_graph(92, 91, 3)
    N = len(rowptr) - 1
    assert N > M.SWEEP and (selfpair > 0).any() and (selfpair == 0).any()
    graph = (rowptr, col, selfpair, eattr)
    ops = M.operands(N, C, C, H, 77)
    ref = M.model(*graph, ops.proj, ops.We, ops.Wt, ops.blin, C, H, KEEP, SEED, EPOCH)
    return graph, ops, ref, _rev(rowptr, col)


def _outputs(tamper=None):
    graph, ops, _, rev = _big()
    return M.float32_outputs(graph, ops, C, H, KEEP, SEED, EPOCH, rev, tamper)


def test_clean_float32_form_passes_every_bound():
    graph, ops, ref, rev = _big()
    M.check_all('host clean', ref, ops.g, rev, graph[2], _outputs())


@pytest.mark.parametrize('heads', [1, 2, 3, 4])
@pytest.mark.parametrize('width,c_real', [(4, 1), (8, 5), (16, 16), (32, 32)])
def test_clean_float32_form_passes_at_every_head_count_and_width(heads, width, c_real):
    rowptr, col, eattr, selfpair = _random_symmetric_graph(201, heads + width)
    graph = (rowptr, col, selfpair, eattr)
    ops = M.operands(201, width, c_real, heads, heads * 100 + width)
    ref = M.model(*graph, ops.proj, ops.We, ops.Wt, ops.blin, c_real, heads, 0.9, 1234, 1)
    rev = _rev(rowptr, col)
    M.check_all(f'host H={heads} C={width}', ref, ops.g, rev, selfpair, M.float32_outputs(graph, ops, c_real, heads, 0.9, 1234, 1, rev))


# tamper -> (the checker that must fail, the outputs it reads)
CAUGHT_BY = {
    'wt_blocks_swapped': 'forward',
    'head1_draws_head0_seed': 'forward',
    'blin_per_head_group': 'forward',
    'rows_past_sweep_dropped': 'merge_grads',
    'lsum_from_head0': 'stats',
    'alpha_at_e': 'alpha',
}


def _run(checker, out):
    graph, ops, ref, rev = _big()
    gr = M.gradients(ref, ops.g)
    if checker == 'forward':
        M.check_forward('host', ref, out['y'], out['cat'])
    elif checker == 'merge_grads':
        M.check_merge_grads('host', gr, out['dWt'], out['dblin'])
    elif checker == 'stats':
        M.check_stats('host', ref, out['stats'])
    elif checker == 'alpha':
        M.check_alpha('host', ref, rev, graph[2], out['alpha_e'], out['alpha_s'])
    else:
        raise KeyError(checker)


def test_every_tamper_has_a_checker():
    assert set(CAUGHT_BY) == set(M.TAMPERS)


@pytest.mark.parametrize('tamper', M.TAMPERS)
def test_tampered_float32_form_fails_its_checker(tamper):
    """Each wrong kernel fails the checker that reads what it spoils (and so check_all); the clean form passes the same checker."""
    graph, ops, ref, rev = _big()
    _run(CAUGHT_BY[tamper], _outputs())
    bad = _outputs(tamper)
    with pytest.raises(AssertionError):
        _run(CAUGHT_BY[tamper], bad)
    with pytest.raises(AssertionError):
        M.check_all('host ' + tamper, ref, ops.g, rev, graph[2], bad)


def test_head_seed_tamper_changes_only_head_one():
    """The one-head restatement of a head's mask (seed + h 0x632BE5AB as a one-head launch's seed) reproduces the H-head model for the
    heads that keep their seed: the tampered cat differs from the clean one in head 1's columns only."""
    clean, bad = _outputs()['cat'], _outputs('head1_draws_head0_seed')['cat']
    same = (clean == bad).view(-1, H, C).all(dim=0).all(dim=1)
    assert same.tolist() == [True, False, True]


def test_case_table_covers_what_the_gpu_file_promises():
    assert {(c['H'], c['C']) for c in M.APPLY_HEADS} == {(h, c) for h in M.HEADS for c in M.WIDTHS}
    assert all(c['kind'] == 'D' and c['keep'] == 1.0 for c in M.APPLY_HEADS)
    assert {(c['C'], c['c_real']) for c in M.APPLY_CREAL} == {(4, 1), (8, 5)}
    assert {(c['kind'], c['C'], c['H']) for c in M.APPLY_MESHES} == {(k, c, h) for k in 'SPTL' for c, h in ((16, 3), (32, 4))}
    assert {(c['kind'], c['keep'], c['epoch'], c['seed']) for c in M.APPLY_DROPOUT} == {(k, *d) for k in 'DT' for d in M.DROPOUT}
    assert all(c['C'] == 16 and c['H'] == 3 for c in M.APPLY_DROPOUT)
    assert set(M.RAW) == {(k, c, h) for k in 'DTL' for c in (8, 32) for h in (3, 4)}
    assert set(M.WEIGHTS) == {('D', 4), ('D', 8), ('D', 16), ('D', 32), ('S', 16), ('P', 16), ('T', 16)}
    names = [c['name'] for c in M.APPLY_HEADS + M.APPLY_CREAL + M.APPLY_MESHES + M.APPLY_DROPOUT]
    assert len(set(names)) == len(names)
    assert M.SWEEP == 8192
