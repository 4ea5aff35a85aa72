"""Host checks of the float64 model of the LSTM cell (tests/cell_f64.py) on its own: it agrees with float64 torch autograd of the
oracle's cell arithmetic (oracle/qt_oracle.py GConvLSTM.forward's closing statements + layer_norm), the backward from stored gates
included; a float32 emulation of the kernels' arithmetic stays within every bound on the cases of tests/test_gpu_cell_f64.py, with
v_exp_f32 / v_rcp_f32 pushed by +-1 ulp in all four combinations; single mutations of that emulation exceed the bound on a named
case of that file; the restated row ownership of the three backward launches partitions the valid rows.  No GPU, nothing of qtmpnn.

Mutation -> the GPU case (cell_f64.BY_NAME) whose comparison sees it:
  LN eps 1e-6                              h8-N777-live-nog2-c-ln-go-gcn-dense-exact                Hn, Cn
  output-gate peephole reads C             h16-N777-live-nog2-c-ln-go-gcn-dense-exact               Og
  gc_ without ggo w_co                     h32-N777-live-nog2-c-ln-go-gcn-dense-exact               gG
  1 - tc instead of 1 - tc^2               h64-N777-live-nog2-c-ln-go-gcn-dense-exact               gG
  gcp without ggf w_cf                     h128-N777-live-nog2-c-ln-go-gcn-dense-exact              gCprev
  G2 ignored                               h8-N37-live-g2-c-ln-go-gcn-view-cap107                   I
  tanh series without x^5                  h8-N83-branch-nog2-c-ln-go-gcn-dense-cap120              T
  tanh threshold 0.5                       h16-N777-live-nog2-c-ln-go-gcn-dense-exact               T
  sums drop the last ragged group          h128-N777-live-nog2-c-ln-go-gcn-dense-exact, h8-N65573-live-nog2-c-ln-go-gcn-view-exact   part
  sums count capacity rows                 h16-N37-live-g2-c-ln-go-gcn-view-cap107                  part (NaN rows reach them)
  accumulate overwrites                    h8-N777-live-nog2-c-ln-go-gcn-dense-exact                part over a prefill
"""
import numpy as np
import pytest
import torch

import cell_f64 as M
from test_head_f64_host import worst

PREFILL = 3.0
_X = {}


def inputs(c):
    if c['name'] not in _X:
        _X.clear()
        _X[c['name']] = M.inputs(c)
    return _X[c['name']]


def _pad(a, cap):
    if a is None or a.shape[0] >= cap:
        return a
    return np.concatenate([a, np.full((cap - a.shape[0], a.shape[1]), np.nan, np.float32)])


def ratios(case, push=(0, 0), launch=None, accumulate=False, forward=True, **mut):
    """Worst error / bound per output of the (mutated) emulation against the model on a case of the GPU file."""
    c = M.BY_NAME[case] if isinstance(case, str) else case
    x = inputs(c)
    h, N, cap = c['h'], c['N'], c['cap'] or c['N']
    out = {}
    fmut = {k: v for k, v in mut.items() if k in ('eps', 'o_reads_c', 'no_g2', 'no_x5', 'thr')}
    bmut = {k: v for k, v in mut.items() if k not in ('o_reads_c', 'no_g2')}
    fa = (x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'])
    if forward:
        m, fb = M.forward(*fa), M.forward_bounds(*fa)
        e = M.emulate_forward(*fa, push=push, **fmut)
        out.update({k: worst(e[k], m[k], fb[k]) for k in e})
    ba = (x['gates'], x['Cprev'], x['gO'], x['gHn'], x['gCn'], x['wc'], x['ln'])
    gG, gcp, terms = M.backward_terms(*ba)
    bb = M.backward_bounds(*ba)
    launch = launch or M.launch_bwd(cap, h)
    part, pb = M.part_rows(terms, bb['e_terms'], launch, N, h // 4)
    prev = None
    if accumulate:
        prev = np.full(part.shape, PREFILL, np.float32)
        part = PREFILL + part                             # (a workgroup that writes nothing owns no row: prefill + 0)
        pb = pb + 2.0 * M.U * np.abs(part)
    padded = [_pad(a, cap) for a in ba[:5]]
    e = M.emulate_backward(*padded, x['wc'], x['ln'], launch=launch, n_valid=N, prev=prev, push=push, **bmut)
    out.update(gG=worst(e['gG'], gG, bb['gG']), gCprev=worst(e['gCprev'], gcp, bb['gCprev']), part=worst(e['part'], part, pb))
    return out


# -------------------------------------------------------------------------------------------------- model against autograd
def _torch_cell(G, G2, C, wc, b, ln):
    """oracle/qt_oracle.py GConvLSTM.forward from the gate sums on, + the LayerNorms of H' and C'."""
    h = C.shape[1]
    g = G if G2 is None else G + G2
    q = lambda k: g[:, k * h:(k + 1) * h]
    I = torch.sigmoid(q(0) + wc[0] * C + b[0])
    Fg = torch.sigmoid(q(1) + wc[1] * C + b[1])
    T = torch.tanh(q(2) + b[2])
    Cn = Fg * C + I * T
    O = torch.sigmoid(q(3) + wc[2] * Cn + b[3])
    Hn = O * torch.tanh(Cn)
    gates = torch.cat([I, Fg, T, O], dim=1)
    if ln is not None:
        lnf = torch.nn.functional.layer_norm
        Hn, Cn = lnf(Hn, (h,), ln[0], ln[1], 1e-5), lnf(Cn, (h,), ln[2], ln[3], 1e-5)
    return O, Hn, Cn, gates


@pytest.mark.parametrize('h,N,g2,cprev,ln,go', [(8, 5, True, True, True, True), (16, 33, False, True, False, True),
                                                 (64, 9, True, False, True, False), (128, 3, False, True, True, True)])
def test_model_equals_float64_autograd(h, N, g2, cprev, ln, go):
    rng = np.random.default_rng(h + N)
    r = lambda *s: rng.standard_normal(s)
    G, G2, C, wc, b, lnp = r(N, 4 * h), (r(N, 4 * h) if g2 else None), r(N, h), r(3, h), r(4, h), (r(4, h) if ln else None)
    gO, gHn, gCn = (r(N, h) if go else None), r(N, h), r(N, h)
    leaf = lambda a: None if a is None else torch.from_numpy(a).requires_grad_(True)
    tG, tG2, tC, twc, tb, tln = (leaf(a) for a in (G, G2, C, wc, b, lnp))
    if not cprev:
        tC = torch.zeros(N, h, dtype=torch.float64, requires_grad=True)
    O, Hn, Cn, gates = _torch_cell(tG, tG2, tC, twc, tb, tln)
    m = M.forward(G, G2, C if cprev else None, wc, b, lnp)
    for k, t in (('Og', O), ('Hn', Hn), ('Cn', Cn), ('I', gates[:, :h]), ('F', gates[:, h:2 * h]), ('T', gates[:, 2 * h:3 * h])):
        np.testing.assert_allclose(m[k], t.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg=k)
    loss = (Hn * torch.from_numpy(gHn)).sum() + (Cn * torch.from_numpy(gCn)).sum()
    if go:
        loss = loss + (O * torch.from_numpy(gO)).sum()
    wrt = [tG, tC, twc, tb] + ([tln] if ln else [])
    gs = [g.numpy() for g in torch.autograd.grad(loss, wrt)]
    # the backward from the stored gates, here the float64 gates themselves
    gG, gcp, psum = M.backward(gates.detach().numpy(), C if cprev else None, gO, gHn, gCn, wc, lnp)
    tol = dict(rtol=1e-12, atol=1e-12 * max(1.0, np.abs(gs[0]).max()))
    np.testing.assert_allclose(gG, gs[0], **tol)
    np.testing.assert_allclose(gcp, gs[1], **tol)
    np.testing.assert_allclose(psum[:3 * h], gs[2].reshape(-1), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(psum[3 * h:7 * h], gs[3].reshape(-1), rtol=1e-11, atol=1e-11)
    if ln:
        np.testing.assert_allclose(psum[7 * h:], gs[4].reshape(-1), rtol=1e-11, atol=1e-11)
    else:
        assert not psum[[7 * h + j for j in range(h)] + [9 * h + j for j in range(h)]].any()      # (xhat = 0 without a LayerNorm)
    # a second gradient of H' is added on load
    g2n = r(N, h)
    a = M.backward(gates.detach().numpy(), C, gO, gHn, gCn, wc, lnp, gHn2=g2n)
    bsum = M.backward(gates.detach().numpy(), C, gO, gHn + g2n, gCn, wc, lnp)
    for u, v in zip(a, bsum):
        np.testing.assert_allclose(u, v, rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------------------ ownership
@pytest.mark.parametrize('h', M.HIDDEN)
def test_lstm_bwd_ownership_partitions_the_rows(h):
    lpn, R = h // 4, 256 // (h // 4)
    for cap, n in ((1, 1), (777, 777), (1100, 777), (M.SWEEP2[h], M.SWEEP2[h])):
        L = M.launch_bwd(cap, h)
        assert L['nblk'] == min(-(-cap // R), 512)
        idx = M.row_index(L, n, lpn)
        assert np.array_equal(np.sort(idx[idx < n]), np.arange(n))
        t = np.random.default_rng(n).standard_normal((n, 3))
        np.testing.assert_allclose(M.owned(t, L, n, lpn).sum(axis=(0, 1, 2)), t.sum(axis=0), rtol=1e-10, atol=1e-10)
        assert np.array_equal(M.owned(t, L, n, lpn), np.concatenate([t, np.zeros((1, 3))])[idx])      # _by_block IS row_index
    assert M.row_index(M.launch_bwd(M.SWEEP2[h], h), M.SWEEP2[h], lpn).shape[0] == 2                # a second, ragged sweep
    assert (M.SWEEP2[h] - 512 * R) % R == 37 % R and 37 % R != 0


@pytest.mark.parametrize('h', [8, 16])
def test_dgrad_ownership_partitions_the_rows(h):
    lpn = h // 4
    for n in M.DGRAD_ROWS_CASES + (128, 256):
        L = M.launch_dgrad(n + 70, h)
        idx = M.row_index(L, n, lpn)
        assert idx.shape == (128 // (256 // lpn), -(-(n + 70) // 128), 256 // lpn)
        assert np.array_equal(np.sort(idx[idx < n]), np.arange(n))
        own = np.where(idx < n, idx // 128, -1)
        assert all(set(np.unique(own[:, b])) <= {-1, b} for b in range(L['nblk']))                  # rows [128 b, 128 b + 128)
        assert np.array_equal(M.written(L, n), np.arange(L['nblk']) * 128 < n)
        assert (M.part_count(L, n, lpn)[M.written(L, n)] <= 128 // (256 // lpn) + 1 + M.log2i(64 // lpn) + 4).all()


@pytest.mark.parametrize('n_cu', [1, 2, 3, 256])
@pytest.mark.parametrize('nt', [1, 2, 3, 4])
@pytest.mark.parametrize('h', [8, 16])
def test_fused_ownership_partitions_the_rows(h, nt, n_cu):
    lpn = h // 4
    for n in M.FUSED_ROWS_CASES + (64, 128, 1000):
        L = M.launch_fused(n + 70, h, nt, n_cu)
        tr = L['tr']
        assert L['nblk'] == (min(2 * n_cu, -(-(n + 70) // 64)) if nt <= 3 else min(n_cu, -(-(n + 70) // 128))) and L['nw'] == tr // 16
        idx = M.row_index(L, n, lpn)
        assert np.array_equal(np.sort(idx[idx < n]), np.arange(n))
        assert (idx[:, :, tr:] == n).all()                    # threads past TR LPN hold no node
        t = np.random.default_rng(n).standard_normal((n, 3))
        np.testing.assert_allclose(M.owned(t, L, n, lpn).sum(axis=(0, 1, 2)), t.sum(axis=0), rtol=1e-10, atol=1e-10)
        A, gG = np.random.default_rng(n + 1).standard_normal((n, 16)), np.random.default_rng(n + 2).standard_normal((n, 4 * h))
        sl, _ = M.wslab(A, gG, 0.0 * gG, L, n)
        np.testing.assert_allclose(sl.sum(axis=0), A.T @ gG, rtol=1e-10, atol=1e-10)


# -------------------------------------------------------------------------------------------------------- the cases
def test_case_table_covers_what_the_gpu_file_promises():
    cs = M.CASES
    assert {(c['h'], c['N']) for c in cs} >= {(h, N) for h in M.HIDDEN for N in (1, 37, 777, M.SWEEP2[h])}
    assert M.SWEEP2[128] == 4133 and M.SWEEP2[8] == 65573
    for h in M.HIDDEN:
        mine = [c for c in cs if c['h'] == h]
        for key in ('g2', 'cprev', 'ln', 'go', 'gcn', 'view'):
            assert {c[key] for c in mine} == {False, True}, (h, key)
        assert any(c['cap'] for c in mine)
    for h in (8, 32, 128):
        assert {c['kind'] for c in cs if c['h'] == h} == set(M.KINDS)
    assert M.branch_grid().size == 164 and len(set(M.branch_grid().tolist())) == 163          # (+0 and -0 compare equal)


@pytest.mark.parametrize('name', [c['name'] for c in M.CASES if c['kind'] == 'live'])
def test_live_cases_are_live(name):
    M.assert_live(M.BY_NAME[name], inputs(M.BY_NAME[name]))


def test_branch_case_sits_on_both_sides_of_the_threshold():
    for c in (c for c in M.CASES if c['kind'] == 'branch'):
        x = inputs(c)
        m = M.forward(x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'])
        h = c['h']
        assert set(np.abs(m['pre'][2]).reshape(-1).tolist()) == set(np.abs(M.branch_grid()).tolist())
        cr = np.abs(m['Cr'][:, :h // 2])
        near = np.abs(cr - M.THR) < 1e-5
        assert near.mean() > 0.9 and (cr[near] < M.THR).any() and (cr[near] >= M.THR).any()
        e = M.emulate_forward(x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'])
        cr32 = np.abs(M._fma(e['F'], x['Cprev'], e['I'] * e['T'])[:, :h // 2])
        assert (cr32 < np.float32(M.THR)).mean() > 0.1 and (cr32 >= np.float32(M.THR)).mean() > 0.1


def test_saturated_and_constant_rows():
    """Saturated rows: every output finite, gates in [0, 1] / [-1, 1], exp2's overflow gives 0 and not NaN.  Constant rows: xhat = 0
    exactly, H' = beta_h and C' = beta_c bit for bit."""
    for c in M.CASES:
        x = inputs(c) if c['kind'] in ('sat', 'const') else None
        if x is None:
            continue
        for push in M.PUSHES:
            e = M.emulate_forward(x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'], push)
            assert all(np.isfinite(v).all() for v in e.values())
            assert all(((e[k] >= 0) & (e[k] <= 1)).all() for k in ('I', 'F', 'Og')) and (np.abs(e['T']) <= 1).all()
            if c['kind'] == 'const':
                assert np.array_equal(e['Hn'], np.broadcast_to(x['ln'][1], e['Hn'].shape))
                assert np.array_equal(e['Cn'], np.broadcast_to(x['ln'][3], e['Cn'].shape))
        if c['kind'] == 'sat':
            assert ((x['gates'] == 0) | (np.abs(x['gates']) == 1)).mean() > 0.4


# -------------------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize('name', [c['name'] for c in M.CASES])
def test_float32_emulation_within_one_bound(name):
    w = {}
    for push in M.PUSHES:
        r = ratios(name, push)
        w = {k: max(v, w.get(k, 0.0)) for k, v in r.items()}
    print(f'  {name}: ' + ', '.join(f'{k} {v:.3g}' for k, v in w.items()))
    assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize('h', [8, 16])
def test_float32_emulation_of_the_fused_launches_within_one_bound(h):
    name = f'h{h}-N777-live-nog2-c-ln-go-gcn-dense-exact'
    cap = 777
    for launch in (M.launch_dgrad(cap, h), M.launch_fused(cap, h, 2, 256), M.launch_fused(cap, h, 4, 2)):
        for acc in (False, True):
            r = ratios(name, launch=launch, accumulate=acc, forward=False)
            print(f'  {name} {launch}: part {r["part"]:.3g}')
            assert r['part'] <= 1.0, (launch, r)


def test_float32_emulation_of_an_accumulating_launch_within_bound():
    for name in ('h8-N777-live-nog2-c-ln-go-gcn-dense-exact', 'h128-N777-live-nog2-c-ln-go-gcn-dense-exact'):
        assert ratios(name, accumulate=True, forward=False)['part'] <= 1.0


LIVE = 'h{}-N777-live-nog2-c-ln-go-gcn-dense-exact'
MUTATIONS = [
    ('LN eps 1e-6', LIVE.format(8), dict(eps=1e-6), ('Hn', 'Cn'), False),
    ('output-gate peephole reads C', LIVE.format(16), dict(o_reads_c=True), ('Og',), False),
    ('gc_ without ggo w_co', LIVE.format(32), dict(no_wco=True), ('gG',), False),
    ('1 - tc', LIVE.format(64), dict(tc_lin=True), ('gG',), False),
    ('gcp without ggf w_cf', LIVE.format(128), dict(no_wcf=True), ('gCprev',), False),
    ('G2 ignored', 'h8-N37-live-g2-c-ln-go-gcn-view-cap107', dict(no_g2=True), ('I',), False),
    ('tanh without x^5', 'h8-N83-branch-nog2-c-ln-go-gcn-dense-cap120', dict(no_x5=True), ('T',), False),
    ('tanh threshold 0.5', LIVE.format(16), dict(thr=0.5), ('T',), False),
    ('ragged group dropped', LIVE.format(128), dict(drop_ragged=True), ('part',), False),
    ('ragged group dropped', 'h8-N65573-live-nog2-c-ln-go-gcn-view-exact', dict(drop_ragged=True), ('part',), False),
    ('capacity rows counted', 'h16-N37-live-g2-c-ln-go-gcn-view-cap107', dict(count_capacity=True), ('part',), False),
    ('accumulate overwrites', LIVE.format(8), dict(overwrite=True), ('part',), True),
]


@pytest.mark.parametrize('what,name,mut,outputs,acc', MUTATIONS)
def test_mutations_exceed_the_bound(what, name, mut, outputs, acc):
    assert name in M.BY_NAME
    r = ratios(name, accumulate=acc, **mut)
    print(f'  {what} on {name}: ' + ', '.join(f'{k} {r[k]:.3g}' for k in outputs))
    for k in outputs:
        assert r[k] > 1.0, (what, k, r[k])
