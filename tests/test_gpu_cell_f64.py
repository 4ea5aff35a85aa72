"""The LSTM cell kernels -- qt_lstm_fwd / qt_lstm_infer (k_lstm_fwd<LPN>, LPN = 2 .. 32), qt_lstm_bwd (k_lstm_bwd<LPN>) and the
parameter sums of qt_lstm_bwd_dgrad (k_dgrad_cell) and qt_lstm_bwd_fused (k_cell_bwd_fused, with its weight-gradient slab) --
through the C ABI against the float64 model tests/cell_f64.py.

Every comparison is kernel against model.  The bounds are derived beside the model (twice a count of float32 roundings times 2^-24
times the majorant, propagated at first order through the gates and the LayerNorm; the nonlinearities' own error from the
v_exp_f32 / v_rcp_f32 instruction sequence, as an absolute error); no entry of any case is left out.  Outputs are pre-filled with
the sentinel -7.25, `part` with NaN where the launch must overwrite it and with 3.0 where it must add; capacity rows of the inputs
are NaN and must keep the sentinel in every output.  Operands also come as column views of wider matrices whose other columns are
NaN (ld_g > 4h, ld_c > h, strided gO / gHn / gCn).  The backward reads the STORED gate activations: the model's, rounded to float32.
gG, gCprev and the data-gradient planes of the two fused launches stay with tests/test_gpu_gate_cell_bits.py (bit for bit against
qt_lstm_bwd, which this file holds to the model); the tiled CELL epilogue of k_gemm_fwd is tied to qt_dense -> qt_lstm_fwd there
too.  Every case prints its worst error / bound before it asserts (pytest -s; a recorded run: profiles/cell_f64.txt).
tests/test_cell_f64_host.py names, per mutation, the case here that sees it."""
import numpy as np
import pytest
import torch

import cell_f64 as M
from helpers import dev
from test_gpu_cheb_f64 import compare

pytestmark = pytest.mark.gpu

SENT = -7.25
PREFILL = 3.0
WORST = {}
_X = {}


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
    _lib.call(name, *args)


def p(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def filled(*shape, value=SENT):
    return torch.full(shape, value, device=dev())


def inputs(c):
    if c['name'] not in _X:
        _X.clear()
        _X[c['name']] = M.inputs(c)
    return _X[c['name']]


def operand(a, cap, view):
    """(tensor that owns the storage, offset in floats, row stride) of the (N, w) operand: rows up to cap are NaN; as a view it is
    the columns [4, 4 + w) of a (cap, w + 8) matrix of NaN.  None stays None (stride w is passed by the caller)."""
    if a is None:
        return None, 0, 0
    N, w = a.shape
    wide = np.full((cap, w + 8 if view else w), np.nan, np.float32)
    wide[:N, 4 * view:4 * view + w] = a
    return _t(wide), 4 * view, wide.shape[1]


def n_dev(c):
    return torch.tensor([c['N']], dtype=torch.int32, device=dev()) if c['cap'] else None


def lstm_fwd(c, x, entry='qt_lstm_fwd'):
    h, cap = c['h'], c['cap'] or c['N']
    G, og, ldg = operand(x['G'], cap, c['view'])
    G2, _, _ = operand(x['G2'], cap, c['view'])
    Cp, oc, ldc = operand(x['Cprev'], cap, c['view'])
    wc, b, ln = _t(x['wc']), _t(x['b']), (None if x['ln'] is None else _t(x['ln']))
    O, Hn, Cn, gates = filled(cap, h), filled(cap, h), filled(cap, h), filled(cap, 4 * h)
    nd = n_dev(c)
    args = [p(G, og), p(G2, og), ldg, p(Cp, oc), ldc or h, p(wc), p(b), p(ln), cap, p(nd), h, p(O), p(Hn), p(Cn)]
    call(entry, *(args + ([p(gates)] if entry == 'qt_lstm_fwd' else [])))
    torch.cuda.synchronize()
    return dict(O=_np(O), Hn=_np(Hn), Cn=_np(Cn), gates=_np(gates))


def bwd_operands(c, x, cap, gHn2=False):
    """The device operands of a backward launch: [(pointer, stride) of gO, gHn, gCn], gates, (Cprev, ld_c), wc, ln, keep-alive list."""
    h = c['h']
    keep, out = [], []
    for key in ('gO', 'gHn', 'gCn', 'Cprev') + (('gHn2',) if gHn2 else ()):
        t, o, ld = operand(x[key], cap, c['view'])
        keep.append(t)
        out.append((p(t, o), ld or h))
    gates, wc, ln = operand(x['gates'], cap, False)[0], _t(x['wc']), (None if x['ln'] is None else _t(x['ln']))
    return out, gates, wc, ln, keep


def model_bwd(x, gHn2=False):
    ba = (x['gates'], x['Cprev'], x['gO'], x['gHn'], x['gCn'], x['wc'], x['ln'], x['gHn2'] if gHn2 else None)
    gG, gcp, terms = M.backward_terms(*ba)
    return gG, gcp, terms, M.backward_bounds(*ba)


# ------------------------------------------------------------------------------------------- 1. qt_lstm_fwd / qt_lstm_infer
@pytest.mark.parametrize('name', [c['name'] for c in M.CASES])
def test_lstm_fwd(name):
    c = M.BY_NAME[name]
    x = inputs(c)
    N, h, kind = c['N'], c['h'], c['kind']
    fa = (x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'])
    m, fb = M.forward(*fa), M.forward_bounds(*fa)
    o = lstm_fwd(c, x)
    for k, key in enumerate(('I', 'F', 'T', 'Og')):
        check(f'fwd {kind} gates', f'{name} {key}', o['gates'][:N, k * h:(k + 1) * h], m[key], fb[key])
    check(f'fwd {kind} O', name, o['O'][:N], m['Og'], fb['Og'])
    check(f'fwd {kind} Hn', name, o['Hn'][:N], m['Hn'], fb['Hn'])
    check(f'fwd {kind} Cn', name, o['Cn'][:N], m['Cn'], fb['Cn'])
    assert np.array_equal(o['O'][:N], o['gates'][:N, 3 * h:]), f'{name}: O is not the stored output gate'
    g = o['gates'][:N]
    assert ((g[:, :2 * h] >= 0) & (g[:, :2 * h] <= 1)).all() and (np.abs(g[:, 2 * h:3 * h]) <= 1).all() and ((g[:, 3 * h:] >= 0) & (g[:, 3 * h:] <= 1)).all()
    for key in ('O', 'Hn', 'Cn', 'gates'):
        assert (o[key][N:] == SENT).all(), f'{name}: a capacity row of {key} was written'
    if kind == 'const':                                   # xhat = 0 exactly: H' = beta_h, C' = beta_c bit for bit
        assert np.array_equal(o['Hn'][:N], np.broadcast_to(x['ln'][1], (N, h))) and np.array_equal(o['Cn'][:N], np.broadcast_to(x['ln'][3], (N, h)))
    i = lstm_fwd(c, x, 'qt_lstm_infer')
    for key in ('O', 'Hn', 'Cn'):
        assert np.array_equal(i[key], o[key]), f'{name}: qt_lstm_infer differs from qt_lstm_fwd in {key}'
    assert (i['gates'] == SENT).all()


# ------------------------------------------------------------------------------------------------------- 2. qt_lstm_bwd
@pytest.mark.parametrize('name', [c['name'] for c in M.CASES])
def test_lstm_bwd(name):
    """gG, gCprev and every part row, workgroup by workgroup: accumulate = 0 over NaN leaves no NaN, accumulate = 1 over 3.0 adds."""
    from qtmpnn import _lib
    c = M.BY_NAME[name]
    x = inputs(c)
    N, h, kind, cap = c['N'], c['h'], c['kind'], c['cap'] or c['N']
    (go, ghn, gcn, cp), gates, wc, ln, keep = bwd_operands(c, x, cap)
    L = M.launch_bwd(cap, h)
    assert _lib.value('qt_lstm_bwd_blocks', cap, h) == L['nblk']
    gG, gcp, terms, bb = model_bwd(x)
    part, pb = M.part_rows(terms, bb['e_terms'], L, N, h // 4)
    nd = n_dev(c)
    for accumulate in (0, 1):
        dG, dCp = filled(cap, 4 * h), filled(cap, h)
        dpart = filled(L['nblk'], 11 * h, value=PREFILL if accumulate else float('nan'))
        call('qt_lstm_bwd', go[0], go[1], ghn[0], ghn[1], gcn[0], gcn[1], p(gates), cp[0], cp[1], p(wc), p(ln), cap, p(nd), h,
             p(dG), p(dCp), p(dpart), accumulate)
        torch.cuda.synchronize()
        dG, dCp = _np(dG), _np(dCp)
        check(f'bwd {kind} gG', f'{name} acc={accumulate}', dG[:N], gG, bb['gG'])
        check(f'bwd {kind} gCprev', f'{name} acc={accumulate}', dCp[:N], gcp, bb['gCprev'])
        assert (dG[N:] == SENT).all() and (dCp[N:] == SENT).all(), f'{name}: a capacity row of gG / gCprev was written'
        if accumulate:
            check(f'part {kind} accumulate', name, dpart, PREFILL + part, pb + 2.0 * M.U * np.abs(PREFILL + part))
        else:
            check(f'part {kind}', name, dpart, part, pb)


# ------------------------------------------------------------------------------------- 3. the fused launches' parameter sums
CB, CBB = 16, 16


def _fused_case(h, rows):
    c = M._case(h, rows, cap=rows + 70, view=rows % 2 == 1 and rows > 1, seed=5)
    return c, inputs(c)


@pytest.mark.parametrize('rows', M.DGRAD_ROWS_CASES)
@pytest.mark.parametrize('h', [8, 16])
def test_dgrad_cell_part_rows(h, rows):
    """part of qt_lstm_bwd_dgrad, workgroup by workgroup (fixed 128-row ownership), with and without a second gradient of H'; a
    workgroup past the valid rows writes nothing; accumulate = 1 adds."""
    from qtmpnn import _lib
    c, x = _fused_case(h, rows)
    cap, Kb = c['cap'], 2
    L = M.launch_dgrad(cap, h)
    assert _lib.value('qt_lstm_dgrad_blocks', cap) == L['nblk']
    W = _t(0.3 * np.random.default_rng(rows).standard_normal((Kb * (CB + CBB), 4 * h)))
    nd = n_dev(c)
    for second in (False, True):
        ops, gates, wc, ln, keep = bwd_operands(c, x, cap, second)
        go, ghn, gcn, cp = ops[:4]
        g2 = ops[4] if second else (None, 0)
        _, _, terms, bb = model_bwd(x, second)
        part, pb = M.part_rows(terms, bb['e_terms'], L, rows, h // 4)
        wr = M.written(L, rows)
        for accumulate in (0, 1):
            dG, dCp, out, outb = filled(cap, 4 * h), filled(cap, h), filled(Kb, cap, CB), filled(Kb, cap, CBB)
            dpart = filled(L['nblk'], 11 * h, value=PREFILL if accumulate else SENT)
            call('qt_lstm_bwd_dgrad', go[0], go[1], ghn[0], ghn[1], gcn[0], gcn[1], p(gates), cp[0], cp[1], p(wc), p(ln), cap, p(nd),
                 h, p(dG), p(dCp), p(dpart), accumulate, p(W), None, None, Kb, CB, CBB, p(out), p(outb), 0, g2[0], g2[1], None)
            torch.cuda.synchronize()
            dpart = _np(dpart)
            what = f'h{h} rows{rows} gHn2={second} acc={accumulate}'
            if accumulate:
                check('part dgrad accumulate', what, dpart, PREFILL + part, pb + 2.0 * M.U * np.abs(PREFILL + part))
            else:
                check('part dgrad', what, dpart[wr], part[wr], pb[wr])
                assert (dpart[~wr] == SENT).all(), f'{what}: a workgroup past the valid rows wrote its part row'


@pytest.mark.parametrize('rows', M.FUSED_ROWS_CASES)
@pytest.mark.parametrize('h,Kb', [(8, 2), (16, 2), (16, 4)])          # 64-row tiles of 256 threads; 128-row tiles of 512 (8 waves)
def test_fused_cell_backward_part_and_slab(h, Kb, rows):
    """part and the weight-gradient slab of qt_lstm_bwd_fused, workgroup by workgroup (fixed tile ranges); the launch adds to the
    slab whatever `accumulate` says, and to part with accumulate = 1."""
    from qtmpnn import _lib
    c, x = _fused_case(h, rows)
    cap = c['cap']
    nslab, n_cu = _lib.value('qt_lstm_fused_blocks'), _lib.value('qt_num_cus')
    L = M.launch_fused(cap, h, Kb, n_cu)
    assert L['nblk'] <= nslab
    rng = np.random.default_rng(rows + h)
    W, A = _t(0.3 * rng.standard_normal((Kb * (CB + CBB), 4 * h))), M.draw(rng, rows, 16)
    dA = operand(A, cap, False)[0]
    (go, ghn, gcn, cp), gates, wc, ln, keep = bwd_operands(c, x, cap)
    gG, _, terms, bb = model_bwd(x)
    part, pb = M.part_rows(terms, bb['e_terms'], L, rows, h // 4)
    sl, sb = M.wslab(A, gG, bb['gG'], L, rows)
    nd = n_dev(c)
    for accumulate in (0, 1):
        dCp, out, outb = filled(cap, h), filled(Kb, cap, CB), filled(Kb, cap, CBB)
        dpart = filled(nslab, 11 * h, value=PREFILL if accumulate else float('nan'))
        dslab = filled(nslab, 16, 4 * h, value=PREFILL if accumulate else 0.0)
        call('qt_lstm_bwd_fused', go[0], go[1], ghn[0], ghn[1], gcn[0], gcn[1], p(gates), cp[0], cp[1], p(wc), p(ln), cap, p(nd), h,
             p(dCp), p(dpart), accumulate, p(W), Kb, CB, CBB, p(out), p(outb), p(dA), 16, None, None, 0, None, 1, 16, 0, None, 0,
             p(dslab), nslab)
        torch.cuda.synchronize()
        dpart, dslab = _np(dpart), _np(dslab)
        what = f'h{h} Kb{Kb} rows{rows} acc={accumulate}'
        base = PREFILL if accumulate else 0.0
        check('part fused' + (' accumulate' if accumulate else ''), what, dpart[:L['nblk']], base + part,
              pb + (2.0 * M.U * np.abs(base + part) if accumulate else 0.0))
        check('slab fused' + (' accumulate' if accumulate else ''), what, dslab[:L['nblk']], base + sl,
              sb + (2.0 * M.U * np.abs(base + sl) if accumulate else 0.0))
        rest = dpart[L['nblk']:]
        assert (rest == PREFILL).all() if accumulate else np.isnan(rest).all(), f'{what}: a part row past the grid was written'
        assert (dslab[L['nblk']:] == base).all(), f'{what}: a slab past the grid was written'


def test_zz_report_worst_ratios():
    """Prints the worst error / bound per family of this session (the figures of profiles/cell_f64.txt)."""
    for fam in sorted(WORST):
        print(f'  worst [{fam}]: {WORST[fam]:.3g}')
    assert all(v <= 1.0 for v in WORST.values())
