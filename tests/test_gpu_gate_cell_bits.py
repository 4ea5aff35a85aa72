"""The fused gate GEMM + LSTM cell launch (qt_dense_lstm: k_gate_cell_p at hidden 8 / 16) against the unfused pair qt_dense
-> qt_lstm_fwd, bit for bit, at the row counts where a wave's 32-row unit is empty, partial, full and just over, and with a
device-side row count below the buffers' capacity: rows past the count must keep the bytes they had before the launch.
The persistent kernel loads clamped rows for the units' tails and masks only its stores, so this pins both the values of the
valid rows and the store range.

The tiled CELL epilogue of k_gemm_fwd -- qt_dense_lstm at hidden 32, and at hidden 8 / 16 when the packed gate matrix has more than
GATE_P_MAXK = 256 rows -- is tied to the same pair in the same way.  That is the bit-for-bit route: qt_dense launches the very
k_gemm_fwd<NT, KWT> the epilogue is compiled into (NB = 4h = 128 columns: <4, 64>; NB = 64: <2, 128>), so the accumulators hold the
same k-ordered MFMA chain, and cell_forward is one function.  Its row tile is 128 rows: partial, full and just over.

qt_lstm_fwd and qt_lstm_bwd, the anchors of every comparison here, are held to the float64 cell model by tests/test_gpu_cell_f64.py,
and so are the `part` rows and the weight-gradient slab of the fused backward launches, accumulate = 1 included."""
import pytest
import torch

from helpers import dev

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


def _run(h, Ka, rows, with_c, with_o):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    torch.manual_seed(1000 * h + 10 * Ka + rows % 97)
    d = dev()
    cap = rows + 70                       # capacity > count: two more units' worth of rows that no launch may write
    C, Ks = 4 + h, 4
    K = Ka * C + Ks
    Z = torch.randn(cap, C, device=d)
    TZ = torch.randn(Ka - 1, cap, C, device=d)
    S = torch.randn(cap, Ks, device=d)
    W = 0.3 * torch.randn(K, 4 * h, device=d)
    Cp = torch.randn(cap, h, device=d) if with_c else None
    wc, b, ln = torch.randn(3, h, device=d), torch.randn(4, h, device=d), torch.randn(4, h, device=d)
    n_dev = torch.tensor([rows], dtype=torch.int32, device=d)
    full = lambda *s: torch.full(s, SENTINEL, device=d)

    # unfused: the gate sums as a matrix, then the stand-alone cell kernel
    G = full(cap, 4 * h)
    _lib.call('qt_dense', ptr(Z), ptr(TZ), Ka, C, ptr(W), ptr(S), Ks, ptr(W[Ka * C:]), 1, 4 * h, cap, ptr(n_dev), 0, None, 0, None, ptr(G))
    ref = dict(O=full(cap, h), Hn=full(cap, h), Cn=full(cap, h), gates=full(cap, 4 * h))
    _lib.call('qt_lstm_fwd', ptr(G), None, 0, ptr(Cp), h if with_c else 0, ptr(wc), ptr(b), ptr(ln), cap, ptr(n_dev), h,
              ptr(ref['O']), ptr(ref['Hn']), ptr(ref['Cn']), ptr(ref['gates']))

    out = dict(O=full(cap, h) if with_o else None, Hn=full(cap, h), Cn=full(cap, h), gates=full(cap, 4 * h))
    _lib.call('qt_dense_lstm', ptr(Z), C, ptr(TZ), None, 0, None, Ka, C, 0, ptr(W), None, ptr(S), Ks, ptr(W[Ka * C:]), h, cap,
              ptr(n_dev), ptr(Cp), h if with_c else 0, ptr(wc), ptr(b), ptr(ln), ptr(out['O']), ptr(out['Hn']), ptr(out['Cn']),
              ptr(out['gates']), 0)
    torch.cuda.synchronize()
    return out, ref


@pytest.mark.parametrize('with_o', [True, False])
@pytest.mark.parametrize('with_c', [True, False])
@pytest.mark.parametrize('rows', [1, 31, 32, 33, 4075])
@pytest.mark.parametrize('h,Ka', [(8, 3), (8, 5), (16, 3), (16, 5)])   # reductions of 40 / 64 (h = 8), 64 / 104 (h = 16): generic and unrolled rings
def test_fused_gate_cell_bits_and_store_range(h, Ka, rows, with_c, with_o):
    out, ref = _run(h, Ka, rows, with_c, with_o)
    for name, a in out.items():
        if a is None:
            continue
        assert torch.equal(a[:rows], ref[name][:rows]), f'{name}: valid rows differ from qt_dense + qt_lstm_fwd'
        assert bool((a[rows:] == SENTINEL).all()), f'{name}: rows past the device-side count were written'
        assert bool((ref[name][rows:] == SENTINEL).all()), f'{name} (unfused): rows past the device-side count were written'
    # the gate block's last quarter IS the output gate: the O output is its second copy
    if with_o:
        assert torch.equal(out['O'][:rows], out['gates'][:rows, 3 * h:])


@pytest.mark.parametrize('with_o', [True, False])
@pytest.mark.parametrize('with_c', [True, False])
@pytest.mark.parametrize('rows', [1, 127, 128, 129])
@pytest.mark.parametrize('h,Ka', [(32, 3), (16, 13)])    # k_gemm_fwd<4, 64, 8> (two k passes of 112); <2, 128, 4> at a reduction of 264 > GATE_P_MAXK
def test_tiled_cell_epilogue_bits_and_store_range(h, Ka, rows, with_c, with_o):
    assert h == 32 or Ka * (4 + h) + 4 > 256
    out, ref = _run(h, Ka, rows, with_c, with_o)
    for name, a in out.items():
        if a is None:
            continue
        assert torch.equal(a[:rows], ref[name][:rows]), f'{name}: valid rows differ from qt_dense + qt_lstm_fwd'
        assert bool((a[rows:] == SENTINEL).all()), f'{name}: rows past the device-side count were written'
    if with_o:
        assert torch.equal(out['O'][:rows], out['gates'][:rows, 3 * h:])


# ---- the backward launches against the unfused pair qt_lstm_bwd -> qt_dense2: every launch is cell_backward per node, and the
# data gradient is the MFMA chain of k_gemm_fwd on the stored gG.  The `part` rows are summed in another order per launch shape:
# tests/test_gpu_cell_f64.py compares them, and the fused launch's weight-gradient slab, with the float64 model workgroup by workgroup.
CB, CBB = 16, 16          # both parts of an output plane: 32 columns a plane, Kb planes = Kb 32-column MFMA tiles
OPTS = [(True, True, True), (False, False, False), (True, False, True), (False, True, False)]     # (ln, Cprev, gO)


def _bwd_inputs(h, rows, cap):
    torch.manual_seed(7000 + 10 * h + rows % 89)
    d = dev()
    gates = torch.cat([torch.sigmoid(torch.randn(cap, 2 * h, device=d)), torch.tanh(torch.randn(cap, h, device=d)),
                       torch.sigmoid(torch.randn(cap, h, device=d))], 1).contiguous()
    t = dict(gates=gates, Cp=torch.randn(cap, h, device=d), gHn=torch.randn(cap, h, device=d), gCn=torch.randn(cap, h, device=d),
             gO=torch.randn(cap, h, device=d), wc=torch.randn(3, h, device=d), ln=torch.randn(4, h, device=d),
             Wrows=0.3 * torch.randn(4 * (CB + CBB), 4 * h, device=d), A=torch.randn(cap, 16, device=d),
             n_dev=torch.tensor([rows], dtype=torch.int32, device=d))
    return t


def _reference(t, h, cap, Kb, ln, cp, go, out_sm):
    """qt_lstm_bwd, then qt_dense2 on its stored gG: (gG, gCprev, out, outb), sentinel-filled"""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    full = lambda *s: torch.full(s, SENTINEL, device=dev())
    gG, gCp, out, outb = full(cap, 4 * h), full(cap, h), full(Kb, cap, CB), full(Kb, cap, CBB)
    part = torch.zeros(_lib.value('qt_lstm_bwd_blocks', cap, h), 11 * h, device=dev())
    _lib.call('qt_lstm_bwd', ptr(t['gO']) if go else None, h, ptr(t['gHn']), h, ptr(t['gCn']), h, ptr(t['gates']),
              ptr(t['Cp']) if cp else None, h, ptr(t['wc']), ptr(t['ln']) if ln else None, cap, ptr(t['n_dev']), h, ptr(gG),
              ptr(gCp), ptr(part), 0)
    _lib.call('qt_dense2', ptr(gG), 0, None, None, 0, None, 1, 4 * h, 0, None, ptr(t['Wrows']), None, 0, None, Kb, CB, CBB, cap,
              ptr(t['n_dev']), 0, None, 0, None, ptr(out), ptr(outb), 2 * out_sm, None, None)
    return gG, gCp, out, outb


def _check_planes(name, got, ref, rows, cap, Kb, C, out_sm):
    assert torch.equal(got, ref), f'{name}: differs from qt_dense2 on the stored gG'
    assert bool((got[0, rows:] == SENTINEL).all()), f'{name}: plane 0 written past the device-side count'
    rest = got[1:].reshape(Kb - 1, C // 4, cap, 4)[:, :, rows:] if out_sm else got[1:, rows:]
    assert bool((rest == SENTINEL).all()), f'{name}: planes 1.. written past the device-side count'


@pytest.mark.parametrize('rows', [1, 127, 128, 129, 300])      # the 128-row tile empty, partial, full, just over, a third tile
@pytest.mark.parametrize('h', [8, 16])
def test_dgrad_cell_bits_and_store_range(h, rows):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    cap = rows + 70
    t = _bwd_inputs(h, rows, cap)
    full = lambda *s: torch.full(s, SENTINEL, device=dev())
    for Kb in (2, 3, 4):                  # NB = 64, 96, 128 columns: the three NT instances
        for out_sm in (0, 1):
            for ln, cp, go in OPTS:
                rG, rCp, rout, routb = _reference(t, h, cap, Kb, ln, cp, go, out_sm)
                gG, gCp, out, outb = full(cap, 4 * h), full(cap, h), full(Kb, cap, CB), full(Kb, cap, CBB)
                part = torch.zeros(_lib.value('qt_lstm_dgrad_blocks', cap), 11 * h, device=dev())
                _lib.call('qt_lstm_bwd_dgrad', ptr(t['gO']) if go else None, h, ptr(t['gHn']), h, ptr(t['gCn']), h, ptr(t['gates']),
                          ptr(t['Cp']) if cp else None, h, ptr(t['wc']), ptr(t['ln']) if ln else None, cap, ptr(t['n_dev']), h,
                          ptr(gG), ptr(gCp), ptr(part), 0, ptr(t['Wrows']), None, None, Kb, CB, CBB, ptr(out), ptr(outb), out_sm,
                          None, 0, None)
                torch.cuda.synchronize()
                what = f'Kb={Kb} out_sm={out_sm} ln={ln} Cprev={cp} gO={go}'
                assert torch.equal(gG[:rows], rG[:rows]) and torch.equal(gCp[:rows], rCp[:rows]), f'gG / gCprev differ from qt_lstm_bwd ({what})'
                for name, a in (('gG', gG), ('gCprev', gCp), ('gG (qt_lstm_bwd)', rG), ('gCprev (qt_lstm_bwd)', rCp)):
                    assert bool((a[rows:] == SENTINEL).all()), f'{name}: rows past the device-side count were written ({what})'
                _check_planes(f'out ({what})', out, rout, rows, cap, Kb, CB, out_sm)
                _check_planes(f'outb ({what})', outb, routb, rows, cap, Kb, CBB, out_sm)


@pytest.mark.parametrize('rows', [1, 63, 64, 65, 129])         # the 64-row tile empty, partial, full, just over, a third tile
@pytest.mark.parametrize('h', [8, 16])
def test_fused_cell_backward_bits_and_store_range(h, rows):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    cap = rows + 70
    t = _bwd_inputs(h, rows, cap)
    full = lambda *s: torch.full(s, SENTINEL, device=dev())
    nslab = _lib.value('qt_lstm_fused_blocks')
    for Kb in ((1, 2, 3, 4) if h == 16 else (1, 2)):          # all six instances; four tiles: 128-row tiles, 512 threads
        for ln, cp, go in OPTS:
            _, rCp, rout, routb = _reference(t, h, cap, Kb, ln, cp, go, 0)
            gCp, out, outb = full(cap, h), full(Kb, cap, CB), full(Kb, cap, CBB)
            part = torch.zeros(nslab, 11 * h, device=dev())
            slab = torch.zeros(nslab, 16, 4 * h, device=dev())
            _lib.call('qt_lstm_bwd_fused', ptr(t['gO']) if go else None, h, ptr(t['gHn']), h, ptr(t['gCn']), h, ptr(t['gates']),
                      ptr(t['Cp']) if cp else None, h, ptr(t['wc']), ptr(t['ln']) if ln else None, cap, ptr(t['n_dev']), h,
                      ptr(gCp), ptr(part), 0, ptr(t['Wrows']), Kb, CB, CBB, ptr(out), ptr(outb),
                      ptr(t['A']), 16, None, None, 0, None, 1, 16, 0, None, 0, ptr(slab), nslab)
            torch.cuda.synchronize()
            what = f'Kb={Kb} ln={ln} Cprev={cp} gO={go}'
            assert torch.equal(gCp[:rows], rCp[:rows]), f'gCprev differs from qt_lstm_bwd ({what})'
            assert bool((gCp[rows:] == SENTINEL).all()), f'gCprev: rows past the device-side count were written ({what})'
            _check_planes(f'out ({what})', out, rout, rows, cap, Kb, CB, 0)
            _check_planes(f'outb ({what})', outb, routb, rows, cap, Kb, CBB, 0)
