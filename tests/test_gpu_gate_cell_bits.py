"""The fused gate GEMM + LSTM cell launch (qt_dense_lstm: k_gate_cell_p at hidden 8 / 16) against the unfused pair qt_dense
-> qt_lstm_fwd, bit for bit, at the row counts where a wave's 32-row unit is empty, partial, full and just over, and with a
device-side row count below the buffers' capacity: rows past the count must keep the bytes they had before the launch.
The persistent kernel loads clamped rows for the units' tails and masks only its stores, so this pins both the values of the
valid rows and the store range."""
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
