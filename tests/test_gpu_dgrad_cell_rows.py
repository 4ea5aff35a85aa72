"""k_dgrad_cell's stores, row by row: qt_lstm_bwd_dgrad against qt_lstm_bwd -> qt_dense2 on the stored gG, bit for bit, at the
smallest shapes where a store that moves whole gG rows from the workgroup's LDS tile can go wrong.  At hidden 16 the launch
writes gG as the contiguous run of its 128-row tile, 16 bytes a thread and 1 KB a wave, after the cell phase; at hidden 8 from
the cell phase, a quarter row per lane.  Either way: the valid rows carry qt_lstm_bwd's bits, and no byte of a row at or past the
device-side count changes -- in gG, in gCprev, in the planes of both layouts or in the `part` rows of workgroups without a row.

Shapes: N (the buffers' rows) around one and two 128-row tiles and at half a tile (a wave's share of the run); counts 0, 1, one
less than a tile boundary, a tile boundary, and N itself; NB = 20, 64, 68, 128 output columns (one, two, the odd third and four
32-column MFMA tiles, both passes of the staged epilogue); planes row-major and slice-major; with and without Cprev, gO, the
second gradient of H' and the plane-0 addend; `part` written and accumulated.  gG starts 16 bytes into its allocation: the entry
asks for no more alignment than that, so a store that assumed a whole line would fault or smear here.

The anchors, qt_lstm_bwd and qt_dense2, are held to float64 models by tests/test_gpu_cell_f64.py and tests/test_gpu_gemm_f64.py."""
import pytest
import torch

from helpers import dev

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
# NB -> (Kb, Cb, Cbb): 20 = five 4-channel planes; 64 and 128 = two / four planes of 16 + 16 channels (slice-major planes with four
# pieces a row); 68 = one plane of 48 + 20 channels (the third MFMA tile holds 4 columns, the second epilogue pass one piece a row)
PLANES = {20: (5, 4, 0), 64: (2, 16, 16), 68: (1, 48, 20), 128: (4, 16, 16)}
# (ln, Cprev, gO, gHn2, add0)
OPTS = [(True, True, True, True, True), (False, False, False, False, False), (True, False, True, False, True),
        (False, True, False, True, False)]


def _counts(N):
    c = {0, 1, N}
    for b in range(128, N + 128, 128):
        c |= {b - 1, b}
    return sorted(x for x in c if x <= N)


def _full(*s):
    return torch.full(s, SENTINEL, device=dev())


def _inputs(h, N):
    torch.manual_seed(9100 + 10 * h + N)
    d = dev()
    gates = torch.cat([torch.sigmoid(torch.randn(N, 2 * h, device=d)), torch.tanh(torch.randn(N, h, device=d)),
                       torch.sigmoid(torch.randn(N, h, device=d))], 1).contiguous()
    r = lambda *s: torch.randn(*s, device=d)
    t = dict(gates=gates, Cp=r(N, h), gHn=r(N, h), gHn2=r(N, h), gCn=r(N, h), gO=r(N, h), wc=r(3, h), ln=r(4, h),
             add0=r(N, 48), Wrows=0.3 * r(128, 4 * h), P=r((N + 127) // 128, 11 * h))
    t['gHsum'] = t['gHn'] + t['gHn2']            # the launch adds the second gradient on load: one float32 addition, as here
    return t


def _reference(t, h, N, n_dev, rows, Kb, Cb, Cbb, opt, out_sm):
    """(gG, gCprev, out, outb) of qt_lstm_bwd, then qt_dense2 on its stored gG, then the plane-0 addend; sentinel-filled"""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    ln, cp, go, gh2, add0 = opt
    gG, gCp, out = _full(N, 4 * h), _full(N, h), _full(Kb, N, Cb)
    outb = _full(Kb, N, Cbb) if Cbb else None
    part = torch.zeros(_lib.value('qt_lstm_bwd_blocks', N, h), 11 * h, device=dev())
    _lib.call('qt_lstm_bwd', ptr(t['gO']) if go else None, h, ptr(t['gHsum'] if gh2 else t['gHn']), h, ptr(t['gCn']), h,
              ptr(t['gates']), ptr(t['Cp']) if cp else None, h, ptr(t['wc']), ptr(t['ln']) if ln else None, N, ptr(n_dev), h,
              ptr(gG), ptr(gCp), ptr(part), 0)
    _lib.call('qt_dense2', ptr(gG), 0, None, None, 0, None, 1, 4 * h, 0, None, ptr(t['Wrows'][:Kb * (Cb + Cbb)]), None, 0, None,
              Kb, Cb, Cbb, N, ptr(n_dev), 0, None, 0, None, ptr(out), ptr(outb), 2 * out_sm, None, None)
    if add0:
        out[0, :rows] += t['add0'][:rows, :Cb]
    return gG, gCp, out, outb


def _check_planes(name, got, ref, rows, N, Kb, C, out_sm):
    assert torch.equal(got, ref), f'{name}: differs from qt_dense2 on the stored gG'
    assert bool((got[0, rows:] == SENTINEL).all()), f'{name}: plane 0 written at or past the device-side count'
    rest = got[1:].reshape(Kb - 1, C // 4, N, 4)[:, :, rows:] if out_sm else got[1:, rows:]
    assert bool((rest == SENTINEL).all()), f'{name}: planes 1.. written at or past the device-side count'


@pytest.mark.parametrize('N', [1, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize('h', [8, 16])
def test_dgrad_cell_row_stores_bits_and_range(h, N):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    t = _inputs(h, N)
    nblk = _lib.value('qt_lstm_dgrad_blocks', N)
    assert nblk == (N + 127) // 128
    i = 0
    for rows in _counts(N):
        n_dev = torch.tensor([rows], dtype=torch.int32, device=dev())
        live = (rows + 127) // 128                 # workgroups that hold a valid row
        for NB, (Kb, Cb, Cbb) in PLANES.items():
            for out_sm in (0, 1):
                # every option set meets every (count, NB, layout) over two neighbouring cases; all four at the tile boundaries
                for opt in (OPTS if rows % 128 in (0, 127) and rows else (OPTS[i % 4], OPTS[(i + 1) % 4])):
                    ln, cp, go, gh2, add0 = opt
                    what = f'rows={rows} NB={NB} out_sm={out_sm} ln={ln} Cprev={cp} gO={go} gHn2={gh2} add0={add0}'
                    rG, rCp, rout, routb = _reference(t, h, N, n_dev, rows, Kb, Cb, Cbb, opt, out_sm)
                    # gG one 16-byte step into a sentinel-filled allocation: base aligned to 16 bytes and no more
                    buf = _full(N * 4 * h + 8)
                    gG = buf[4:4 + N * 4 * h].view(N, 4 * h)
                    assert gG.data_ptr() % 32 == 16
                    gCp, out = _full(N, h), _full(Kb, N, Cb)
                    outb = _full(Kb, N, Cbb) if Cbb else None
                    a0 = t['add0'][:, :Cb].contiguous() if add0 else None
                    part0, part1 = _full(nblk, 11 * h), t['P'].clone()
                    for part, accumulate in ((part0, 0), (part1, 1)):      # (the second launch rewrites the same values elsewhere)
                        _lib.call('qt_lstm_bwd_dgrad', ptr(t['gO']) if go else None, h, ptr(t['gHn']), h, ptr(t['gCn']), h,
                                  ptr(t['gates']), ptr(t['Cp']) if cp else None, h, ptr(t['wc']), ptr(t['ln']) if ln else None, N,
                                  ptr(n_dev), h, ptr(gG), ptr(gCp), ptr(part), accumulate, ptr(t['Wrows'][:NB]), None, None, Kb, Cb,
                                  Cbb, ptr(out), ptr(outb), out_sm, ptr(t['gHn2']) if gh2 else None, h, ptr(a0))
                    torch.cuda.synchronize()
                    assert torch.equal(gG[:rows], rG[:rows]), f'gG differs from qt_lstm_bwd ({what})'
                    assert torch.equal(gCp[:rows], rCp[:rows]), f'gCprev differs from qt_lstm_bwd ({what})'
                    assert bool((gG[rows:] == SENTINEL).all()), f'gG: rows at or past the device-side count were written ({what})'
                    assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + N * 4 * h:] == SENTINEL).all()), f'gG: written outside the buffer ({what})'
                    assert bool((gCp[rows:] == SENTINEL).all()), f'gCprev: rows at or past the device-side count were written ({what})'
                    for name, a in (('gG (qt_lstm_bwd)', rG), ('gCprev (qt_lstm_bwd)', rCp)):
                        assert bool((a[rows:] == SENTINEL).all()), f'{name}: rows at or past the device-side count were written ({what})'
                    _check_planes(f'out ({what})', out, rout, rows, N, Kb, Cb, out_sm)
                    if Cbb:
                        _check_planes(f'outb ({what})', outb, routb, rows, N, Kb, Cbb, out_sm)
                    # `part`: a workgroup with a valid row writes its row (accumulate = 0) or adds to it (one float32 addition);
                    # a workgroup without one leaves its row alone
                    assert bool((part0[live:] == SENTINEL).all()) and torch.equal(part1[live:], t['P'][live:]), f'part: a row of a workgroup without valid rows changed ({what})'
                    assert bool((part0[:live] != SENTINEL).all()), f'part: a live workgroup left its row unwritten ({what})'
                    assert torch.equal(part1[:live], t['P'][:live] + part0[:live]), f'part: accumulate = 1 is not P + the accumulate = 0 row ({what})'
                    i += 1
