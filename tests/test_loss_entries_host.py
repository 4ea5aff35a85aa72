"""CPU-side refusals of the eight rollout-loss entry points (no GPU): qt_{sse,bce,wsse,wbce}_rollout and _bwd run through one
forward and one backward launcher, so every pair refuses the same bad arguments, before any launch, and the error begins with the
name of the entry that was called.  The squared-error pair had no such test; the other three keep theirs beside their models."""
import ctypes

import pytest

_BUF = (ctypes.c_void_p * 64)()
X = ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16         # only ever validated, never dereferenced
ONE = (ctypes.c_int * 16)(*([1] * 16))
PTRS = (ctypes.c_void_p * 16)(*([X] * 16))
NO_PTRS, ZEROS = (ctypes.c_void_p * 16)(), (ctypes.c_int * 16)()
BAD_PW = [dict(pw=0.0), dict(pw=-1.0), dict(pw=float('nan')), dict(pw=float('inf')), dict(pw=-float('inf'))]
# the list of tests/test_bce_host.py::test_bce_entries_refuse_bad_arguments, and what the shared checks add to it
FWD = [dict(nseg=0), dict(nseg=17), dict(y=None), dict(part=None), dict(B=0), dict(n=0), dict(m=-8), dict(sums=None),
       dict(sums=NO_PTRS), dict(strides=ZEROS), dict(Ns=(ctypes.c_int * 16)(*([-1] * 16))), dict(y_clip=-1), dict(y_step=-64)]
BWD = [dict(nseg=0), dict(nseg=17), dict(g=None), dict(W=0), dict(gouts=None), dict(sums=NO_PTRS),
       dict(Ns=(ctypes.c_int * 16)(*([1 << 30] * 16)), W=4)]


@pytest.mark.parametrize('kind', ['sse', 'bce', 'wsse', 'wbce'])
def test_rollout_loss_entries_refuse_bad_arguments_by_name(kind):
    from qtmpnn import _lib
    lib = _lib.load()
    weighted, has_pw = kind[0] == 'w', kind == 'wbce'

    def fwd(nseg=1, outs=PTRS, strides=ONE, labels=PTRS, levels=PTRS, Ns=ONE, sums=PTRS, y=X, y_clip=64, y_step=64, w=X, lam=X,
            B=1, n=8, m=8, part=X, pw=1.0):
        return getattr(lib, f'qt_{kind}_rollout')(nseg, outs, strides, labels, levels, Ns, sums, y, y_clip, y_step,
                                                  *((w, lam) if weighted else ()), B, n, m, part, *((pw,) if has_pw else ()), None)

    def bwd(nseg=1, outs=PTRS, strides=ONE, npixs=PTRS, sums=PTRS, Ns=ONE, n_devs=PTRS, g=X, lam=X, W=1, gouts=PTRS, pw=1.0):
        return getattr(lib, f'qt_{kind}_rollout_bwd')(nseg, outs, strides, *(() if weighted else (npixs,)), sums, Ns, n_devs, g,
                                                      *((lam,) if weighted else ()), W, gouts, *((pw,) if has_pw else ()), None)
    own = ([dict(w=None), dict(lam=None)] if weighted else []) + (BAD_PW if has_pw else [])
    own_bwd = ([dict(lam=None)] if weighted else [dict(npixs=None), dict(npixs=NO_PTRS)]) + (BAD_PW if has_pw else [])
    for call, cases, name in ((fwd, FWD + own, f'qt_{kind}_rollout'), (bwd, BWD + own_bwd, f'qt_{kind}_rollout_bwd')):
        for kw in cases:
            assert call(**kw) != 0, (name, kw)
            err = lib.qt_last_error()
            assert err.startswith(name.encode() + b': '), (name, kw, err)
            if 'pw' in kw:
                assert b'pos_weight' in err, (name, kw, err)
