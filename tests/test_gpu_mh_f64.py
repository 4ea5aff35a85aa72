"""The multi-head attention kernels (csrc/mhattn.hip: k_mh_fwd, k_mh_merge_bwd) and the attention coefficients (csrc/attnw.hip:
k_attn_weights) against the float64 model tests/mh_f64.py: through ops._MHAttention at every head count and width, on every mesh and
with dropout; through the C ABI (cat, stats, the merge backward on a column block, accumulate, sentinels, the grid-stride loop above
8192 rows); qt_attn_weights in both operand layouts; and the refusals of the entry points.

The meshes are those of tests/test_gpu_attn_f64.py (S, D, P, T) and L: three all-pixel 64 x 64 clips, more rows than one sweep of
k_mh_merge_bwd's grid.  Bounds and checkers: tests/mh_f64.py (every majorant from the float64 reference alone); every case prints its
worst error / bound ratios before it asserts (profiles/mh_f64.txt holds a recorded run)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mh_f64 as M
import test_gpu_attn_f64 as A
from helpers import dev

pytestmark = pytest.mark.gpu

SENT = 7777.0              # what the outputs hold before a launch: rows the kernels must not touch keep it
PAD_ROWS = 3               # rows of y, cat and gcat beyond the mesh's capacity


# ------------------------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    if kind != 'L':
        return A._mesh(kind)
    from qtmpnn.mesh import build_mesh
    f = 0.2 + 0.5 * np.random.default_rng(9).random((3, 64, 64), dtype=np.float32)
    return build_mesh(src=torch.from_numpy(f).to(dev()), thresh=A.THRESH)


@functools.lru_cache(maxsize=None)
def _geo(kind):
    if kind != 'L':
        return A._geo(kind)
    mesh = _mesh('L')
    N = mesh.n_valid
    _, selfpair, eattr, rev = mesh.attn_geometry()
    rowptr = mesh.rowptr[:N + 1].cpu().numpy()
    E = int(rowptr[-1])
    g = SimpleNamespace(N=N, E=E, cap=mesh.N, rowptr=rowptr, col=mesh.col[:E].cpu().numpy(), eattr=eattr[:E].cpu().numpy(),
                        rev=rev[:E].cpu().numpy().astype(np.int64), slots=int(rev.numel()),
                        selfpair=None if selfpair is None else selfpair[:N].cpu().numpy())
    g.deg = np.diff(rowptr)
    tgt = np.repeat(np.arange(N), g.deg)
    assert np.array_equal(g.col[g.rev], tgt) and np.array_equal(tgt[g.rev], g.col)
    return g


def _props(kind, C):
    """The properties the case relies on, asserted; -> the geometry the reference reads (mesh D's for mesh T)."""
    if kind == 'S':
        geo = _geo('S')
        assert geo.N % (256 // C) != 0 and geo.N % 64 != 0, (geo.N, C)       # a last workgroup that is not full (256 / C nodes each)
        return geo
    if kind == 'L':
        geo, mesh = _geo('L'), _mesh('L')
        assert mesh.n_dev is None and geo.N == mesh.N == 3 * 64 * 64 and geo.N > M.SWEEP       # every pixel a node: a second sweep
        assert geo.selfpair is None or not (geo.selfpair > 0).any()
        return geo
    return A._assert_kind(kind, C)


def _base(kind):
    return 'D' if kind == 'T' else kind


# ------------------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def _ref(kind, C, c_real, H, keep, seed, epoch, opseed, dtype=torch.float64):
    """(operands, model) on the valid part of mesh `kind` (D for T): computed once per case, shared, never written."""
    geo = _geo(kind)
    o = M.operands(geo.N, C, c_real, H, opseed)
    return o, M.model(geo.rowptr, geo.col, geo.selfpair, geo.eattr, o.proj, o.We, o.Wt, o.blin, c_real, H, keep, seed, epoch, dtype)


def _case_ref(c):
    return _ref(_base(c['kind']), c['C'], c['c_real'], c['H'], c['keep'], c['seed'], c['epoch'], c['opseed'])


def _pad(t, rows, fill=float('nan')):
    out = torch.full((rows,) + tuple(t.shape[1:]), fill, device=dev())
    out[:t.shape[0]] = t.to(dev())
    return out


# ------------------------------------------------------------------------------------------------------------------ ops._MHAttention
def _apply(mesh, o, c_real, H, keep, seed, epoch, grad=True):
    """ops._MHAttention on `mesh` with the device's dropout epoch set to `epoch` (restored afterwards); NaN in the capacity rows of
    proj and of the incoming gradient."""
    from qtmpnn import ops
    ins = [_pad(o.proj, mesh.N)] + [t.to(dev()) for t in (o.We, o.Wt, o.blin)]
    if grad:
        ins = [t.requires_grad_(True) for t in ins]
    ep = ops.dropout_epoch(dev())
    saved = int(ep.item())
    try:
        ep.fill_(epoch)
        y = ops._MHAttention.apply(*ins, mesh, c_real, keep, seed, None, None, H)
        grads = torch.autograd.grad(y, ins, _pad(o.g, mesh.N)) if grad else None
        torch.cuda.synchronize()
    finally:
        ep.fill_(saved)
    return y.detach(), grads


def _run_apply(c):
    _props(c['kind'], c['C'])
    mesh = _mesh(c['kind'])
    o, ref = _case_ref(c)
    y, (gp, gw, gwt, gb) = _apply(mesh, o, c['c_real'], c['H'], c['keep'], c['seed'], c['epoch'])
    assert not torch.isnan(y[:ref.N]).any(), f"{c['name']}: NaN in a valid row of y"
    assert not torch.isnan(gp[:ref.N]).any(), f"{c['name']}: NaN in a valid row of the projection gradient"
    M.check_forward(c['name'], ref, y)
    M.check_grads(c['name'], ref, M.gradients(ref, o.g), gp, gw, gwt, gb)
    if c['c_real'] < c['C']:
        assert not y[:ref.N, c['c_real']:].any() and not gp[:ref.N].view(ref.N, c['H'], 4, c['C'])[..., c['c_real']:].any()
    return mesh, o, ref, y


_ids = lambda cases: [c['name'] for c in cases]


@pytest.mark.parametrize('c', M.APPLY_HEADS, ids=_ids(M.APPLY_HEADS))
def test_every_head_count_and_width(c):
    """H = 1 .. 4 (three, two, one and no idle lane group in the merge's shuffles) x C = 4 .. 32 on mesh D, no dropout."""
    _run_apply(c)


@pytest.mark.parametrize('c', M.APPLY_CREAL, ids=_ids(M.APPLY_CREAL))
def test_fewer_real_channels_than_columns(c):
    """c_real < C with the caller's zero padding: scores scaled by 1 / sqrt(c_real), the padded columns of y and d proj stay zero."""
    _run_apply(c)


@pytest.mark.parametrize('c', M.APPLY_MESHES, ids=_ids(M.APPLY_MESHES))
def test_every_mesh(c):
    """Meshes S, P, T (static, NaN capacity rows, mesh D's reference) and L (the merge backward's second sweep)."""
    _run_apply(c)


def test_dropout_triples_are_those_of_the_attention_file():
    assert M.DROPOUT == A.DROPOUT


@pytest.mark.parametrize('c', M.APPLY_DROPOUT, ids=_ids(M.APPLY_DROPOUT))
def test_dropout_masks_of_three_heads(c):
    """C = 16, H = 3 on D and T: y under the reference's masks (head h draws seed + h 0x632BE5AB, mixed with the device epoch) within
    its bound -- one pair kept or dropped against them moves y by O(1) -- and keep < 1 did change y."""
    mesh, o, ref, y = _run_apply(c)
    if c['keep'] < 1.0:
        y1, _ = _apply(mesh, o, c['c_real'], c['H'], 1.0, c['seed'], c['epoch'], grad=False)
        M.check_dropout_acted(c['name'], y, y1, ref.N)
        kept = (ref.att.mult > 0)
        assert any(not torch.equal(kept[:, 0], kept[:, h]) for h in range(1, c['H']))
    else:
        assert bool((ref.att.mult == 1).all())


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _fwd(mesh, o, C, c_real, H, with_cat=True):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    _, selfpair, eattr, _ = mesh.attn_geometry()
    rows = mesh.N + PAD_ROWS
    ins = [_pad(o.proj, mesh.N)] + [t.to(dev()) for t in (o.We, o.Wt, o.blin)]
    y = torch.full((rows, C), SENT, device=dev())
    cat = torch.full((rows, H * C), SENT, device=dev()) if with_cat else None
    stats = torch.full((H, mesh.N, 2), SENT, device=dev())
    _lib.call('qt_mhattn_fwd', ptr(mesh.rowptr), ptr(mesh.col), ptr(eattr), ptr(selfpair), *[ptr(t) for t in ins], C, c_real, H, mesh.N,
              ptr(mesh.n_dev), 1.0, 1, None, ptr(y), ptr(stats), ptr(cat))
    torch.cuda.synchronize()
    return y, cat, stats


def _merge(mesh, C, H, g, Wt, cat, part, accumulate):
    """qt_mhattn_bwd_merge with g handed as the columns 20 .. 20 + C of a matrix C + 36 wide whose other entries, and whose
    capacity rows, are NaN -> gcat (capacity + PAD_ROWS rows, pre-filled with the sentinel)."""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    ld = C + M.LD_G_EXTRA
    wide = torch.full((mesh.N, ld), float('nan'), device=dev())
    wide[:g.shape[0], 20:20 + C] = g.to(dev())
    gcat = torch.full((mesh.N + PAD_ROWS, H * C), SENT, device=dev())
    _lib.call('qt_mhattn_bwd_merge', wide[:, 20:].data_ptr(), ld, ptr(Wt), ptr(cat), C, H, mesh.N, ptr(mesh.n_dev), ptr(gcat), ptr(part),
              accumulate)
    torch.cuda.synchronize()
    return gcat


def _colsum(part, H, C):
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    out = torch.full((part.shape[1],), float('nan'), device=dev())
    _lib.call('qt_colsum', ptr(part), part.shape[0], part.shape[1], ptr(out))
    torch.cuda.synchronize()
    return out[:H * C * C].view(H * C, C), out[H * C * C:]


@pytest.mark.parametrize('kind,C,H', M.RAW, ids=[f'{k}-C{c}-H{h}' for k, c, h in M.RAW])
def test_entry_points(kind, C, H):
    """qt_mhattn_fwd, qt_mhattn_bwd_merge and qt_colsum as the C ABI states them, on D, T (static) and L (more than 8192 rows)."""
    from qtmpnn import _lib
    _props(kind, C)
    mesh, tag = _mesh(kind), f'raw {kind}-C{C}-H{H}'
    o, ref = _ref(_base(kind), C, C, H, 1.0, 1, 0, 2000 + 16 * C + H)
    N = ref.N
    nblk = _lib.value('qt_mhattn_blocks', mesh.N, C, H)
    assert nblk == (M.MERGE_GRID if mesh.N > M.SWEEP else -(-mesh.N // M.MERGE_ROWS)), nblk
    if kind == 'L':
        assert nblk == 256 and N > nblk * M.MERGE_ROWS         # valid rows beyond one sweep: the stride loop and its second barrier round
    if kind == 'D':
        assert nblk < 256

    # forward: cat, y, stats (H, Ncap, 2); cat = NULL gives the same y; rows past the valid ones untouched
    y, cat, stats = _fwd(mesh, o, C, C, H)
    y0, _, stats0 = _fwd(mesh, o, C, C, H, with_cat=False)
    M.check_forward(tag, ref, y, cat)
    M.check_stats(tag, ref, stats)
    assert torch.equal(y0[:N], y[:N]) and torch.equal(stats0[:, :N], stats[:, :N]), f'{tag}: cat = NULL changed the result'
    for name, t in (('y', y), ('y (cat = NULL)', y0), ('cat', cat)):
        assert bool((t[N:] == SENT).all()), f'{tag}: a row of {name} past the valid rows was written'
    assert bool((stats[:, N:] == SENT).all()), f'{tag}: stats written past the valid rows of a head plane'
    if N < mesh.N:
        cat[N:] = float('nan')                                # capacity rows are garbage by contract

    # merge backward: gcat, and [dWt | dblin] over slabs pre-filled with NaN (accumulate = 0 overwrites)
    Wt = o.Wt.to(dev())
    nent = H * C * C + C
    part = torch.full((nblk, nent), float('nan'), device=dev())
    gcat = _merge(mesh, C, H, o.g, Wt, cat, part, 0)
    grads = M.gradients(ref, o.g)
    M.check_gcat(tag, ref, grads, gcat)
    assert bool((gcat[N:] == SENT).all()), f'{tag}: a row of gcat past the valid rows was written'
    assert not torch.isnan(part).any(), f'{tag}: accumulate = 0 left a NaN in a slab'
    M.check_merge_grads(tag, grads, *_colsum(part, H, C))

    # two uses with accumulate = 1 into zeroed slabs: the float64 sum of both
    part = torch.zeros(nblk, nent, device=dev())
    _merge(mesh, C, H, o.g, Wt, cat, part, 1)
    gcat2 = _merge(mesh, C, H, o.g2, Wt, cat, part, 1)
    grads2 = M.gradients(ref, o.g2)
    M.check_gcat(tag + ' second', ref, grads2, gcat2)
    M.check_merge_grads(tag + ' accumulated', None, *_colsum(part, H, C), scale=(grads.Wt + grads2.Wt, grads.blin + grads2.blin))


# ------------------------------------------------------------------------------------------------------------------ qt_attn_weights
@pytest.mark.parametrize('layout', M.LAYOUTS)
@pytest.mark.parametrize('kind,C', M.WEIGHTS, ids=[f'{k}-C{c}' for k, c in M.WEIGHTS])
def test_attention_weights(kind, C, layout):
    """qt_attn_weights at G = 3 with rows side by side (ps = hs = 0) and with one dense (Ncap, C) plane per head and block (ld = C,
    ps = Ncap C, hs = 4 Ncap C: the layout of ops.multi_conv), NaN in the capacity rows; operands at qk = 1.0."""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    geo, mesh, G = _props(kind, C), _mesh(kind), M.WEIGHTS_G
    key = (_base(kind), C, C, G, 1.0, 1, 0, 3000 + C)
    (o, ref), (_, f32) = _ref(*key), _ref(*key, torch.float32)
    N, cap = ref.N, mesh.N
    if layout == 'rows':
        p, ld, ps, hs = _pad(o.proj, cap), G * 4 * C, 0, 0
    else:
        p = torch.full((G, 4, cap, C), float('nan'), device=dev())
        p[:, :, :N] = o.proj.view(N, G, 4, C).permute(1, 2, 0, 3).to(dev())
        ld, ps, hs = C, cap * C, 4 * cap * C
    _, selfpair, eattr, rev = mesh.attn_geometry()
    slots = int(rev.numel())
    alpha_e = torch.full((G, slots), SENT, device=dev())
    alpha_s = torch.full((G, cap), SENT, device=dev())
    _lib.call('qt_attn_weights', ptr(mesh.rowptr), ptr(mesh.col), ptr(eattr), ptr(selfpair), ptr(p), ld, ps, hs, ptr(o.We.to(dev())), C, C,
              G, cap, ptr(mesh.n_dev), ptr(rev), slots, ptr(alpha_e), ptr(alpha_s))
    torch.cuda.synchronize()
    M.check_alpha(f'weights {kind}-C{C} {layout}', ref, geo.rev, geo.selfpair, alpha_e, alpha_s, yardstick=f32)
    assert bool((alpha_s[:, N:] == SENT).all()), 'alpha_s written past the valid rows'
    unused = np.ones(slots, dtype=bool)
    unused[geo.rev] = False
    assert bool((alpha_e[:, torch.from_numpy(unused).to(dev())] == SENT).all()), 'alpha_e written at a slot no valid edge owns'
    if kind == 'T':
        assert N < cap


# ------------------------------------------------------------------------------------------------------------------ refusals
REFUSALS = [
    ('heads=0', dict(heads=0), 'bad head count'),
    ('heads=5', dict(heads=5), 'bad head count'),
    ('C=12', dict(C=12), 'bad channel count'),
    ('c_real=C+1', dict(c_real=17), 'bad channel count'),
    ('misaligned y', dict(y_shift=1), '16-byte aligned'),
    ('ld_g<C', dict(ld_g=15), 'bad row stride'),
]


@pytest.mark.parametrize('what,change,reason', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, change, reason):
    """A non-zero code with qt_last_error naming the reason (ops._lib.call raises with both), and nothing launched: every output
    still holds the sentinel."""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    mesh = _mesh('S')
    N, C, H = mesh.N, 16, 3
    a = dict(C=C, c_real=C, heads=H, y_shift=0, ld_g=C)
    a.update(change)
    _, selfpair, eattr, _ = mesh.attn_geometry()
    wide = 5 * 4 * 16                                          # room for five heads, whatever is asked for
    proj, We, Wt, blin = (torch.zeros(s, device=dev()) for s in ((N, wide), (5, 16, 2), (5 * 16, 16), (16,)))
    y, stats, cat = (torch.full(s, SENT, device=dev()) for s in ((N + 1, 16), (5, N, 2), (N, 5 * 16)))
    g, gcat, part = torch.zeros(N, 16, device=dev()), torch.full((N, 5 * 16), SENT, device=dev()), torch.full((256, 5 * 16 * 16 + 16), SENT, device=dev())
    if what != 'ld_g<C':
        with pytest.raises(RuntimeError, match=f'qt_mhattn_fwd failed .*{reason}'):
            _lib.call('qt_mhattn_fwd', ptr(mesh.rowptr), ptr(mesh.col), ptr(eattr), ptr(selfpair), ptr(proj), ptr(We), ptr(Wt), ptr(blin),
                      a['C'], a['c_real'], a['heads'], N, ptr(mesh.n_dev), 1.0, 1, None, y.data_ptr() + 4 * a['y_shift'], ptr(stats), ptr(cat))
    if what in ('heads=0', 'heads=5', 'C=12', 'ld_g<C'):
        named = 'bad row stride' if what == 'ld_g<C' else 'bad channel / head count'
        with pytest.raises(RuntimeError, match=f'qt_mhattn_bwd_merge failed .*{named}'):
            _lib.call('qt_mhattn_bwd_merge', ptr(g), a['ld_g'], ptr(Wt), ptr(cat), a['C'], a['heads'], N, ptr(mesh.n_dev), ptr(gcat), ptr(part), 0)
    if what in ('heads=0', 'heads=5', 'C=12'):
        assert _lib.value('qt_mhattn_blocks', N, a['C'], a['heads']) == 0
    torch.cuda.synchronize()
    for t in (y, stats, cat, gcat, part):
        assert bool((t == SENT).all()), f'{what}: an output was written'
