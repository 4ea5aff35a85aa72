"""The edge-softmax attention kernels (csrc/attn.hip: k_attn_fwd, k_attn_bwd_target, k_attn_bwd_source) against the float64
restatement tests/attn_f64.py: forward, the gradient of all four projection blocks and of We, and the dropout mask edge by edge, at
every lane-group width, in both operand layouts, with head groups, static capacities and the split and unsplit source sweep.

Bounds (the reference is float64, so all of the error is the kernel's): forward |out - ref| <= RTOL * (sum_pairs alpha d |v_j + We a|
+ |skip_i|) per entry, the sum taken from the reference; gradients helpers.grad_close with its defaults, per projection block.
Every case prints its worst error / bound ratios before it asserts (profiles/attn_f64.txt holds a recorded run)."""
import functools
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from attn_f64 import attention_f64, gradients
from helpers import RTOL, dev, grad_close

pytestmark = pytest.mark.gpu

THRESH = 0.1


# ------------------------------------------------------------------------------------------------------------------ meshes
def _frames_d():
    """Three 64 x 64 clips: two whose unsplit 32 x 32 quadrant lies beside a strip of 1 x 1 cells (a bright line one pixel past the
    quadrant's split window), and a noisy one that splits down to single pixels everywhere."""
    f = np.zeros((3, 64, 64), np.float32)
    f[0, 0:32, 33] = 1.0
    f[1, 33, 32:64] = 1.0
    f[1, 10:13, 5:9] = 1.0
    f[2] = 0.2 + 0.5 * np.random.default_rng(5).random((64, 64), dtype=np.float32)
    return f


def _frame_s():
    f = np.zeros((1, 24, 32), np.float32)
    f[0, 5:9, 9:14] = 1.0
    f[0, 17, 20:27] = 1.0
    f[0, 12:21, 2:4] = 1.0
    return f


@functools.lru_cache(maxsize=None)
def _mesh(kind):
    from qtmpnn.mesh import build_mesh, build_pixel_mesh
    if kind == 'S':
        return build_mesh(src=torch.from_numpy(_frame_s()).to(dev()), thresh=THRESH)
    if kind in ('D', 'T'):
        return build_mesh(src=torch.from_numpy(_frames_d()).to(dev()), thresh=THRESH, static=kind == 'T')
    assert kind == 'P'
    mask = np.zeros((24, 32), dtype=bool)                   # (the pixelwise mesh of tests/test_gpu_attn_weights.py)
    mask[:5, :7] = True
    return build_pixel_mesh(1, 24, 32, mask, dev())


@functools.lru_cache(maxsize=None)
def _geo(kind):
    """The valid part of the mesh's attention geometry on the host: what the reference reads."""
    mesh = _mesh(kind)
    N = mesh.n_valid
    _, selfpair, eattr, rev = mesh.attn_geometry()
    rowptr = mesh.rowptr[:N + 1].cpu().numpy()
    E = int(rowptr[-1])
    g = SimpleNamespace(N=N, E=E, cap=mesh.N, rowptr=rowptr, col=mesh.col[:E].cpu().numpy(), eattr=eattr[:E].cpu().numpy(),
                        rev=rev[:E].cpu().numpy().astype(np.int64), slots=int(rev.numel()),
                        selfpair=None if selfpair is None else selfpair[:N].cpu().numpy())
    g.deg = np.diff(rowptr)
    g.pairs = g.deg + (0 if g.selfpair is None else (g.selfpair > 0))
    # the adjacency is symmetric and rev names the transposed entry (the source pass relies on both)
    tgt = np.repeat(np.arange(N), g.deg)
    assert np.array_equal(g.col[g.rev], tgt) and np.array_equal(tgt[g.rev], g.col)
    return g


def _blocks(N, C):
    from qtmpnn import _lib
    return _lib.value('qt_attn_blocks', N, C)


def _assert_small(geo, C):
    """Mesh S: fewer than 8 workgroups in the source pass (plain sweep), a last forward / target workgroup that is not full."""
    assert geo.N * C // 4 < 8 * 256 and _blocks(geo.N, C) < 8, (geo.N, C)
    assert geo.N % 64 != 0


def _assert_split(geo, C):
    """At least 8 workgroups: the source pass deals eighths of the nodes to the XCDs; the eighths are ragged."""
    assert _blocks(geo.N, C) >= 8, (geo.N, C)
    assert geo.N % 8 != 0


def _assert_degrees(geo):
    """Mesh D: a row of 32 or more edges, odd and even pair counts (edges + self pair; two pairs per loop trip), nodes with and
    without a self pair."""
    assert geo.deg.max() >= 32, geo.deg.max()
    assert (geo.pairs % 2 == 1).any() and (geo.pairs % 2 == 0).any()
    assert (geo.selfpair > 0).any() and (geo.selfpair == 0).any()


def _assert_kind(kind, C):
    geo = _geo('D' if kind == 'T' else kind)
    if kind == 'S':
        _assert_small(geo, C)
    elif kind == 'P':
        assert geo.selfpair is None and _mesh('P').pixelwise
    else:
        _assert_degrees(geo)
        _assert_split(geo, C)
    if kind == 'T':
        sta, st = _mesh('T'), _geo('T')
        assert sta.n_dev is not None and st.N == geo.N and st.cap == 3 * 64 * 64 and st.N < st.cap
        assert np.array_equal(st.rowptr, geo.rowptr) and np.array_equal(st.col, geo.col) and np.array_equal(st.rev, geo.rev)
        assert np.array_equal(st.eattr, geo.eattr) and np.array_equal(st.selfpair, geo.selfpair)
    return geo


# ------------------------------------------------------------------------------------------------------------------ checks
_GC = {k: v.default for k, v in inspect.signature(grad_close).parameters.items()}


def _grad_ratio(a, b):
    """worst |a - b| / (atol + rtol |b|) with helpers.grad_close's own defaults (read from its signature)."""
    rtol, rel_atol, floor = _GC['rtol'], _GC['rel_atol'], _GC['floor']
    a, b = a.detach().double().cpu().numpy(), b.detach().numpy()
    tol = rel_atol * max(floor, float(np.abs(b).max())) + rtol * np.abs(b)
    return float((np.abs(a - b) / tol).max())


def _check(tag, ref, g, out, gproj, gWe):
    """out (>= N rows, gmod C), gproj (>= N rows, G 4C) rows side by side, gWe (G, C, 2) against the reference and its gradients."""
    N, G, C = ref.N, ref.G, ref.C
    rp, rw = gradients(ref, g)
    err = (out[:N].detach().double().cpu() - ref.out.detach()).abs()
    ratios = [('out', float((err / (RTOL * ref.absum)).max()))]
    blocks = []
    for b, name in enumerate(('q', 'k', 'v', 'skip')):
        a, r = gproj[:N].view(N, G, 4, C)[:, :, b], rp.view(N, G, 4, C)[:, :, b]
        blocks.append((f'd{name}', a, r))
    blocks.append(('dWe', gWe.reshape(G, C, 2), rw))
    ratios += [(name, _grad_ratio(a, r)) for name, a, r in blocks]
    print(f'attn_f64 {tag}: ' + ' '.join(f'{n}={v:.3g}' for n, v in ratios))
    assert not torch.isnan(gWe).any(), f'{tag}: NaN in the We gradient'
    assert not torch.isnan(gproj[:N]).any(), f'{tag}: NaN in a valid row of the projection gradient'
    assert not torch.isnan(out[:N]).any(), f'{tag}: NaN in a valid row of the output'
    assert ratios[0][1] <= 1.0, f'{tag}: forward error is {ratios[0][1]:.3g} x its bound'
    for name, a, r in blocks:
        grad_close(a, r, msg=f'{tag} {name}')


def _operands(geo, C, G, gmod, seed, qk=1.0, we=0.3):
    """Host fp32 operands: proj (N, G 4C), We (G, C, 2), incoming gradient (N, gmod C)."""
    gen = torch.Generator().manual_seed(seed)
    P = torch.randn(geo.N, G, 4, C, generator=gen)
    P[:, :, :2] *= qk
    We = torch.randn(G, C, 2, generator=gen) * we
    g = torch.randn(geo.N, (gmod or G) * C, generator=gen)
    return P.reshape(geo.N, G * 4 * C).contiguous(), We, g


def _reference(geo, proj, We, c_real, G, keep, seed, epoch, gmod=0):
    return attention_f64(geo.rowptr, geo.col, geo.selfpair, geo.eattr, proj.numpy(), We.numpy(), c_real, G, keep, seed, epoch, gmod)


def _pad(t, rows):
    """t on the device, with NaN rows up to `rows` (the capacity rows of a static mesh are garbage by contract)."""
    out = torch.full((rows, t.shape[1]), float('nan'), device=dev())
    out[:t.shape[0]] = t.to(dev())
    return out


def _apply(kind, geo, proj, We, g, c_real, G, gmod, keep, seed, epoch):
    """ops._Attention on mesh `kind` with the device's dropout epoch set to `epoch` (restored afterwards)."""
    from qtmpnn import ops
    mesh = _mesh(kind)
    p = _pad(proj, mesh.N).requires_grad_(True)
    w = We.to(dev()).requires_grad_(True)
    ep = ops.dropout_epoch(dev())
    saved = int(ep.item())
    try:
        ep.fill_(epoch)
        out = ops._Attention.apply(p, w, mesh, c_real, keep, seed, None, G, gmod)
        gp, gw = torch.autograd.grad(out, [p, w], _pad(g, mesh.N))
        torch.cuda.synchronize()
    finally:
        ep.fill_(saved)
    return out, gp, gw


def _case(tag, kind, C, c_real, G, gmod, keep, seed, epoch, opseed, qk=1.0, props=_assert_kind):
    geo = props(kind, C)
    proj, We, g = _operands(geo, C, G, gmod, opseed, qk)
    ref = _reference(geo, proj, We, c_real, G, keep, seed, epoch, gmod)
    out, gp, gw = _apply(kind, geo, proj, We, g, c_real, G, gmod, keep, seed, epoch)
    _check(tag, ref, g, out, gp, gw)
    return ref


# ------------------------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize('C', [4, 8, 16, 32, 64, 128])
def test_every_channel_width(C):
    """One head, no dropout, every lane-group width, the source sweep split over the XCDs: mesh D, and for C = 64 / 128 mesh S, the
    smallest mesh here that still launches 8 source workgroups at that width."""
    def split_only(kind, C):                    # mesh S: unsplit sweep at C = 16 (_assert_small), 8 or more workgroups at C >= 64
        _assert_split(_geo(kind), C)
        return _geo(kind)
    if C >= 64:
        _case(f'width C={C} mesh=S', 'S', C, C, 1, 0, 1.0, 1, 0, 100 + C, props=split_only)
    else:
        _case(f'width C={C} mesh=D', 'D', C, C, 1, 0, 1.0, 1, 0, 100 + C)


@pytest.mark.parametrize('C,c_real', [(4, 1), (8, 5)])
def test_fewer_real_channels_than_columns(C, c_real):
    """c_real < C: the scores are scaled by 1 / sqrt(c_real), nothing else changes."""
    _case(f'c_real C={C} c_real={c_real}', 'D', C, c_real, 1, 0, 1.0, 1, 0, 200 + C)


@pytest.mark.parametrize('G,gmod', [(3, 0), (8, 0), (4, 2)])
def test_heads_and_head_groups(G, gmod):
    """G heads in one launch at C = 8; gmod = 2 of G = 4: the output is the sum of the two head groups and both groups read the
    same incoming gradient."""
    _case(f'heads G={G} gmod={gmod}', 'D', 8, 8, G, gmod, 1.0, 1, 0, 300 + G)


# (keep, device epoch, host seed): every epoch with every keep < 1, the seeds dealt so that neither follows the other
DROPOUT = [(1.0, 7, 1), (0.9, 0, 0xDEADBEEF), (0.9, 1, 1234), (0.9, 7, 2654435768), (0.5, 0, 1234), (0.5, 1, 2654435768),
           (0.5, 7, 0xDEADBEEF)]


@pytest.mark.parametrize('keep,epoch,seed', DROPOUT)
@pytest.mark.parametrize('kind', ['S', 'D', 'P', 'T'])
def test_every_mesh_with_dropout(kind, keep, epoch, seed):
    """C = 16, two heads, on the small (unsplit sweep), the degrees (split sweep), the pixelwise and the static mesh (NaN in the
    capacity rows of proj and of the incoming gradient; the reference is that of the dynamic mesh), at the device epochs 0, 1, 7."""
    ref = _case(f'mesh={kind} keep={keep} epoch={epoch} seed={seed}', kind, 16, 16, 2, 0, keep, seed, epoch, 400 + epoch)
    if keep < 1.0:
        rate = float((ref.mult > 0).double().mean())
        assert abs(rate - keep) <= 5 * (keep * (1 - keep) / ref.mult.numel()) ** 0.5, rate
    else:
        assert bool((ref.mult == 1).all())


def _raw(mesh, geo, C, c_real, G, keep, seed, epoch_t, proj, ld, ps, hs, We, g, ld_g, hs_g, out_shape, ld_o, hs_o, gmod=0,
         accumulate=0, part=None, fwd=None):
    """qt_attn_fwd (unless `fwd` = (out, stats) is given) and qt_attn_bwd -> out, stats, gproj, part, coef."""
    from qtmpnn import _lib
    from qtmpnn._lib import ptr
    xy, selfpair, eattr, rev = mesh.attn_geometry()
    args = (ptr(mesh.rowptr), ptr(mesh.col), ptr(xy), ptr(eattr), ptr(selfpair))
    N = mesh.N
    if fwd is None:
        out, stats = torch.empty(out_shape, device=dev()), torch.empty(G, N, 2, device=dev())
        _lib.call('qt_attn_fwd', *args, ptr(proj), ld, ptr(We), C, c_real, N, ptr(mesh.n_dev), keep, seed, ptr(epoch_t), ptr(out),
                  ptr(stats), G, ld_o, ps, hs, hs_o)
    else:
        out, stats = fwd
    gp = torch.full_like(proj, float('nan'))
    if part is None:
        part = torch.full((_blocks(N, C), G * 2 * C), float('nan'), device=dev())
    coef = torch.zeros(G, geo.slots + N, 2, device=dev())
    _lib.call('qt_attn_bwd', *args, ptr(proj), ld, ptr(We), C, c_real, N, ptr(mesh.n_dev), keep, seed, ptr(epoch_t), ptr(g), ld_g,
              ptr(stats), ptr(out), ld_o, ptr(gp), ptr(part), accumulate, ptr(rev), ptr(coef), geo.slots, G, gmod, ps, hs, hs_g, hs_o)
    torch.cuda.synchronize()
    return out, stats, gp, part, coef


def _we_grad(part, G, C):
    return part.sum(0).view(G, 2, C).transpose(1, 2)


def test_planes_layout_with_dropout():
    """One dense (N, C) plane per head and block (ld = C, ps = N C, hs = 4 N C) through the raw entry points, keep = 0.5, G = 3."""
    geo, mesh = _assert_kind('D', 8), _mesh('D')
    N, G, C, keep, seed, epoch = geo.N, 3, 8, 0.5, 77, 3
    proj, We, g = _operands(geo, C, G, 0, 500)
    ref = _reference(geo, proj, We, C, G, keep, seed, epoch)
    planes = proj.view(N, G, 4, C).permute(1, 2, 0, 3).contiguous().to(dev())
    gpl = g.view(N, G, C).permute(1, 0, 2).contiguous().to(dev())
    ep = torch.tensor([epoch], dtype=torch.int32, device=dev())
    out, _, gp, part, _ = _raw(mesh, geo, C, C, G, keep, seed, ep, planes, C, N * C, 4 * N * C, We.to(dev()), gpl, C, N * C,
                               (G, N, C), C, N * C)
    _check('planes G=3 keep=0.5', ref, g, out.permute(1, 0, 2).reshape(N, G * C), gp.permute(2, 0, 1, 3).reshape(N, G * 4 * C),
           _we_grad(part, G, C))


def test_wide_scores():
    """q and k scaled until the largest per-target spread of the scores lies between 20 and 40 (read from the reference): the online
    softmax rescales by exp(-20 ...) and __expf runs far from 0.  No dropout."""
    geo = _assert_kind('D', 16)
    C = 16
    for qk in (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0):
        proj, We, g = _operands(geo, C, 1, 0, 600, qk)
        ref = _reference(geo, proj, We, C, 1, 1.0, 1, 0)
        if float(ref.spread.max()) >= 20.0:
            break
    spread = float(ref.spread.max())
    assert 20.0 <= spread <= 40.0, spread
    out, gp, gw = _apply('D', geo, proj, We, g, C, 1, 0, 1.0, 1, 0)
    _check(f'wide scores spread={spread:.1f}', ref, g, out, gp, gw)


def test_accumulate_adds_the_second_launch_into_the_slab():
    """accumulate bit 0: two backward launches with different incoming gradients into one `part` slab, the second adding; the slab
    then holds the sum of the two float64 We gradients."""
    geo, mesh = _assert_kind('D', 8), _mesh('D')
    N, G, C = geo.N, 2, 8
    proj, We, g1 = _operands(geo, C, G, 0, 700)
    g2 = torch.randn(N, G * C, generator=torch.Generator().manual_seed(701))
    ref = _reference(geo, proj, We, C, G, 1.0, 1, 0)
    want = gradients(ref, g1)[1] + gradients(ref, g2)[1]
    p, w = proj.to(dev()), We.to(dev())
    lay = (p, G * 4 * C, C, 4 * C, w)
    out, stats, _, part, _ = _raw(mesh, geo, C, C, G, 1.0, 1, None, *lay, g1.to(dev()), G * C, C, (N, G * C), G * C, C)
    first = _we_grad(part, G, C).clone()
    _raw(mesh, geo, C, C, G, 1.0, 1, None, *lay, g2.to(dev()), G * C, C, (N, G * C), G * C, C, accumulate=1, part=part, fwd=(out, stats))
    got = _we_grad(part, G, C)
    print(f'attn_f64 accumulate: dWe={_grad_ratio(got, want):.3g} first={_grad_ratio(first, gradients(ref, g1)[1]):.3g}')
    grad_close(first, gradients(ref, g1)[1], msg='first launch')
    grad_close(got, want, msg='both launches')


@pytest.mark.parametrize('kind', ['S', 'D'])
def test_dropout_mask_edge_by_edge(kind):
    """The mask the kernels drew, read from the target pass: coef[g, rev[e], 1] = alpha d of the message col[e] -> row(e) (self pairs
    at slot E + i, E the capacity of the edge arrays) is non-zero exactly where attn_f64.dropout_mask keeps the pair and equals
    alpha / keep there (alpha before dropout from ops.attention_weights, same slot order); the forward under the same mask matches
    the reference.  So the forward pass, the target pass and the specification agree pair by pair."""
    from qtmpnn import ops
    geo, mesh = _assert_kind(kind, 8), _mesh(kind)
    N, G, C, keep, seed, epoch = geo.N, 3, 8, 0.5, 0xDEADBEEF, 5
    proj, We, g = _operands(geo, C, G, 0, 800, qk=0.5, we=0.1)
    ref = _reference(geo, proj, We, C, G, keep, seed, epoch)
    assert float(ref.alpha.min()) > 1e-6, float(ref.alpha.min())
    p, w = proj.to(dev()), We.to(dev())
    ep = torch.tensor([epoch], dtype=torch.int32, device=dev())
    out, _, gp, part, coef = _raw(mesh, geo, C, C, G, keep, seed, ep, p, G * 4 * C, C, 4 * C, w, g.to(dev()), G * C, C, (N, G * C),
                                  G * C, C)
    _check(f'mask mesh={kind}', ref, g, out, gp, _we_grad(part, G, C))
    alpha_e, alpha_s = ops.attention_weights(p, w, mesh, C, G)
    alpha = torch.cat([alpha_e, alpha_s], dim=1).double().cpu().numpy()                    # (G, slots + N) in slot order
    slot = np.where(ref.edge >= 0, geo.rev[np.maximum(ref.edge, 0)], geo.slots + ref.tgt)
    assert len(np.unique(slot)) == len(slot)
    got = coef[:, :, 1].double().cpu().numpy()[:, slot]                                   # (G, pairs)
    kept = (ref.mult.numpy() > 0).T
    assert 0.4 < kept.mean() < 0.6
    for h in range(G):
        wrong = np.nonzero((got[h] != 0) != kept[h])[0]
        assert wrong.size == 0, f'head {h}: {wrong.size} pairs kept / dropped against the specification, first (i, j) = ' \
                                f'({ref.tgt[wrong[0]]}, {ref.src[wrong[0]]})'
        want = alpha[h, slot][kept[h]] / float(np.float32(keep))
        rel = np.abs(got[h][kept[h]] - want) / want
        assert rel.max() <= 1e-5, (h, rel.max())
    assert any(not np.array_equal(kept[0], kept[h]) for h in range(1, G))
