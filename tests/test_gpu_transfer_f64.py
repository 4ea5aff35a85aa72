"""The mesh <-> image transfer kernels (csrc/transfer.hip, csrc/remeshclip.hip) and the training-loss kernels against the float64
pixel model tests/transfer_f64.py, which knows a mesh only by its label map.

Bound, everywhere: an output entry whose exact value is sum_k t_k lies within 64 * 2^-24 * sum_k |t_k| of the model (the model
returns sum_k |t_k|); copies and gathers of one value are compared bit for bit.  64 is derived, not measured: the longest rounding
chain is 16 serial pixel adds, four 4-way pyramid levels (<= 12 adds), the 1 / npix scale and the optional source scale, about 30
roundings, doubled.  Inputs are sign * (0.5 + U[0, 1)): no term is small against its neighbours, so one missing, extra or misplaced
pixel of a 4096-pixel cell is an error of >= 0.5 / 4096, twenty times the bound.  All valid rows and all pixels are compared; every
case prints its worst error / (2^-24 sum |t|) before it asserts (pytest -s; a recorded run: profiles/transfer_f64.txt).
Every transfer case runs with ops._CLIP_REMESH True and False, and each run is held to the model, not to the other run."""
import copy

import numpy as np
import pytest
import torch

import transfer_f64 as M
from helpers import dev, golden

pytestmark = pytest.mark.gpu

LIMIT = 64.0
SENT = -7.25            # sentinel of pre-filled outputs
FLAGS = [True, False]


# ------------------------------------------------------------------------------------------------------------------ helpers
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


def _draw(rng, *shape):
    """sign * (0.5 + U[0, 1)) as float32."""
    return (rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))).astype(np.float32)


def _labels(mesh):
    return _np(mesh.labels).reshape(mesh.B, -1).astype(np.int64)


def _nv(mesh):
    return mesh.n_valid


def _rows(mesh, a, rng=None):
    """Node tensor for `mesh` from the (n_valid, ...) array a: in static mode padded to the capacity with NaN rows."""
    a = np.asarray(a, np.float32)
    if mesh.N > a.shape[0]:
        a = np.concatenate([a, np.full((mesh.N - a.shape[0], *a.shape[1:]), np.nan, np.float32)])
    return _t(a)


class _flag:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from qtmpnn import ops
        self.prev, ops._CLIP_REMESH = ops._CLIP_REMESH, self.on

    def __exit__(self, *exc):
        from qtmpnn import ops
        ops._CLIP_REMESH = self.prev


def check(name, got, ref, mag):
    """|got - ref| <= 64 u mag, entry by entry; where mag == 0 the entry must equal ref exactly.  Prints the worst ratio."""
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, np.float64)
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{name}: non-finite value in a compared entry'
    err = np.abs(got - ref)
    # the float32 rounding of the exact value itself is part of the chain, nothing is added for it
    pos = mag > 0
    ratio = float((err[pos] / (M.U * mag[pos])).max()) if pos.any() else 0.0
    print(f'  {name}: {ratio:.3g}')
    assert (err[~pos] == 0).all(), f'{name}: an entry without terms is not exactly {ref[~pos][:1]}'
    assert ratio <= LIMIT, f'{name}: worst error / (2^-24 sum|t|) = {ratio:.4g} > {LIMIT}'
    return ratio


def same_bits(name, got, ref):
    got = _np(got) if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref).astype(np.float32)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=True), f'{name}: {int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum())} entries differ'
    print(f'  {name}: bit for bit')


# ------------------------------------------------------------------------------------------------------------------- meshes
_CACHE = {}


def _crit(tag, variant):
    """Criterion images (B, n, m) of mesh `tag`; variant 0 / 1: two different images of the same kind (a transfer's old and new)."""
    rng = np.random.default_rng(100 * variant + ord('D' if tag == 'T' else tag))      # (T repeats D's images)
    if tag == 'S':
        c = np.zeros((1, 24, 32), np.float32)
        if variant == 0:
            c[0, 0:5, 0:7] = 1.0
        else:
            c[0, 17:22, 9:12] = 1.0
            c[0, 3, 29] = 1.0
        return c
    if tag == 'C':
        c = np.zeros((2, 64, 40), np.float32)
        c[0, 30:36, 33:40] = 1.0
        c[1] = rng.random((64, 40)) < 0.03
        if variant:
            c = c[::-1].copy()
            c[0, 5, 5] = 1.0
        return c
    if tag in ('D', 'T'):
        c = np.zeros((3, 64, 64), np.float32)
        fine, noise, zero = (0, 1, 2) if variant == 0 else (2, 0, 1)
        for _ in range(3):
            r, q = rng.integers(0, 58), rng.integers(0, 56)
            c[fine, r:r + 5, q:q + 7] = 1.0
        c[noise] = rng.random((64, 64)) < 0.12
        c[zero] = 0.0
        return c
    if tag == 'M':
        c = np.zeros((2, 100, 150), np.float32)
        c[0] = rng.random((100, 150)) < 0.04
        c[1, 10:17, 70:90] = 1.0
        c[1, 80:85, 20:24] = 1.0
        if variant:
            c = c[::-1].copy()
            c[0, 50:53, 100:120] = 1.0
        return c
    raise KeyError(tag)


def _mask(tag):
    if tag == 'M':
        mk = np.zeros((100, 150), bool)
        mk[37:42, 5:91] = True            # a strip that is aligned to no cell border
        mk[64:100, 128:150] = True        # all of tile (1, 2)
        return mk
    if tag == 'P':
        mk = np.zeros((24, 32), bool)
        mk[5:9, 10:30] = True
        mk[20, 0:3] = True
        return mk
    return None


def mesh_of(tag, variant=0):
    """The test meshes, built once.  S 24x32 B=1 | C 64x40 B=2 | D 64x64 B=3 | M 100x150 B=2 masked | T = D static | P 24x32 pixelwise,
    masked | H 48x64 homogeneous preset with loss_mask, B=2 | R = (old D, new built from old's node values)."""
    from qtmpnn.mesh import build_mesh, build_pixel_mesh
    key = (tag, variant)
    if key in _CACHE:
        return _CACHE[key]
    if tag == 'P':
        ms = build_pixel_mesh(2, 24, 32, mask=_mask('P'), device=dev())
    elif tag == 'H':
        from model.graph_functions import create_static_homogeneous_graph
        g = golden('fixed_homog48x64.npz')
        ms = create_static_homogeneous_graph((48, 64), int(g['max_grid_size']), g['mask'], use_edge_attrs=False, device=dev())['mapping']
        ms = ms.for_batch(2)
    elif tag == 'R':
        old = mesh_of('D', 0)
        rng = np.random.default_rng(5)
        val = _t(rng.random(old.N) * 0.6)
        new = build_mesh(prev=(val, old), thresh=0.5)
        ms = (old, new)
    else:
        ms = build_mesh(src=_t(_crit(tag, variant)), thresh=0.5, mask=_mask(tag), static=(tag == 'T'))
    _CACHE[key] = ms
    return ms


def _mixed_blocks(lab, n, m, z):
    """Number of aligned z x z pixel blocks of a (n, m) label image that hold pixels with AND without a node."""
    cnt = 0
    for r in range(0, n, z):
        for c in range(0, m, z):
            blk = lab[r:r + z, c:c + z]
            cnt += int((blk < 0).any() and (blk >= 0).any())
    return cnt


def test_every_mesh_holds_the_condition_it_was_built_for():
    """The edges the cases below are meant to reach are present in the meshes, and the pixel counts the kernels divide by are the
    model's bincount of the labels (an independent check of `npix`)."""
    from qtmpnn import ops
    lv = lambda ms: (int(ms.level.min()), int(ms.level.max()))
    for tag in 'SCDMTPH':
        for variant in ((0, 1) if tag in 'SCDMT' else (0,)):
            ms = mesh_of(tag, variant)
            nv = _nv(ms)
            lab = _labels(ms)
            assert lab.max() == nv - 1 and np.array_equal(M.npix(lab, nv), _np(ms.npix)[:nv].astype(np.float64)), tag
    S, C, D, Mm, T, P, H = (mesh_of(t) for t in 'SCDMTPH')
    assert (S.B, S.n, S.m) == (1, 24, 32) and lv(S) == (0, 4)                  # smaller than a tile: the LDS pyramid's levels 3, 4 only
    assert (C.B, C.n, C.m) == (2, 64, 40) and lv(C)[0] == 0 and lv(C)[1] >= 4   # a ragged column tile
    assert D.B == 3 and lv(D) == (0, 6)
    labD = _labels(D)
    per_clip = [len(np.unique(labD[b])) for b in range(3)]
    assert per_clip[2] == 1 and per_clip[1] > 400 and 1 < per_clip[0] < per_clip[1]     # one unsplit 64 x 64 cell, noise down to 1 x 1, fine patches
    assert Mm.P == 15000 and Mm.P % 1024 == 664 and Mm.B == 2 and lv(Mm)[0] == 0 and lv(Mm)[1] >= 5
    labM = _labels(Mm).reshape(2, 100, 150)
    assert (labM[:, 64:100, 128:150] < 0).all()                                 # one empty tile
    off = _np(Mm.cell_off)
    assert (np.diff(off) == 0).sum() == 2 and (np.diff(off) > 0).sum() == 10    # ... in both clips, by the row ranges too
    # The mask strip cuts through what would be cells: aligned 2 x 2, 4 x 4 and 8 x 8 blocks (the units the kernels sum in registers)
    # hold pixels with a node beside pixels without one.  (The decomposition itself splits every cell that holds a masked pixel down
    # to single pixels -- csrc/quadtree.hip stage 1 -- so on a quadtree mesh a pixel without a node is a level-0 pixel; the
    # homogeneous mesh H is the one whose cells keep masked pixels, under loss_mask.)
    assert all(_mixed_blocks(labM[b], 100, 150, z) > 0 for b in range(2) for z in (2, 4, 8))
    inside = (labM[:, 37:42, 5:91] < 0).all() and (labM[:, 36, 5:91] >= 0).all() and (labM[:, 42, 5:91] >= 0).all()
    assert inside
    assert T.n_dev is not None and T.n_valid < T.N and T.N == 3 * 4096 and torch.equal(T.labels, D.labels)
    assert P.pixelwise and P.mask is not None and (_labels(P) < 0).any() and lv(P) == (0, 0)
    assert H.loss_mask is not None and H.B == 2 and (H.n, H.m) == (48, 64)
    labH, mkH = _labels(H), _np(H.loss_mask).reshape(-1) != 0
    assert (mkH & (labH[0] >= 0)).any() and (labH[0] < 0).any()                # masked pixels inside kept cells, and removed cells
    old, new = mesh_of('R')
    assert new.built_from() is old and new.fwd_src is not None and old is mesh_of('D')
    fs = _np(new.fwd_src)[:new.N]
    assert (fs >= 0).any() and (fs < 0).any() and new.N != old.N                # direct copies and multi-pixel nodes
    for a, b in (('S', 'S'), ('D', 'D'), ('M', 'M'), ('T', 'T')):
        with _flag(True):
            assert ops.clip_remesh_ok(mesh_of(a, 0), mesh_of(b, 1))
        with _flag(False):
            assert not ops.clip_remesh_ok(mesh_of(a, 0), mesh_of(b, 1))
    with _flag(True):
        assert ops.clip_remesh_ok(old, new)


# --------------------------------------------------------------------------------------------------------------- pool_image
POOL_SC = [(1, 1), (4, 1), (2, 3), (1, 5), (10, 4), (1, 16)]


@pytest.mark.parametrize('clip', FLAGS)
@pytest.mark.parametrize('tag', list('SCDMTPH'))
def test_pool_image_forward_and_pixel_gradient(tag, clip):
    """ops.pool_image: node sums / means of (B, S, P, C) frames and the gradient back onto the pixels, for a contiguous image and for
    a strided view of the frames [1, 1 + S) of a longer clip; (1, 16) lies beyond the clip kernel's C <= 8 (qt_pool's float4 path)."""
    from qtmpnn import ops
    ms = mesh_of(tag)
    lab, nv, B, P = _labels(ms), _nv(ms), ms.B, ms.P
    inv = 1.0 / np.maximum(M.npix(lab, nv), 1.0)
    rng = np.random.default_rng(11)
    worst = 0.0
    with _flag(clip):
        for S, C in POOL_SC:
            x = _draw(rng, B, S + 2, P, C)
            g = _draw(rng, S, nv, C)
            for strided in (False, True):
                for mean in (True, False):
                    base = _t(x).requires_grad_(True) if strided else _t(x[:, 1:1 + S]).requires_grad_(True)
                    img = base[:, 1:1 + S] if strided else base
                    out = ops.pool_image(img, ms, mean)
                    ref, mag = M.pool(x[:, 1:1 + S], lab, nv, mean)
                    nm = f'pool {tag} clip={int(clip)} S={S} C={C} strided={int(strided)} mean={int(mean)}'
                    worst = max(worst, check(nm, out[:, :nv], ref, mag))
                    (gx,) = torch.autograd.grad(out, base, _rows_s(ms, g))
                    gx = _np(gx)
                    if strided:
                        assert (gx[:, 0] == 0).all() and (gx[:, S + 1] == 0).all()
                        gx = gx[:, 1:1 + S]
                    for s in range(S):
                        gr, gm = M.gather(g[s], lab, inv if mean else None)
                        if mean:
                            worst = max(worst, check(nm + f' grad s={s}', gx[:, s], gr, gm))
                        else:
                            same_bits(nm + f' grad s={s}', gx[:, s], gr)
    print(f'pool_image {tag} clip={int(clip)}: worst {worst:.3g}')


def _rows_s(mesh, a):
    """(S, n_valid, C) -> (S, N, C) with NaN capacity rows."""
    a = np.asarray(a, np.float32)
    if mesh.N > a.shape[1]:
        a = np.concatenate([a, np.full((a.shape[0], mesh.N - a.shape[1], a.shape[2]), np.nan, np.float32)], axis=1)
    return _t(a)


@pytest.mark.parametrize('clip', FLAGS)
@pytest.mark.parametrize('tag', list('SMT'))
def test_pool_image_into_writes_its_columns_only(tag, clip):
    from qtmpnn import ops
    ms = mesh_of(tag)
    lab, nv, B, P = _labels(ms), _nv(ms), ms.B, ms.P
    rng = np.random.default_rng(12)
    with _flag(clip):
        for S, C in ((2, 3), (1, 4), (3, 1)):
            x = _draw(rng, B, S + 1, P, C)
            for strided in (False, True):
                img = _t(x)[:, :S] if strided else _t(x[:, :S])
                out = torch.full((S, ms.N, 7), SENT, device=dev())
                ops.pool_image_into(img, ms, out, coff=3, mean=True)
                ref, mag = M.pool(x[:, :S], lab, nv, True)
                check(f'pool_into {tag} clip={int(clip)} S={S} C={C} strided={int(strided)}', out[:, :nv, 3:3 + C], ref, mag)
                o = _np(out)
                assert (o[:, :, :3] == SENT).all() and (o[:, :, 3 + C:] == SENT).all(), 'a column outside [coff, coff + C) was written'
                assert (o[:, nv:] == SENT).all(), 'a capacity row was written'


# ------------------------------------------------------------------------------------------------------------ gather_pixels
@pytest.mark.parametrize('clip', FLAGS)
@pytest.mark.parametrize('C', [1, 4, 20])
@pytest.mark.parametrize('tag', list('SCDMTP'))
def test_gather_pixels_forward_and_backward(tag, C, clip):
    from qtmpnn import ops
    ms = mesh_of(tag)
    lab, nv = _labels(ms), _nv(ms)
    rng = np.random.default_rng(13 + C)
    v = _draw(rng, nv, C)
    g = _draw(rng, ms.B, ms.P, C)
    with _flag(clip):
        val = _rows(ms, v).requires_grad_(True)
        img = ops.gather_pixels(val, ms)
        same_bits(f'gather {tag} C={C} clip={int(clip)}', img, M.gather(v, lab)[0])
        (gv,) = torch.autograd.grad(img, val, _t(g))
        ref, mag = M.pool(g[:, None], lab, nv, False)
        check(f'gather {tag} C={C} clip={int(clip)} grad', gv[:nv], ref[0], mag[0])


# ---------------------------------------------------------------------------------------------------------- remesh_transfer
def _pair(name):
    if name == 'R':
        return mesh_of('R')
    return mesh_of(name, 0), mesh_of(name, 1)


def _remesh_case(nm, old, new, widths_in, widths_out, rng, views):
    """One transfer of the column parts `widths_in` (row-strided column views of one wide matrix when `views`), returned as
    `widths_out` (None: one matrix), forward and backward against the model."""
    from qtmpnn import ops
    lo, ln, no, nn_ = _labels(old), _labels(new), _nv(old), _nv(new)
    C = sum(widths_in)
    v = _draw(rng, no, C)
    g = _draw(rng, nn_, C)
    if views:
        wide = _rows(old, np.concatenate([_draw(rng, no, 4), v, _draw(rng, no, 4)], axis=1))
        offs = np.cumsum([4] + list(widths_in))
        parts = [wide[:, a:a + w].requires_grad_(True) for a, w in zip(offs, widths_in)]
        assert all(not p.is_contiguous() for p in parts)
    else:
        offs = np.cumsum([0] + list(widths_in))
        parts = [_rows(old, v[:, a:a + w]).requires_grad_(True) for a, w in zip(offs, widths_in)]
    arg = parts[0] if len(parts) == 1 else parts
    outs = ops.remesh_transfer(arg, old, new, widths_out)
    outs_l = [outs] if widths_out is None else list(outs)
    assert [o.shape[1] for o in outs_l] == (list(widths_out) if widths_out is not None else [C])
    ref, mag = M.remesh(v, lo, ln, nn_)
    check(nm, torch.cat([o[:nn_] for o in outs_l], dim=1), ref, mag)
    go = np.cumsum([0] + [o.shape[1] for o in outs_l])
    grads = torch.autograd.grad(outs_l, parts, [_rows(new, g[:, a:b]) for a, b in zip(go[:-1], go[1:])])
    gref, gmag = M.remesh_t(g, lo, ln, no)
    check(nm + ' grad', torch.cat([x[:no] for x in grads], dim=1), gref, gmag)


@pytest.mark.parametrize('clip', FLAGS)
@pytest.mark.parametrize('pair', ['S', 'D', 'M', 'T', 'R'])
def test_remesh_transfer_forward_and_backward(pair, clip):
    """ops.remesh_transfer old -> new and its transpose: one 8-wide matrix; the bench's 68-column state as five row-strided column
    views in and five parts out; odd widths (qt_pool through _RemeshOne); nine 4-wide parts into one matrix (the run-splitting
    branch).  Pair R: the new mesh was decomposed from the old one's node values, so with the general kernels its single-pixel
    nodes are k_pool_nodes' direct copies, both ways."""
    from qtmpnn import ops
    old, new = _pair(pair)
    rng = np.random.default_rng(21)
    with _flag(clip):
        assert ops.clip_remesh_ok(old, new) == clip
        tg = f'remesh {pair} clip={int(clip)}'
        _remesh_case(f'{tg} [8]', old, new, [8], None, rng, False)
        _remesh_case(f'{tg} [4,16,16,16,16] views', old, new, [4, 16, 16, 16, 16], [4, 16, 16, 16, 16], rng, True)
        _remesh_case(f'{tg} [3]', old, new, [3], None, rng, False)
        _remesh_case(f'{tg} [5]', old, new, [5], None, rng, False)
        _remesh_case(f'{tg} 9x[4]', old, new, [4] * 9, None, rng, False)


@pytest.mark.parametrize('pair', ['D', 'M', 'T', 'R'])
def test_remesh_transfer_assembles_the_decoder_input(pair):
    """dec_input=True (the tile-resident transfer only): part 0 comes back as [transferred value | new.posfeat], columns 1..3 bit for
    bit, and only column 0 of part 0 carries a gradient back -- as the scalar chunk on its own and riding with a second part."""
    from qtmpnn import ops
    old, new = _pair(pair)
    lo, ln, no, nn_ = _labels(old), _labels(new), _nv(old), _nv(new)
    rng = np.random.default_rng(22)
    pf = _np(new.posfeat)[:nn_]
    for widths in ([4], [4, 16, 16]):
        C = sum(widths)
        v, g = _draw(rng, no, C), _draw(rng, nn_, C)
        offs = np.cumsum([0] + widths)
        parts = [_rows(old, v[:, a:b]).requires_grad_(True) for a, b in zip(offs[:-1], offs[1:])]
        with _flag(True):
            outs = ops.remesh_transfer(parts, old, new, widths, dec_input=True)
        ref, mag = M.remesh(v, lo, ln, nn_)
        nm = f'dec_input {pair} {widths}'
        check(nm + ' value', torch.cat([outs[0][:nn_, :1]] + [o[:nn_] for o in outs[1:]], dim=1), ref[:, [0] + list(range(4, C))],
              mag[:, [0] + list(range(4, C))])
        same_bits(nm + ' posfeat', outs[0][:nn_, 1:], pf)
        with _flag(True):
            grads = torch.autograd.grad(list(outs), parts, [_rows(new, g[:, a:b]) for a, b in zip(offs[:-1], offs[1:])])
        g0 = g.copy()
        g0[:, 1:4] = 0.0
        gref, gmag = M.remesh_t(g0, lo, ln, no)
        check(nm + ' grad', torch.cat([x[:no] for x in grads], dim=1), gref, gmag)
        assert (_np(grads[0])[:no, 1:] == 0).all()


@pytest.mark.parametrize('tag', ['D', 'T'])
def test_decoder_input_on_its_own(tag):
    from qtmpnn import ops
    ms = mesh_of(tag)
    nv = _nv(ms)
    rng = np.random.default_rng(23)
    v, g = _draw(rng, nv, 8), _draw(rng, nv, 4)
    pf = _np(ms.posfeat)[:nv]
    for view in (False, True):
        val = (_rows(ms, v)[:, 4:8] if view else _rows(ms, v[:, 4:8])).requires_grad_(True)
        out = ops.decoder_input(val, ms)
        same_bits(f'decoder_input {tag} view={int(view)}', out[:nv], M.decoder_input(v[:, 4:8], pf)[0])
        (gv,) = torch.autograd.grad(out, val, _rows(ms, g))
        same_bits(f'decoder_input {tag} view={int(view)} grad', gv[:nv], M.decoder_input_t(g)[0])


# --------------------------------------------------------------------------------------------------------------------- loss
def _keep(ms):
    return None if ms.loss_mask is None else (_np(ms.loss_mask).reshape(-1) == 0)


@pytest.mark.parametrize('clip', FLAGS)
@pytest.mark.parametrize('tag', list('SDMTH'))
def test_step_sse_total_and_gradient(tag, clip):
    """ops.step_sse_partials / step_sse of one step: `out` as an (N, 1) tensor and as column 0 of a contiguous (N, 4) matrix (the
    gradient is then full rows, columns 1..3 exactly 0), y as a strided step view of (B, T, W, H, 1).  Static mesh: NaN in the
    capacity rows of `out`."""
    from qtmpnn import ops
    ms = mesh_of(tag)
    lab, nv, B = _labels(ms), _nv(ms), ms.B
    rng = np.random.default_rng(31)
    o = _draw(rng, nv, 4)
    yy = _draw(rng, B, 3, ms.n, ms.m, 1)
    y = _t(yy)[:, 1]
    assert not y.is_contiguous() or B == 1
    gs = np.float32(0.37)
    with _flag(clip):
        for wide in (False, True):
            if wide:
                base = _rows(ms, o).requires_grad_(True)
                out = base[:, :1]
            else:
                base = _rows(ms, o[:, :1]).requires_grad_(True)
                out = base
            part = ops.step_sse_partials(out, y, ms)
            total, tmag, gref, gmag = M.sse(o[:, 0], lab, yy[:, 1], _keep(ms), g=float(gs), W=4 if wide else 1)
            nm = f'step_sse {tag} clip={int(clip)} wide={int(wide)}'
            check(nm + ' total', part.double().sum().reshape(1), [total], [tmag])
            (gb,) = torch.autograd.grad(part.sum() * float(gs), base)
            check(nm + ' grad', gb[:nv], gref, gmag)
            if wide:
                assert (_np(gb)[:nv, 1:] == 0).all()
        if ms.loss_mask is None:
            base = _rows(ms, o[:, :1])
            check(f'step_sse {tag} clip={int(clip)} sum', ops.step_sse(base, y, ms).reshape(1), [total], [tmag])


def _step_meshes(tag, T, static):
    """T meshes of kind `tag`, every one decomposed from its own image (the criterion perturbed per step), node counts all different."""
    from qtmpnn.mesh import build_mesh
    key = ('steps', tag, T, static)
    if key not in _CACHE:
        base = _crit(tag, 0)
        rng = np.random.default_rng(41)
        out, seen = [], set()
        for t in range(T):
            for _ in range(8):             # (another patch position when the node count repeats an earlier step's)
                c = base.copy()
                for b in range(c.shape[0]):
                    r, q = rng.integers(0, c.shape[1] - 4), rng.integers(0, c.shape[2] - 4)
                    c[b, r:r + 1 + t % 4, q:q + 2] = 1.0
                ms = build_mesh(src=_t(c), thresh=0.5, mask=_mask(tag), static=static)
                if ms.n_valid not in seen:
                    break
            seen.add(ms.n_valid)
            out.append(ms)
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize('static', [False, True])
@pytest.mark.parametrize('tag', ['M', 'D'])
def test_rollout_sse_over_two_launches(tag, static):
    """_RolloutLoss 'sse' (qt_sse_rollout / _bwd) over T_out = 18 steps = two launches (16 + 2), a different mesh at every step, outputs
    (N_t, 4): the total, every step's own partial sums (a step that wrote into another step's slots shows there) and every step's
    gradient rows.  M: B = 2, P = 15000 = 14 * 1024 + 664; D: B = 3.  Static: capacity rows of the outputs hold NaN."""
    from qtmpnn import ops
    T = 18
    meshes = _step_meshes(tag, T, static)
    B, P = meshes[0].B, meshes[0].P
    nvs = [_nv(ms) for ms in meshes]
    assert len(set(nvs)) == T, 'every step has a mesh of its own size'
    assert (not static) or all(ms.n_dev is not None and ms.n_valid < ms.N for ms in meshes)
    rng = np.random.default_rng(42)
    os_ = [_draw(rng, nv, 4) for nv in nvs]
    yy = _draw(rng, B, T, meshes[0].n, meshes[0].m, 1)
    bases = [_rows(ms, o).requires_grad_(True) for ms, o in zip(meshes, os_)]
    outs = [b[:, :1] for b in bases]
    part = ops.rollout_sse_partials(outs, _t(yy), meshes)
    assert part is not None and part.shape == (T, B * -(-P // 1024))
    gs = np.float32(0.37)
    grads = torch.autograd.grad(part.sum() * float(gs), bases)
    tot, nm = 0.0, f'rollout_sse {tag} static={int(static)}'
    pt = _np(part.double().sum(dim=1))
    step_tot = []
    for t, ms in enumerate(meshes):
        total, tmag, gref, gmag = M.sse(os_[t][:, 0], _labels(ms), yy[:, t], None, g=float(gs), W=4)
        step_tot.append(total)
        tot += total
        check(f'{nm} grad t={t}', grads[t][:nvs[t]], gref, gmag)
    check(f'{nm} per-step partial sums', pt, step_tot, step_tot)
    check(f'{nm} total', part.double().sum().reshape(1), [tot], [tot])


@pytest.mark.parametrize('form', ['rollout', 'per_step'])
@pytest.mark.parametrize('tag', ['D', 'M', 'H'])
def test_masked_mse_divisor(tag, form):
    """model.mpnnlstm.masked_mse == model total / (B * T * n_valid) in float64, n_valid the unmasked pixels of a frame: through the
    rollout launches, and through the per-step fallback (forced by a y that is not contiguous: every second step of a longer
    tensor).  H goes step by step in both forms (loss_mask)."""
    from model.mpnnlstm import masked_mse
    from qtmpnn import ops
    ms = mesh_of(tag)
    B, T, nv, lab = ms.B, 3, _nv(ms), _labels(ms)
    mask = {'D': None, 'M': _mask('M'), 'H': golden('fixed_homog48x64.npz')['mask']}[tag]
    n_valid = ms.P if mask is None else int((~np.asarray(mask, bool)).sum())
    rng = np.random.default_rng(51)
    os_ = [_draw(rng, nv, 4) for _ in range(T)]
    yy = _draw(rng, B, 2 * T, ms.n, ms.m, 1)
    if form == 'rollout':
        y, ysel = _t(yy[:, ::2]), yy[:, ::2]
    else:
        y, ysel = _t(yy)[:, ::2], yy[:, ::2]
        assert not y.is_contiguous()
    outs = [_t(o)[:, :1] for o in os_]
    took = ops.rollout_sse_partials(outs, y, [ms] * T) is not None
    assert took == (form == 'rollout' and tag != 'H')
    loss = masked_mse(outs, [ms] * T, y, mask)
    keep = None if tag != 'H' else ~np.asarray(mask, bool).reshape(-1)
    tot = sum(M.sse(os_[t][:, 0], lab, ysel[:, t], keep)[0] for t in range(T))
    ref = tot / float(B * T * n_valid)
    check(f'masked_mse {tag} {form}', loss.reshape(1), [ref], [ref])


# -------------------------------------------------------------------------------------------------------- gather_frame_into
@pytest.mark.parametrize('tag', ['P', 'M', 'T'])
def test_gather_frame_into_its_slot(tag):
    """ops.gather_frame_into writes slots 0 and T - 1 of a (B, T, n, m, 1) stack and nothing else; pixels without a node get NaN on
    the masked pixelwise mesh and 0.0 elsewhere; `val` is read in place as a column of a 4-wide matrix.  On the static mesh a
    device node count smaller than the labels' range gives the pixels of the rows beyond it the fill."""
    from qtmpnn import ops
    ms = mesh_of(tag)
    lab, nv, B, T = _labels(ms), _nv(ms), ms.B, 4
    fill = np.nan if tag == 'P' else 0.0
    assert (lab < 0).any() or tag == 'T'
    rng = np.random.default_rng(61)
    v = _draw(rng, nv, 4)
    counts = [nv]
    meshes = [ms]
    if tag == 'T':
        stale = copy.copy(ms)
        stale.n_dev = torch.tensor([nv - 300], dtype=torch.int32, device=dev())
        meshes.append(stale)
        counts.append(nv - 300)
        assert (lab >= nv - 300).any()
    for mesh, cnt in zip(meshes, counts):
        for col in (0, 2):
            out = torch.full((B, T, ms.n, ms.m, 1), SENT, device=dev())
            val = _rows(ms, v)[:, col:col + 1]
            assert val.stride(0) == 4
            for t in (0, T - 1):
                ops.gather_frame_into(val, mesh, out, t)
            ref = M.frame(v[:, col:col + 1], lab, cnt, fill)[0]
            o = _np(out).reshape(B, T, ms.P, 1)
            same_bits(f'gather_frame {tag} count={cnt} col={col} t=0', o[:, 0], ref)
            same_bits(f'gather_frame {tag} count={cnt} col={col} t={T - 1}', o[:, T - 1], ref)
            assert (o[:, 1:T - 1] == SENT).all(), 'a slot that was not asked for was written'
