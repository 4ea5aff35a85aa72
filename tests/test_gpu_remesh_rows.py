"""csrc/remeshclip.hip, one workgroup per (clip, tile, 32 x 32 quadrant, column group of up to four float4 chunks), against the
general node / tile kernels of transfer.hip (ops._CLIP_REMESH = False), bit for bit, forward and backward, at B = 2.

The two families sum a node's pixels in different associations, so the operands are small integers: every partial sum (at most
4096 pixels x 8 x 8) is an exact float32 and every node of these meshes has a power-of-two pixel count, so 1 / npix scales
exactly -- the result does not depend on the association and the comparison is torch.equal.  (That the new organisation keeps the
association of the old one for arbitrary floats is what the bench's dumped loss / parameters / gradients pin.)"""
import numpy as np
import pytest
import torch

from helpers import dev

pytestmark = pytest.mark.gpu

B = 2


def _ints(rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (rows, width), generator=g).float().to(dev())


def _quadtree(img, mask=None):
    from qtmpnn.mesh import build_mesh
    return build_mesh(src=torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(dev()), thresh=0.5, mask=mask)


def _sparse(n, m, seed, p=0.03):
    rng = np.random.default_rng(seed)
    return (rng.random((B, n, m)) < p).astype(np.float32)


def _corner(n, m):
    """One pixel set in the frame's corner: the decomposition around it leaves nodes of every level 0 .. 5."""
    img = np.zeros((B, n, m), np.float32)
    img[:, 0, 0] = 1.0
    img[1, n - 1, m - 1] = 1.0
    return img


def _both(monkeypatch, old, new, win, wout, dec=False):
    """Values and gradients of the transfer old -> new on the clip-resident kernel and on the general kernels."""
    from qtmpnn import ops
    assert ops.clip_remesh_ok(old, new)
    parts = [_ints(old.N, w, 10 + i).requires_grad_(True) for i, w in enumerate(win)]
    gouts = [_ints(new.N, w, 20 + i) for i, w in enumerate(wout)]

    def run(clip):
        outs = list(ops.remesh_transfer(parts, old, new, wout, dec_input=dec and clip))
        if dec and not clip:                # (the general kernels do not assemble the decoder input: the separate op does)
            outs[0] = ops.decoder_input(outs[0], new)
        grads = torch.autograd.grad(outs, parts, gouts)
        return [o.detach() for o in outs] + list(grads)
    fast = run(True)
    monkeypatch.setattr(ops, '_CLIP_REMESH', False)
    ref = run(False)
    monkeypatch.undo()
    names = [f'out{i}' for i in range(len(wout))] + [f'grad{i}' for i in range(len(win))]
    for name, a, r in zip(names, fast, ref):
        bad = int((a != r).sum())
        print(f'{name}: {tuple(a.shape)} mismatches {bad}')
        assert torch.equal(a, r), f'{name}: {bad} of {a.numel()} values differ'
    return fast


STATE = ([4, 16, 16, 16, 16], [4, 16, 16, 16, 16])      # the benchmark's state: decoder input, H and C of two layers


def test_every_level_of_the_pyramid(monkeypatch):
    new = _quadtree(_corner(64, 64))
    assert set(range(6)) <= set(new.level.unique().tolist())
    old = _quadtree(_sparse(64, 64, 1))
    _both(monkeypatch, old, new, *STATE)
    _both(monkeypatch, new, old, *STATE)


def test_whole_tile_nodes(monkeypatch):
    one = _quadtree(np.zeros((B, 64, 64), np.float32))
    assert one.N == B and int(one.level.max()) == 6
    fine = _quadtree(_sparse(64, 64, 2))
    _both(monkeypatch, fine, one, *STATE)               # destination clip = one level-6 node (and its transposed transfer)
    _both(monkeypatch, one, fine, *STATE)               # source clip = one node
    _both(monkeypatch, one, one, *STATE)


@pytest.mark.parametrize('kind', ['pixelwise', 'preset'])
def test_source_range_wider_than_a_window(monkeypatch, kind):
    from qtmpnn.mesh import build_homogeneous_mesh, build_pixel_mesh
    if kind == 'pixelwise':
        src = build_pixel_mesh(B, 64, 64, device=dev())
    else:
        src = build_homogeneous_mesh(64, 64, 2, None, B=B, device=dev())         # raster order of 2 x 2 cells: no depth-first ranges
    lab = src.labels[0, 32:, 32:]
    span = int(lab.max()) - int(lab.min()) + 1
    assert span > lab.unique().numel()      # the quadrant's source rows are no contiguous range ...
    assert kind != 'pixelwise' or span > 1024                                       # ... and here wider than one window
    tree = _quadtree(_corner(64, 64))
    _both(monkeypatch, src, tree, *STATE)
    _both(monkeypatch, tree, src, *STATE)


@pytest.mark.parametrize('kind', ['quadrant', 'ends'])
def test_masked_pixels(monkeypatch, kind):
    mask = np.zeros((64, 64), bool)
    if kind == 'quadrant':
        mask[:32, 32:] = True               # a whole quadrant: no valid source row there
    else:
        mask[32, 0] = mask[63, 31] = True   # a quadrant's first and last pixel
    old = _quadtree(_sparse(64, 64, 3), mask)
    new = _quadtree(_corner(64, 64), mask)
    assert int((new.labels < 0).sum()) == B * int(mask.sum())
    pw = np.log2(torch.cat([old.npix, new.npix]).cpu().numpy())
    assert np.array_equal(pw, np.round(pw))             # (power-of-two pixel counts: the module docstring's exactness argument)
    _both(monkeypatch, old, new, *STATE)


def test_rider_and_narrow_groups(monkeypatch):
    old, new = _quadtree(_sparse(64, 64, 4)), _quadtree(_sparse(64, 64, 5, p=0.01))
    x = _both(monkeypatch, old, new, [4, 16, 16], [4, 16, 16], dec=True)
    assert torch.equal(x[0][:, 1:], new.posfeat) and bool((x[3][:, 1:] == 0).all())
    _both(monkeypatch, old, new, [8, 12], [4, 16])      # groups of 1, 1 and 3 chunks
    _both(monkeypatch, old, new, [8, 12], [12, 8])      # groups of 2, 1 and 2 chunks


def test_two_tiles(monkeypatch):
    old, new = _quadtree(_sparse(64, 128, 6)), _quadtree(_corner(64, 128))          # tiles_c = 2 (the cases above: 1)
    assert old.cell_off.numel() == 2 * B + 1
    _both(monkeypatch, old, new, *STATE)
