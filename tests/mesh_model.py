"""The host model of a batched quadtree mesh: what qtmpnn.mesh.build_mesh must return, assembled from per-clip walks of the oracle.

Plain numpy; nothing of qtmpnn is imported.  The decomposition itself is oracle/qt_oracle.py::quadtree_decompose, the sequential
LIFO walk that tests/test_oracle_golden.py pins to the reference's own output; this module only adds what a BATCH of clips needs
(clip offsets, the first label of every base cell, levels, cell records, pixel counts, positional features, the direct row
indices of a re-mesh) and the table of cases that both tests/test_mesh_model_host.py and tests/test_gpu_mesh_oracle.py walk.

Threshold.  The split test is strict (`>` / `<`) and the kernels make it in float32.  The model therefore casts `thresh` to
np.float32 before the walk: a float32 pixel against a Python float compares in float64 under numpy 1.x's value-based casting and
in float32 under numpy 2's weak scalars, so a threshold that float32 cannot hold (0.1) would decide ties differently from one numpy
to the next.  Images are cast to float32 for the same reason.

The module also holds `local_walk`, a deliberately parametrised restatement of the walk with one flag per hazard (HAZARDS).  With
no flag it must equal the oracle on every case of the table; with a flag, the cases designated for that hazard must give other
labels.  It exists so that the host test can prove that the cases bite -- it is never compared with the device.
"""
from types import SimpleNamespace

import numpy as np

from oracle import qt_oracle as O

CONDITIONS = O.CONDITIONS
U = 2.0 ** -24          # unit roundoff of float32

HAZARDS = {
    'window_s': 'split window of s x s instead of (s + 1) x (s + 1)',
    'ge': '>= for > (<= for <): a value equal to the threshold splits',
    'zero_pad': 'zero padding to the base grid instead of replicate padding',
    'child_order': 'children visited in another order (the two middle ones swapped)',
    'mask_window_s': 'mask / high-interest window of s x s instead of (s + 1) x (s + 1)',
    'mask_multi': 'mask test on the head pixel of a cell of any side, not only of side 1: the cell is dropped whole',
}


def dist_from_05(arr):
    return abs(abs(arr - 0.5) - 0.5)


def cdiv(a, b):
    return -(a // -b)


# ----------------------------------------------------------------------------------------------------------------- the walks
def walk(img, thresh, max_size, mask=None, hir=None, condition='max_larger_than', transform=None):
    """(labels (n, m), cells (N, 3) = (x, y, s) in label order) of one clip: the oracle's walk, threshold and image in float32."""
    return O.quadtree_decompose(np.asarray(img, np.float32), thresh=np.float32(thresh), max_size=max_size, mask=mask,
                                high_interest_region=hir, transform_func=transform, condition=condition, return_cells=True)


def local_walk(img, thresh, max_size, mask=None, hir=None, condition='max_larger_than', transform=None, hazard=None):
    """Labels of one clip by a walk of this module's own; `hazard` (a key of HAZARDS) makes it wrong in that one way."""
    assert hazard is None or hazard in HAZARDS
    img, thresh = np.asarray(img, np.float32), np.float32(thresh)
    n, m = img.shape
    n_pad, m_pad = cdiv(n, max_size) * max_size, cdiv(m, max_size) * max_size
    if n_pad > m_pad:
        raise IndexError('more base rows than base columns')
    crit = np.pad(img, ((0, n_pad - n), (0, m_pad - m)), mode='constant' if hazard == 'zero_pad' else 'edge')
    if transform is not None:
        crit = transform(crit)
    e = 0 if hazard == 'window_s' else 1
    em = 0 if hazard == 'mask_window_s' else 1
    red = np.max if condition.startswith('max') else np.min
    if condition.endswith('larger_than'):
        hit = (lambda v: v >= thresh) if hazard == 'ge' else (lambda v: v > thresh)
    else:
        hit = (lambda v: v <= thresh) if hazard == 'ge' else (lambda v: v < thresh)
    forcing = [a for a in (mask, hir) if a is not None]
    labels = np.full((n, m), -1, np.int64)
    nxt = 0
    stack = [(bi * max_size, bj * max_size, max_size) for bi in range(n_pad // max_size) for bj in range(m_pad // max_size)]
    while stack:
        x, y, s = stack.pop()
        if x >= n or y >= m:
            continue
        if mask is not None and mask[x, y] and (s == 1 or hazard == 'mask_multi'):
            continue
        if s > 1 and (hit(red(crit[x:x + s + e, y:y + s + e])) or any(f[x:x + s + em, y:y + s + em].any() for f in forcing)):
            h = s // 2
            kids = [(x, y, h), (x + h, y, h), (x, y + h, h), (x + h, y + h, h)]
            if hazard == 'child_order':
                kids[1], kids[2] = kids[2], kids[1]
            stack.extend(kids)
            continue
        labels[x:x + s, y:y + s] = nxt
        nxt += 1
    return labels


# ----------------------------------------------------------------------------------------------------------------- the model
def assemble(walks, n, m, max_size, size_norm=None):
    """The batched mesh of B per-clip walks [(labels (n, m), cells (N_b, 3)), ...]:

      N, B, n, m, max_size
      labels   (B, n, m) int64   clip-global node row of every pixel, -1 = no node
      node_off (B + 1)           first label of every clip, node_off[B] = N
      cell_off (B * nbase + 1)   first label of every base cell in label order: slot b * nbase + j belongs to base cell
                                 nbase - 1 - j of clip b (base cells are walked in reverse row-major order); a base cell without a
                                 node repeats the next slot's value; the last slot is N
      level    (B, n, m) uint8   log2 of the side of the leaf that owns the pixel (0 for a masked pixel: the walk reaches side 1)
      cell     (N, 4)            (row, col, s, clip) of every node -- s from the walk, not from the pixels
      npix     (N)               pixels of the node inside the frame
      posfeat  (N, 3) float64    (mean column / m, mean row / n, npix / size_norm), means over the node's pixels
    """
    B = len(walks)
    nbj = cdiv(m, max_size)
    nbase = cdiv(n, max_size) * nbj
    size_norm = (max_size / 2) ** 2 if size_norm is None else size_norm
    node_off = np.zeros(B + 1, np.int64)
    node_off[1:] = np.cumsum([len(c) for _, c in walks])
    N = int(node_off[-1])
    labels = np.stack([np.where(lab >= 0, lab + node_off[b], -1) for b, (lab, _) in enumerate(walks)]).astype(np.int64)
    cell = np.concatenate([np.concatenate([c, np.full((len(c), 1), b, np.int64)], axis=1) for b, (_, c) in enumerate(walks)]
                          + [np.zeros((0, 4), np.int64)])
    cell_off = np.empty(B * nbase + 1, np.int64)
    for b, (_, c) in enumerate(walks):
        per_base = np.bincount((c[:, 0] // max_size) * nbj + c[:, 1] // max_size, minlength=nbase)
        cell_off[b * nbase:(b + 1) * nbase] = node_off[b] + np.cumsum(per_base[::-1]) - per_base[::-1]
    cell_off[-1] = N
    lv = np.round(np.log2(np.maximum(cell[:, 2], 1))).astype(np.uint8)
    assert N == 0 or ((1 << lv.astype(np.int64)) == cell[:, 2]).all()
    level = np.where(labels >= 0, lv[np.maximum(labels, 0)] if N else 0, 0).astype(np.uint8)
    ok = labels >= 0
    _, rr, cc = np.meshgrid(np.arange(B), np.arange(n), np.arange(m), indexing='ij')
    npix = np.bincount(labels[ok], minlength=N).astype(np.int64)
    mean_c = np.bincount(labels[ok], weights=cc[ok].astype(np.float64), minlength=N) / np.maximum(npix, 1)
    mean_r = np.bincount(labels[ok], weights=rr[ok].astype(np.float64), minlength=N) / np.maximum(npix, 1)
    posfeat = np.stack([mean_c / m, mean_r / n, npix / float(size_norm)], axis=1)
    return SimpleNamespace(N=N, B=B, n=n, m=m, max_size=max_size, nbase=nbase, labels=labels, node_off=node_off, cell_off=cell_off,
                           level=level, cell=cell, npix=npix, posfeat=posfeat)


def model_of(imgs, max_size, thresh, condition='max_larger_than', mask=None, hir=None, transform=None, size_norm=None):
    """The model of build_mesh(src=imgs (B, n, m), ...): one oracle walk per clip, assembled."""
    imgs = np.asarray(imgs, np.float32)
    walks = [walk(im, thresh, max_size, mask, hir, condition, transform) for im in imgs]
    return assemble(walks, imgs.shape[1], imgs.shape[2], max_size, size_norm)


def remesh_criterion(nodeval, old_labels):
    """(B, n, m) float32 image that build_mesh(prev=(nodeval, old)) decomposes: O.unflatten of the node values on the old labels;
    masked pixels read 0."""
    import torch
    data = torch.from_numpy(np.ascontiguousarray(np.asarray(nodeval, np.float32).reshape(-1, 1)))
    return O.unflatten(data, np.array(old_labels), tuple(old_labels.shape)).numpy()[..., 0]


def remesh_indices(old, new):
    """(fwd_src (new.N), bwd_src (old.N)): fwd_src[i] = the old label under new node i if that node is a leaf of side 1, else -1;
    bwd_src[j] = the new label under old node j if that node is a leaf of side 1, else -1.  A masked pixel gives -1 for either.
    A leaf of a larger side that the frame border clips to one pixel counts as larger: -1 sends a row down the general path."""
    def under(a, b):
        out = np.full(a.N, -1, np.int64)
        one = a.cell[:, 2] == 1
        c = a.cell[one]
        out[one] = b.labels[c[:, 3], c[:, 0], c[:, 1]]
        return out
    return under(new, old), under(old, new)


def posfeat_bound(model):
    """|device - model| per entry of posfeat.  Each channel is one float32 division of operands that float32 holds exactly (a
    half-integer mean below 2^12 or a pixel count, over m, n or a power of two): one rounding, U relative, doubled for the
    float64 quotient's own representation."""
    return 2.0 * U * np.abs(model.posfeat)


# ----------------------------------------------------------------------------------------------------------------- the cases
FRAMES = [(24, 32), (33, 65), (50, 70), (64, 40), (64, 64), (65, 129), (80, 150), (100, 100), (128, 128)]
MAX_SIZES = [2, 4, 8, 16, 32, 64]


def _rng(*key):
    # (strings are spelt out as bytes: hash() of a str changes from process to process)
    return np.random.default_rng([b for k in key for b in (list(str(k).encode()) + [255])])


def img_blob(rng, n, m):
    a = np.zeros((n, m), np.float32)
    blk = a[n // 3:n // 3 + 9, m // 2:m // 2 + 13]
    blk[...] = 0.625 + 0.375 * rng.random(blk.shape)
    return a


def img_scattered(rng, n, m):
    return (rng.random((n, m)) < 0.03).astype(np.float32)


def img_quantised(rng, n, m, condition):
    """Multiples of 1/8 around thresh = 0.5 with ties (for the min_* conditions some values negative).  Where a tie must not split
    (`>` / `<` is strict) it sits among values of the side that decides the other way, so that `>=` / `<=` changes the labels."""
    side = -1.0 if condition in ('max_larger_than', 'max_smaller_than') else 1.0          # where the bulk lies
    tie_stops = condition in ('max_smaller_than', 'min_larger_than')                      # a tie is what keeps a window whole
    u = rng.integers(1, 9, (n, m)) / 8.0
    a = 0.5 + side * u
    if tie_stops:
        # the bulk splits down to pixels; a handful of pixels ON the threshold (and, for min_larger_than, a few negative ones)
        # keep the windows that hold them whole -- more of them and no window of a large base cell would split at all
        spots = rng.permutation(n * m)[:7]
        a.reshape(-1)[spots[:4]] = 0.5
        if condition == 'min_larger_than':
            a.reshape(-1)[spots[4:]] = -0.25
        return a.astype(np.float32)
    a[rng.random((n, m)) < 0.1] = 0.5
    far = rng.random((n, m)) < 0.02
    if condition == 'max_larger_than':
        a[far] = 0.5 + rng.integers(1, 5, int(far.sum())) / 8.0
    else:
        a[far] = 0.5 - rng.integers(1, 13, int(far.sum())) / 8.0                          # min_smaller_than: down to -1
    return a.astype(np.float32)


def _case(name, imgs, max_size, thresh=0.5, condition='max_larger_than', mask=None, hir=None, transform=False, quads=None,
          props=(), detects=()):
    imgs = np.ascontiguousarray(imgs, np.float32)
    _, n, m = imgs.shape
    tall = cdiv(n, max_size) > cdiv(m, max_size)
    return SimpleNamespace(name=name, imgs=imgs, B=imgs.shape[0], n=n, m=m, max_size=max_size, thresh=thresh, condition=condition,
                           mask=mask, hir=hir, transform=transform, quads=quads, props=tuple(props) + (('tall',) if tall else ()),
                           detects=tuple(detects), tall=tall, key=name)


def _with_quads(c):
    """A max_size 64 case twice: stage 1 with one workgroup per 32 x 32 quadrant (the default) and with one per base cell.  Both
    share one model (key)."""
    if c.max_size != 64:
        return [c]
    out = []
    for q in (True, False):
        d = SimpleNamespace(**vars(c))
        d.quads, d.name = q, f'{c.name}-q{int(q)}'
        out.append(d)
    return out


def _grid_case(n, m, ms):
    """Five clips: all zero | all above the threshold | one blob | scattered pixels | quantised with ties."""
    rng = _rng('grid', n, m, ms)
    imgs = np.stack([np.zeros((n, m), np.float32), np.ones((n, m), np.float32), img_blob(rng, n, m), img_scattered(rng, n, m),
                     img_quantised(rng, n, m, 'max_larger_than')])
    props = ['unsplit_base', 'per_pixel_clip1', 'tie']
    if n % ms or m % ms:
        props.append('clipped')
    if n < ms or m < ms:
        props.append('narrow')
    if n % ms == 1 or m % ms == 1:
        props.append('sliver')
    if 0 < n % ms <= ms // 2 or 0 < m % ms <= ms // 2:
        props.append('outside_quadrant')
    if ms == 64:
        props.append('level6')
    return _case(f'grid-{n}x{m}-ms{ms}', imgs, ms, props=props, detects=('child_order', 'ge'))


def _hot_case(n, m, ms):
    """One hot pixel per clip: last row | last column | column ms of base cell (0, 0)'s window, which is the first column of the
    neighbouring base cell | the window's far corner (ms, ms)."""
    imgs = np.zeros((4, n, m), np.float32)
    imgs[0, n - 1, m // 3] = 1.0
    imgs[1, n // 3, m - 1] = 1.0
    imgs[2, 1, ms] = 1.0
    imgs[3, ms, ms] = 1.0
    return _case(f'hot-{n}x{m}-ms{ms}', imgs, ms, props=('hot_outside_cell00', 'clipped'), detects=('window_s',))


def _build_cases():
    cases = []
    # ---- frames x max_size (the combinations with more base rows than columns are the refusal cases)
    for n, m in FRAMES:
        for ms in MAX_SIZES:
            cases += _with_quads(_grid_case(n, m, ms))
    # ---- ties under all four conditions
    for (n, m), ms in (((50, 70), 16), ((65, 129), 64), ((100, 100), 4), ((33, 65), 32)):
        for cond in CONDITIONS:
            rng = _rng('cond', n, m, ms, cond)
            imgs = np.stack([img_quantised(rng, n, m, cond) for _ in range(3)])
            props = ['tie'] + (['negative'] if cond.startswith('min') else [])
            if (n % ms or m % ms) and cond in ('max_larger_than', 'min_smaller_than'):     # (the other two split the border to pixels)
                props.append('clipped')
            # child order: the conditions whose bulk stays whole leave trees of several depths.  Zero padding: under
            # min_larger_than every in-frame value but a few is > 0.5, so a padded 0 is what keeps a border window whole
            det = ('ge',) + (('child_order',) if cond in ('max_larger_than', 'min_smaller_than') else ())
            if cond == 'min_larger_than' and (n % ms or m % ms):
                det += ('zero_pad',)
            cases += _with_quads(_case(f'cond-{n}x{m}-ms{ms}-{cond}', imgs, ms, condition=cond, props=props, detects=det))
    # ---- a single hot pixel
    for (n, m), ms in (((50, 70), 8), ((50, 70), 16), ((65, 129), 64), ((100, 100), 32), ((33, 65), 2)):
        cases += _with_quads(_hot_case(n, m, ms))
    # ---- thresholds that no value reaches: +inf (the preset meshes) and -inf
    rng = _rng('inf')
    mk = np.zeros((50, 70), bool)
    mk[20:27, 3:23] = True
    hr = np.zeros((50, 70), bool)
    hr[5:9, 58:68] = True
    cases.append(_case('inf-50x70-ms4', rng.random((3, 50, 70)), 4, thresh=np.inf, props=('all_base',)))
    cases.append(_case('inf-50x70-ms4-masked', rng.random((3, 50, 70)), 4, thresh=np.inf, mask=mk, hir=hr, props=('masked', 'clipped')))
    cases += _with_quads(_case('inf-64x64-ms64', rng.random((3, 64, 64)), 64, thresh=np.inf, props=('all_base', 'level6')))
    cases += _with_quads(_case('neginf-64x64-ms64', rng.random((3, 64, 64)) - 0.5, 64, thresh=-np.inf, props=('per_pixel',)))
    cases.append(_case('neginf-24x32-ms8-max_smaller', rng.random((3, 24, 32)), 8, thresh=-np.inf, condition='max_smaller_than',
                       props=('all_base',)))
    # ---- masks and high-interest regions
    for (n, m), ms in (((64, 150), 64), ((50, 70), 16), ((33, 65), 32)):
        # a masked pixel that base cell (0, 0) sees only in the extra column (row) of its window
        for where, (r, c) in (('col', (1, ms)), ('row', (ms, 1))):
            if r >= n:
                continue
            rng = _rng('extra', n, m, ms)
            mk = np.zeros((n, m), bool)
            mk[r, c] = True
            imgs = np.stack([np.zeros((n, m), np.float32), img_blob(rng, n, m), np.zeros((n, m), np.float32)])
            cases += _with_quads(_case(f'maskextra-{where}-{n}x{m}-ms{ms}', imgs, ms, mask=mk, props=('mask_extra_only', 'masked'),
                                       detects=('mask_window_s',)))
    for ms in (64, 32):
        # one whole base cell and one whole 32 x 32 block under the mask: zero counts in the scan
        rng = _rng('whole', ms)
        mk = np.zeros((128, 128), bool)
        mk[0:64, 64:128] = True
        mk[64:96, 0:32] = True
        imgs = np.stack([np.zeros((128, 128), np.float32), img_scattered(rng, 128, 128), img_blob(rng, 128, 128)])
        cases += _with_quads(_case(f'maskwhole-128x128-ms{ms}', imgs, ms, mask=mk, props=('zero_counts', 'masked')))
    for (n, m), ms in (((64, 64), 64), ((100, 100), 16)):
        # a mask whose corner is the head pixel of a block that is only partly masked
        rng = _rng('head', n, m, ms)
        mk = np.zeros((n, m), bool)
        mk[32:39, 0:m // 3] = True
        imgs = np.stack([np.zeros((n, m), np.float32), img_scattered(rng, n, m), img_blob(rng, n, m)])
        cases += _with_quads(_case(f'maskhead-{n}x{m}-ms{ms}', imgs, ms, mask=mk, props=('masked_head', 'masked'),
                                   detects=('mask_multi', 'mask_window_s')))
    for (n, m), ms in (((64, 40), 64), ((50, 70), 8)):
        rng = _rng('hir', n, m, ms)
        hr = np.zeros((n, m), bool)
        hr[5:9, m - 12:m - 2] = True
        imgs = np.stack([np.zeros((n, m), np.float32), img_scattered(rng, n, m), img_blob(rng, n, m)])
        cases += _with_quads(_case(f'hir-{n}x{m}-ms{ms}', imgs, ms, hir=hr, props=('hir_only',), detects=('mask_window_s',)))
    for (n, m) in ((80, 150), (100, 100)):
        for ms in (64, 16):
            rng = _rng('both', n, m, ms)
            mk = np.zeros((n, m), bool)
            mk[n // 2:n // 2 + 7, 3:m // 3] = True
            hr = np.zeros((n, m), bool)
            hr[5:9, m - 12:m - 2] = True
            imgs = np.stack([np.zeros((n, m), np.float32), img_scattered(rng, n, m), img_blob(rng, n, m),
                             img_quantised(rng, n, m, 'max_larger_than')])
            cases += _with_quads(_case(f'both-{n}x{m}-ms{ms}', imgs, ms, mask=mk, hir=hr, props=('masked', 'clipped', 'tie'),
                                       detects=('mask_window_s', 'ge')))
    # ---- the transform path: the criterion is dist_from_05 of the edge-padded image
    for (n, m), ms in (((50, 70), 64), ((100, 100), 64), ((50, 70), 8)):
        rng = _rng('transform', n, m, ms)
        imgs = np.stack([rng.integers(0, 9, (n, m)) / 8.0 * (rng.random((n, m)) < 0.05) for _ in range(3)])
        cases += _with_quads(_case(f'transform-{n}x{m}-ms{ms}', imgs, ms, thresh=0.125, transform=True, props=('clipped',),
                                   detects=('ge', 'child_order')))
    return cases


_CASES = None
_MODELS = {}


def cases():
    """The case table, built once.  A case: name, imgs (B, n, m) float32, max_size, thresh, condition, mask, hir, transform (the
    criterion is dist_from_05 of the padded image), quads (max_size 64: which stage-1 kernel), props (the properties it is there
    for, asserted by the host test), detects (the hazards it is designated for), tall (the oracle refuses it with IndexError)."""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def model_for(c):
    """The model of a case of the table, computed once and never changed (the two stage-1 variants of a case share it)."""
    if c.key not in _MODELS:
        md = model_of(c.imgs, c.max_size, c.thresh, c.condition, c.mask, c.hir, dist_from_05 if c.transform else None)
        for a in vars(md).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _MODELS[c.key] = md
    return _MODELS[c.key]
