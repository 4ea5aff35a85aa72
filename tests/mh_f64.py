"""MHTransformerConv -- multi-head edge-softmax attention, the head merge and the attention coefficients -- restated in float64: the
checker of qt_mhattn_fwd / qt_mhattn_bwd_merge (csrc/mhattn.hip), of qt_attn_weights (csrc/attnw.hip) and of ops._MHAttention (tests
only; plain torch / numpy on the CPU, nothing of qtmpnn is imported).

Built on attn_f64.attention_f64(..., heads=H, gmod=0), whose `out` is the cat plane (N, H C):

    y      = cat Wt + blin                                    Wt (H C, C) = Wlin^T, blin (C)
    gcat   = g Wt^T                                           g (N, C) the incoming gradient
    stats  = (m, lsum)[h, i]: max_p s_p and sum_p exp(s_p - m) over the pairs of target i in head h (before dropout)
    alpha  = exp(s_p - m) / lsum                              the coefficients qt_attn_weights writes out

and the gradients of proj, We, Wt, blin by autograd, the dropout mask held constant.

Bounds, every majorant taken from the float64 reference alone (RTOL, ATOL: tests/helpers.py):
    cat    |err| <= RTOL absum                                 absum = sum_p alpha d |v_j + We a| + |skip_i| (attn_f64)
    y      |err| <= RTOL (absum |Wt| + |blin|)
    gcat   |err| <= RTOL |g| |Wt|^T
    m      |err| <= RTOL S_i,  S_i = max_p scale sum_c |q_ic| |k_jc + (We a)_c|: the maximum of perturbed scores moves by no more than
           the largest perturbation, and a float32 score carries a few C units of 2^-24 of its majorant
    lsum   |err| <= RTOL lsum (1 + 2 S_i): every term exp(s_p - m) moves by its own size times |ds_p| + |dm| <= 2 RTOL S_i, and the
           exponentials and their sum carry relative rounding far below RTOL
    alpha  |err| <= ATOL + RTOL alpha                          the project's comparison of coefficients (tests/test_gpu_attn_weights.py)
    gradients: helpers.grad_close with its defaults, d proj per block (q, k, v, skip) and head.

float32_outputs() runs the same statements in single precision (the yardstick: what plain float32 rounding costs under each bound),
and with `tamper` states one subtly wrong kernel each; tests/test_mh_f64_host.py shows that the clean form passes every checker and
every tampered one fails.  The checkers print their worst error / bound ratios before they assert."""
import inspect
import math
from types import SimpleNamespace

import numpy as np
import torch

from attn_f64 import attention_f64
from helpers import ATOL, RTOL, grad_close

MAX_HEADS = 4
HEADS = (1, 2, 3, 4)
WIDTHS = (4, 8, 16, 32)
MERGE_ROWS = 32            # rows per trip of k_mh_merge_bwd
MERGE_GRID = 256           # its grid cap: 256 x 32 = 8192 rows per sweep, the stride loop runs above that
SWEEP = MERGE_ROWS * MERGE_GRID

# ------------------------------------------------------------------------------------------------------------------ case table
# Meshes (tests/test_gpu_mh_f64.py builds them and asserts the properties): S 24 x 32, a last workgroup that is not full; D three
# 64 x 64 clips with a row of >= 32 edges, odd and even pair counts, nodes with and without a self pair; P pixelwise, no self pairs;
# T the static form of D (NaN in the capacity rows of every operand); L three all-pixel 64 x 64 clips, more than 8192 valid rows.
# (keep, device epoch, host seed) as tests/test_gpu_attn_f64.py deals them
DROPOUT = [(1.0, 7, 1), (0.9, 0, 0xDEADBEEF), (0.9, 1, 1234), (0.9, 7, 2654435768), (0.5, 0, 1234), (0.5, 1, 2654435768),
           (0.5, 7, 0xDEADBEEF)]


def _case(kind, C, H, c_real=None, keep=1.0, epoch=0, seed=1):
    c_real = c_real or C
    name = f'{kind}-C{C}-H{H}' + (f'-c{c_real}' if c_real != C else '') + (f'-keep{keep}-ep{epoch}-seed{seed}' if keep < 1 or epoch else '')
    return dict(name=name, kind=kind, C=C, c_real=c_real, H=H, keep=keep, epoch=epoch, seed=seed, opseed=1000 + 16 * C + H)


# through ops._MHAttention
APPLY_HEADS = [_case('D', C, H) for H in HEADS for C in WIDTHS]
APPLY_CREAL = [_case('D', 4, 3, c_real=1), _case('D', 8, 3, c_real=5)]
APPLY_MESHES = [_case(kind, C, H) for kind in 'SPTL' for C, H in ((16, 3), (32, 4))]
APPLY_DROPOUT = [_case(kind, 16, 3, keep=keep, epoch=epoch, seed=seed) for kind in 'DT' for keep, epoch, seed in DROPOUT]
# through the C ABI: (mesh, C, H)
RAW = [(kind, C, H) for kind in 'DTL' for C in (8, 32) for H in (3, 4)]
# qt_attn_weights at G = H = 3: (mesh, C) x layout
WEIGHTS = [('D', C) for C in WIDTHS] + [(kind, 16) for kind in 'SPT']
WEIGHTS_G = 3
LAYOUTS = ('rows', 'planes')
LD_G_EXTRA = 36            # the incoming gradient of the merge backward is a column block of a matrix C + 36 wide


def operands(N, C, c_real, H, opseed, qk=1.0, we=0.3, wt=0.3):
    """Host fp32 operands, zero above c_real as the callers pad them (tests/test_gpu_mh.py): proj (N, H 4C), We (H, C, 2),
    Wt (H C, C), blin (C), incoming gradients g, g2 (N, C)."""
    gen = torch.Generator().manual_seed(opseed)
    live = torch.zeros(C)
    live[:c_real] = 1.0
    P = torch.randn(N, H, 4, C, generator=gen)
    P[:, :, :2] *= qk
    proj = (P * live).reshape(N, H * 4 * C).contiguous()
    We = torch.randn(H, C, 2, generator=gen) * we * live.view(1, C, 1)
    Wt = (torch.randn(H, C, C, generator=gen) * wt * live.view(1, C, 1) * live.view(1, 1, C)).reshape(H * C, C).contiguous()
    blin = torch.randn(C, generator=gen) * live
    g = torch.randn(N, C, generator=gen) * live
    g2 = torch.randn(N, C, generator=gen) * live
    return SimpleNamespace(proj=proj, We=We, Wt=Wt, blin=blin, g=g, g2=g2)


# ------------------------------------------------------------------------------------------------------------------ the model
def model(rowptr, col, selfpair, eattr, proj, We, Wt, blin, c_real, heads, keep, seed, epoch, dtype=torch.float64):
    """-> namespace: att (attention_f64's), cat = att.out, y (N, C) attached to the leaves att.proj, att.We, Wt, blin; ybound (N, C);
    s, smaj (pairs, H): scores and their majorants; m, lsum, S (N, H): row maximum, sum of exp(s - m) and largest majorant per
    target (m = -inf, lsum = 0 where a target has no pair)."""
    att = attention_f64(rowptr, col, selfpair, eattr, proj, We, c_real, heads, keep, seed, epoch, 0, dtype)
    N, H, C = att.N, att.G, att.C
    Wt = torch.as_tensor(np.asarray(Wt)).to(dtype).reshape(H * C, C).clone().requires_grad_(True)
    blin = torch.as_tensor(np.asarray(blin)).to(dtype).reshape(C).clone().requires_grad_(True)
    y = att.out @ Wt + blin
    with torch.no_grad():
        ybound = att.absum @ Wt.abs() + blin.abs()
        tgt, src = torch.from_numpy(att.tgt), torch.from_numpy(att.src)
        attr = torch.zeros(len(att.tgt), 2, dtype=dtype)
        attr[:att.E] = torch.as_tensor(np.asarray(eattr)).to(dtype)[:att.E]
        P = att.proj.view(N, H, 4, C)
        q, ke = P[:, :, 0][tgt], P[:, :, 1][src] + torch.einsum('gck,pk->pgc', att.We, attr)
        scale = 1.0 / math.sqrt(c_real)
        s, smaj = (q * ke).sum(-1) * scale, (q.abs() * ke.abs()).sum(-1) * scale
        idx = tgt.unsqueeze(1).expand(-1, H)
        m = torch.full((N, H), -math.inf, dtype=dtype).scatter_reduce(0, idx, s, 'amax', include_self=True)
        S = torch.zeros(N, H, dtype=dtype).scatter_reduce(0, idx, smaj, 'amax', include_self=True)
        lsum = torch.zeros(N, H, dtype=dtype).index_add(0, tgt, torch.exp(s - m[tgt]))
    return SimpleNamespace(att=att, cat=att.out, y=y, Wt=Wt, blin=blin, ybound=ybound, s=s, smaj=smaj, m=m, lsum=lsum, S=S,
                           N=N, H=H, C=C, E=att.E, dtype=dtype)


def gradients(ref, g):
    """-> namespace of sum(y * g)'s gradients by autograd, the mask held constant: proj (N, H 4C), We (H, C, 2), Wt (H C, C), blin (C);
    and gcat = g Wt^T (N, H C) with its majorant gcat_bound = |g| |Wt|^T."""
    g = torch.as_tensor(np.asarray(g)).to(ref.dtype)[:ref.N]
    gp, gw, gwt, gb = torch.autograd.grad(ref.y, [ref.att.proj, ref.att.We, ref.Wt, ref.blin], g, retain_graph=True)
    W = ref.Wt.detach()
    return SimpleNamespace(proj=gp, We=gw, Wt=gwt, blin=gb, gcat=g @ W.T, gcat_bound=g.abs() @ W.abs().T)


def coefficients(ref, rev, slots=None):
    """(alpha_e (H, slots), alpha_s (H, N)) as qt_attn_weights lays them out: the coefficient of the message col[e] -> row(e) at
    rev[e], that of node i's self pair at i, 0 where there is none (and in the slots no valid edge owns)."""
    rev = np.asarray(rev).astype(np.int64)[:ref.E]
    a = ref.att.alpha.detach().to(torch.float64).numpy()
    alpha_e = np.zeros((ref.H, slots or ref.E))
    alpha_e[:, rev] = a[:ref.E].T
    alpha_s = np.zeros((ref.H, ref.N))
    alpha_s[:, ref.att.tgt[ref.E:]] = a[ref.E:].T
    return alpha_e, alpha_s


# ------------------------------------------------------------------------------------------------------------------ checkers
_GC = {k: v.default for k, v in inspect.signature(grad_close).parameters.items()}


def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def worst(got, want, bound):
    """worst |got - want| / bound; inf for a NaN / inf in `got` or an error where the bound is 0."""
    got, want = _np(got), _np(want)
    bound = np.broadcast_to(_np(bound), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - want)
    pos = bound > 0
    if (err[~pos] != 0).any():
        return math.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def grad_ratio(a, b):
    """worst |a - b| / (atol + rtol |b|) with helpers.grad_close's own defaults (read from its signature)."""
    b = _np(b)
    return worst(a, b, _GC['rel_atol'] * max(_GC['floor'], float(np.abs(b).max())) + _GC['rtol'] * np.abs(b))


def _report(tag, ratios):
    print(f'mh_f64 {tag}: ' + ' '.join(f'{n}={v:.3g}' for n, v in ratios))


def check_forward(tag, ref, y=None, cat=None):
    """y (>= N rows, C) and / or cat (>= N rows, H C) against the reference, each entry within RTOL x its majorant."""
    ratios = []
    if cat is not None:
        ratios.append(('cat', worst(cat[:ref.N], ref.cat, RTOL * ref.att.absum)))
    if y is not None:
        ratios.append(('y', worst(y[:ref.N], ref.y, RTOL * ref.ybound)))
    _report(tag, ratios)
    for name, v in ratios:
        assert v <= 1.0, f'{tag}: {name} is {v:.3g} x its bound'
    return dict(ratios)


def check_stats(tag, ref, stats):
    """stats (H, >= N rows, 2) = (m, lsum) per head and target."""
    got = _np(stats)[:, :ref.N]
    m, lsum, S = ref.m.numpy().T, ref.lsum.numpy().T, ref.S.numpy().T
    has = np.isfinite(m)
    assert np.array_equal(np.isfinite(got[..., 0]), has), f'{tag}: a row maximum is finite where the target has no pair, or not where it has'
    ratios = [('m', worst(np.where(has, got[..., 0], 0.0), np.where(has, m, 0.0), RTOL * S)),
              ('lsum', worst(got[..., 1], lsum, RTOL * lsum * (1.0 + 2.0 * S)))]
    _report(tag + ' stats', ratios)
    for name, v in ratios:
        assert v <= 1.0, f'{tag}: stats {name} is {v:.3g} x its bound'
    return dict(ratios)


def check_gcat(tag, ref, grads, gcat):
    v = worst(gcat[:ref.N], grads.gcat, RTOL * grads.gcat_bound)
    _report(tag, [('gcat', v)])
    assert v <= 1.0, f'{tag}: gcat is {v:.3g} x its bound'
    return v


def check_merge_grads(tag, grads, dWt, dblin, scale=None):
    """dWt (H C, C), dblin (C) with helpers.grad_close at its defaults (`scale`: the reference to hold them to, default grads')."""
    want_w, want_b = (grads.Wt, grads.blin) if scale is None else scale
    _report(tag, [('dWt', grad_ratio(dWt, want_w)), ('dblin', grad_ratio(dblin, want_b))])
    grad_close(torch.as_tensor(_np(dWt)), want_w, msg=f'{tag} dWt')
    grad_close(torch.as_tensor(_np(dblin)), want_b, msg=f'{tag} dblin')


def check_grads(tag, ref, grads, dproj, dWe, dWt, dblin):
    """d proj per block (q, k, v, skip) and head, dWe, dWt, dblin: helpers.grad_close at its defaults; no NaN in a valid row."""
    N, H, C = ref.N, ref.H, ref.C
    got, want = torch.as_tensor(_np(dproj))[:N].view(N, H, 4, C), grads.proj.view(N, H, 4, C)
    blocks = [(f'd{name}[{h}]', got[:, h, b], want[:, h, b]) for b, name in enumerate(('q', 'k', 'v', 'skip')) for h in range(H)]
    blocks += [('dWe', torch.as_tensor(_np(dWe)).reshape(H, C, 2), grads.We), ('dWt', torch.as_tensor(_np(dWt)), grads.Wt),
               ('dblin', torch.as_tensor(_np(dblin)), grads.blin)]
    r = {name: grad_ratio(a, b) for name, a, b in blocks}
    shown = [(f'd{n}', max(r[f'd{n}[{h}]'] for h in range(H))) for n in ('q', 'k', 'v', 'skip')] + [(n, r[n]) for n in ('dWe', 'dWt', 'dblin')]
    _report(tag, shown)
    for name, a, b in blocks:
        assert not torch.isnan(a).any(), f'{tag}: NaN in {name}'
        grad_close(a, b, msg=f'{tag} {name}')
    return dict(shown)


def check_alpha(tag, ref, rev, selfpair, alpha_e, alpha_s, yardstick=None):
    """alpha_e (H, slots), alpha_s (H, >= N rows) against the reference's coefficients at ATOL + RTOL alpha; alpha_s exactly 0 where
    a node has no self pair.  `yardstick`: the float32 model, whose ratio under the same bound is printed beside the kernel's."""
    rev = np.asarray(rev).astype(np.int64)[:ref.E]
    want_e, want_s = coefficients(ref, rev, _np(alpha_e).shape[1])
    got_e, got_s = _np(alpha_e), _np(alpha_s)[:, :ref.N]
    used = np.zeros(want_e.shape[1], dtype=bool)
    used[rev] = True
    ratios = [('alpha_e', worst(got_e[:, used], want_e[:, used], ATOL + RTOL * want_e[:, used])),
              ('alpha_s', worst(got_s, want_s, ATOL + RTOL * want_s))]
    if yardstick is not None:
        ye, ys = coefficients(yardstick, rev, want_e.shape[1])
        ratios += [('f32 alpha_e', worst(ye[:, used], want_e[:, used], ATOL + RTOL * want_e[:, used])),
                   ('f32 alpha_s', worst(ys, want_s, ATOL + RTOL * want_s))]
    _report(tag, ratios)
    none = np.ones(ref.N, dtype=bool) if selfpair is None else ~(np.asarray(selfpair)[:ref.N] > 0)
    assert not got_s[:, none].any(), f'{tag}: alpha_s is not 0 at a node without a self pair'
    for name, v in ratios[:2]:
        assert v <= 1.0, f'{tag}: {name} is {v:.3g} x its bound'
    return dict(ratios)


def check_dropout_acted(tag, y, y_keep1, N):
    """keep < 1 changed y by O(1) (a wrong mask would, too: that is what the forward bound under the reference's mask excludes)."""
    d = float(np.abs(_np(y)[:N] - _np(y_keep1)[:N]).max())
    print(f'mh_f64 {tag}: max |y - y(keep = 1)| = {d:.3g}')
    assert d > 0.1, f'{tag}: dropout moved y by {d:.3g} only'


def check_all(tag, ref, g, rev, selfpair, out):
    """Every checker on a full set of outputs (float32_outputs' keys)."""
    grads = gradients(ref, g)
    check_forward(tag, ref, out['y'], out['cat'])
    check_stats(tag, ref, out['stats'])
    check_gcat(tag, ref, grads, out['gcat'])
    check_grads(tag, ref, grads, out['dproj'], out['dWe'], out['dWt'], out['dblin'])
    check_alpha(tag, ref, rev, selfpair, out['alpha_e'], out['alpha_s'])


# ------------------------------------------------------------------------------------------------------------------ float32 form
TAMPERS = ('wt_blocks_swapped', 'head1_draws_head0_seed', 'blin_per_head_group', 'rows_past_sweep_dropped', 'lsum_from_head0',
           'alpha_at_e')


def float32_outputs(graph, ops, c_real, H, keep, seed, epoch, rev, tamper=None):
    """The outputs of the kernels as the float32 form of the model gives them: y, cat, stats (H, N, 2), gcat, dproj, dWe, dWt,
    dblin, alpha_e (H, E), alpha_s (H, N).  graph = (rowptr, col, selfpair, eattr); ops: operands().  `tamper` states one wrong
    kernel (TAMPERS): two heads' row blocks of Wt swapped; head 1 drawing head 0's dropout seed; blin added once per head group;
    the rows from 8192 on left out of dWt / dblin; lsum of the heads > 0 taken from head 0; alpha_e written at e, not at rev[e]."""
    assert tamper is None or tamper in TAMPERS, tamper
    f32 = torch.float32
    C = ops.Wt.shape[1]
    m = model(*graph, ops.proj, ops.We, ops.Wt, ops.blin, c_real, H, keep, seed, epoch, dtype=f32)
    gr = gradients(m, ops.g)
    N = m.N
    cat, y = m.cat.detach(), m.y.detach()
    gcat, dWt, dblin = gr.gcat, gr.Wt, gr.blin
    stats = torch.stack([m.m.T, m.lsum.T], dim=-1)
    alpha_e, alpha_s = coefficients(m, rev)
    if tamper == 'wt_blocks_swapped':
        assert H >= 2
        W = ops.Wt.view(H, C, C).clone()
        W[[0, 1]] = W[[1, 0]]
        y = cat @ W.view(H * C, C) + ops.blin
    elif tamper == 'head1_draws_head0_seed':
        assert H >= 2 and keep < 1.0
        # a one-head launch on head h's columns with the seed s draws the mask of head 0 under s: head h's own mask is that of
        # seed + h 0x632BE5AB, and head 1 here keeps head 0's seed
        heads = []
        for h in range(H):
            hs = (seed + (0 if h == 1 else h) * 0x632BE5AB) & 0xFFFFFFFF
            one = attention_f64(*graph, ops.proj.view(N, H, 4 * C)[:, h], ops.We[h:h + 1], c_real, 1, keep, hs, epoch, 0, f32)
            heads.append(one.out.detach())
        cat = torch.cat(heads, dim=1)
        y = cat @ ops.Wt + ops.blin
    elif tamper == 'blin_per_head_group':
        y = y + (MAX_HEADS - 1) * ops.blin
    elif tamper == 'rows_past_sweep_dropped':
        assert N > SWEEP
        g = ops.g.clone()
        g[SWEEP:] = 0.0
        dWt, dblin = cat.T @ g, g.sum(0)
    elif tamper == 'lsum_from_head0':
        assert H >= 2
        stats = stats.clone()
        stats[1:, :, 1] = stats[0, :, 1]
    elif tamper == 'alpha_at_e':
        alpha_e = np.zeros_like(alpha_e)
        alpha_e[:, :m.E] = m.att.alpha.detach().double().numpy()[:m.E].T
    return dict(y=y, cat=cat, stats=stats, gcat=gcat, dproj=gr.proj, dWe=gr.We, dWt=dWt, dblin=dblin, alpha_e=alpha_e, alpha_s=alpha_s)
