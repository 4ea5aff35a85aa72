"""Parameter groups (set_param_groups) in numpy float64: one step of clip + decoupled decay + scaled Adam, the bound a float32 run
of the mechanism has to keep, and a float32 emulation of that mechanism with two tampered forms.  Built on the Adam model of
tests/pack_f64.py; not a test module (test_groups_host.py and test_gpu_groups.py import it).  numpy only; nothing of qtmpnn.

THE RULE, per entry i, on the hyperparameters as the device receives them (float32 unless `exact`):

    g      <- g * min(1, max_norm / (|g| + 1e-6))                       the GLOBAL norm, every entry in it
    m, v   <- Adam's moments of g, for every entry                      pack_f64.adam_step
    p1     =  p * (1 - lr * s * lam)                                    decoupled decay
    p_new  =  p1 - s * upd,   upd = (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)

which is torch.optim.AdamW with the learning rate lr * s_i and the decay lam_i (test_groups_host.py holds it to that).

THE MECHANISM under test (qtmpnn.groups.GroupedStep), float32, every line one rounding (nothing is contracted: each line is a
launch of its own):

    t = fl(nsl * lr),  nsl = -fl(s * lam)        D = fl(1 + t)        p0 = fl(p * D)
    q = the optimiser's own step from p0 at the learning rate lr
    w = fl(q - p0);   w = fl(w * s);   p_new = fl(w + p0)             on the entries with s != 1; the others keep q

THE BOUND (grouped_bound), u = 2^-24, by the house rule: first-order propagation of the counted roundings, DOUBLED.
  decay   D carries three roundings of the product lr s lam (fl(s lam), fl(lr) where the optimiser itself holds a double, the
          product) and one of the sum; p0 one more:  e_p0 = u |p| (3 lr s lam + |D|) + u |p1|.  Where s lam = 0, D is exactly 1
          and p0 = p: e_p0 = 0.
  Adam    pack_f64.adam_bound's e_q for one plain clip + Adam step from p0 (its p bound, before its doubling); the error of p0
          passes through with factor 1.
  blend   with d = q - p0 (|d| <= |upd| + e_q) and P = max(|p0|, |q|, |p_new|), each as a multiple of ulp(|p|) ~ u P:
              the subtraction   one rounding of d, then scaled by s:  u s |d|,  |d| <= 2 P     -> at most 2 s
              the product       one rounding of s d:                  u s |d|                  -> at most 2 s
              the sum           one rounding of the result:           u |p_new|                -> at most 1 (1 + 2 s beyond s = 1)
          so e_blend = u (2 s |d| + |p_new|), at most (4 s + 1) ulp(|p|); Adam's error enters scaled: s e_q.
          (Where q lies within a factor 2 of p0 the subtraction is exact, by Sterbenz; the bound does not use that.)
    |p_new - model| <= 2 (e_p0 + s e_q + e_blend)     entries with s != 1
                    <= 2 (e_p0 + e_q)                 entries with s = 1: the blend skips them
  The moments keep adam_bound's bounds: the mechanism does not touch them.

TWO OPTIMISER FORMS.  'flat' is qt_flat_adam: every hyperparameter float32, the corrections 1 - powf(beta, t) on float32 betas.
'list' is torch's fused Adam behind clip_grad_norm_: betas and eps are doubles and the corrections are formed in double; the
learning rate is a double, or a float32 device tensor when capturable (`lr_on_device`); max_norm and 1e-6 enter float32 tensor
ops.  Its kernel rounds once per stored value where qt_flat_adam rounds per operation, and its norm is a tree of per-tensor
norms, so pack_f64's counts bound it as well; the decay launch always reads fl32(lr)."""
import numpy as np

import pack_f64
from pack_f64 import F, U, f32, f64

FORMS = ('flat', 'list')
TAMPERS = ('decay_after', 'scale_on_gradient')


def _hyper(form, lr, beta1, beta2, eps, max_norm, lr_on_device, exact):
    """(kwargs of pack_f64.adam_step, lr of the decay launch)."""
    if exact:
        return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm, exact_hyper=True), lr
    if form == 'flat':
        return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm), f32(lr)
    assert form == 'list', form
    # (adam_step then adds the exact 1e-6 where the device adds fl32(1e-6): 3e-14 absolute on a norm, far below u)
    return dict(lr=f32(lr) if lr_on_device else lr, beta1=beta1, beta2=beta2, eps=eps,
                max_norm=None if max_norm is None else f32(max_norm), exact_hyper=True), f32(lr)


def grouped_step(p, g, m, v, t, s, lam, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0, form='flat', lr_on_device=False,
                 exact=False):
    """One step of the rule in float64 -> pack_f64.adam_step's dict (from the decayed p1) with p the new parameters and, besides,
    p1, D, s, sl (s lam), lr_decay (the learning rate of the decay).  s, lam: per entry (arrays or numbers), rounded to float32
    unless `exact`.  t: the step number of THIS update."""
    kw, lr_d = _hyper(form, lr, beta1, beta2, eps, max_norm, lr_on_device, exact)
    s, lam = np.broadcast_to(f64(s), np.shape(p)), np.broadcast_to(f64(lam), np.shape(p))
    if not exact:
        s, lam = s.astype(F).astype(np.float64), lam.astype(F).astype(np.float64)
    D = 1.0 - lr_d * s * lam
    p1 = f64(p) * D
    out = pack_f64.adam_step(p1, g, m, v, t, **kw)
    return dict(out, p=p1 - s * out['upd'], q=out['p'], p1=p1, D=D, s=s, sl=s * lam, lr_decay=lr_d)


def grouped_bound(p, g, m, v, t, out, n=None, clip=True):
    """dict of bounds |device - grouped_step| for p, m, v, g, norm (the module docstring derives them), for inputs that are the
    float32 values the device reads."""
    adam = pack_f64.adam_bound(out['p1'], g, m, v, t, out, n=n, clip=clip)
    s, D, lr = out['s'], out['D'], out['lr_decay']
    e_q = adam['p'] / 2.0
    decayed = out['sl'] != 0.0
    e_p0 = np.where(decayed, U * np.abs(f64(p)) * (3.0 * lr * out['sl'] + np.abs(D)) + U * np.abs(out['p1']), 0.0)
    d = np.abs(out['upd']) + e_q
    e_blend = U * (2.0 * s * d + np.abs(out['p']))
    e = np.where(s != 1.0, e_p0 + s * e_q + e_blend, e_p0 + e_q)
    return dict(adam, p=2.0 * e)


def ratio(got, want, bound):
    """max |got - want| / bound over the entries; 0 / 0 counts as 0 (an entry that must be, and is, exact)."""
    err = np.abs(f64(got) - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def worst(got, out, bound, keys=('p', 'm', 'v')):
    """{key: max |got[key] - model| / bound}: a value <= 1 keeps the bound."""
    return {k: ratio(got[k], out[k], bound[k]) for k in keys}


def emulate_grouped(p, g, m, v, t, s, lam, lr=0.01, max_norm=10.0, tamper=None, **adam):
    """The mechanism in float32 around pack_f64.emulate_adam (the flat form) -> dict(p, m, v, g, norm).  tamper:
        decay_after         the decay multiplies the parameters after the update (and after the blend)
        scale_on_gradient   lr_scale multiplies the clipped gradient and there is no blend: Adam's normalisation undoes it"""
    assert tamper is None or tamper in TAMPERS
    p, g = np.asarray(p, F), np.asarray(g, F)
    s, lam = np.broadcast_to(np.asarray(s, F), p.shape), np.broadcast_to(np.asarray(lam, F), p.shape)
    nsl = -(s * lam)
    D = F(1) + nsl * F(lr)
    p0 = p if tamper == 'decay_after' else p * D
    if tamper == 'scale_on_gradient':
        first = pack_f64.emulate_adam(p0, g, m, v, t, lr=lr, max_norm=max_norm, **adam)        # (for the clipped gradient)
        out = pack_f64.emulate_adam(p0, first['g'] * s, m, v, t, lr=lr, max_norm=None, **adam)
        return dict(out, norm=first['norm'])
    out = pack_f64.emulate_adam(p0, g, m, v, t, lr=lr, max_norm=max_norm, **adam)
    q = out['p']
    w = q - p0
    w = w * s
    w = w + p0
    new = np.where(s != F(1), w, q)
    if tamper == 'decay_after':
        new = new * D
    return dict(out, p=new)


# The mixed setting of the issue and an all-unit one, as (pattern, options) pairs
MIXED = [('*norm*', {}), ('*bias*', {}), ('encoder.*', dict(lr_scale=0.1, weight_decay=1e-2)), ('*', dict(weight_decay=1e-2))]
ALL_UNIT = [('*', dict(lr_scale=1.0, weight_decay=0.0))]
