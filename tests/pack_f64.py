"""Weight-space composition and clip + Adam in numpy float64, as csrc/pack.hip computes them.

Composition (k_compose_step_*, k_compose2_*): one product of a Chebyshev series with a layer,
    M[g, k] = sum_{a, b} cf(k, a, b) P0[g, a] @ P1[g, b],   cf = ([a + b = k] + [|a - b| = k]) / 2,
the bias series riding along with B1 added at order 0 only, in the natural layout (step_fwd / step_bwd) and in the packed gate
matrix of k_compose2_fwd (packed / unpack_grad / compose2_fwd / compose2_bwd).  Every function is multilinear with non-negative
coefficients, so its majorant sum cf |P0| |P1| is the same function on the absolute values (`maj=True`).

Adam (k_flat_sumsq, k_flat_adam): adam_step is one step of clip + Adam in float64 ON THE HYPERPARAMETERS AS THE ABI RECEIVES THEM --
lr, beta1, beta2, eps and max_norm rounded to float32 -- because the kernel's bias corrections 1 - powf(beta, t) see float32
betas: against torch's host-side double corrections the update differs, at t = 1, by |fl32(beta2) - beta2| / (2 (1 - beta2))
~ 6.4e-6 relative (beta2_deviation; it shrinks with t and is below the project's 1e-4 target and below 1e-5).  That known
deviation is stated on the host (tests/test_pack_f64_host.py); the GPU comparison measures the kernel's arithmetic alone.

The bounds follow the house rule (tests/cheb_f64.py): TWICE a count of float32 roundings times 2^-24 times the majorant.
numpy only; nothing of qtmpnn."""
import numpy as np

U = 2.0 ** -24
# Accuracy the Adam bound grants the device powf, in units of 2^-24 beta^t before the doubling (adam_bound).  The ROCm installation
# carries no documented figure, so it is measured: the smallest integer <= 4 for which the worst error / bound of the real Adam
# families on an MI355X is <= 0.5 (a 2x margin: powf's worst case need not be among the tested t).  Recorded run with 1: 0.497
# (profiles/head_pack_f64.txt).
POW_ULPS = 1
F = np.float32


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def pad4(n):
    return -(-n // 4) * 4


# ------------------------------------------------------------------------------------------------------------- composition
def cf(K2, Ka, K, second_term=True):
    c = np.zeros((K2, Ka, K))
    for a in range(Ka):
        for b in range(K):
            c[a + b, a, b] += 0.5
            if second_term:
                c[abs(a - b), a, b] += 0.5
    return c


def _prep(arrs, maj):
    return [np.abs(f64(a)) if maj else f64(a) for a in arrs]


def step_fwd(P0, B0, P1, B1, maj=False, second_term=True, b1_every_order=False):
    """(P (4, Ka + K - 1, in, h), B (4, Kb0 + K - 1, h)) of the series (P0 (4, Ka, in, h), B0 (4, Kb0, h)) through the layer
    (P1 (4, K, h, h), B1 (4, h))."""
    P0, B0, P1, B1 = _prep((P0, B0, P1, B1), maj)
    Ka, Kb0, K = P0.shape[1], B0.shape[1], P1.shape[1]
    c = cf(Ka + K - 1, Ka, K, second_term)
    P = np.einsum('kab,gaco,gbop->gkcp', c, P0, P1)
    B = np.einsum('kab,gao,gbop->gkp', c[:Kb0 + K - 1, :Kb0], B0, P1)
    if b1_every_order:
        B += B1[:, None]
    else:
        B[:, 0] += B1
    return P, B


def step_bwd(P0, B0, P1, gP, gB, maj=False):
    """(gP0, gB0, gP1, gB1) of step_fwd under the cotangents gP (4, K2, in, h), gB (4, Kbo, h)."""
    P0, B0, P1, gP, gB = _prep((P0, B0, P1, gP, gB), maj)
    Ka, Kb0, K = P0.shape[1], B0.shape[1], P1.shape[1]
    c = cf(Ka + K - 1, Ka, K)
    cb = c[:Kb0 + K - 1, :Kb0]
    gP0 = np.einsum('kab,gkcp,gbop->gaco', c, gP, P1)
    gP1 = np.einsum('kab,gaco,gkcp->gbop', c, P0, gP) + np.einsum('kab,gao,gkp->gbop', cb, B0, gB)
    gB0 = np.einsum('kab,gkp,gbop->gao', cb, gB, P1)
    return gP0, gB0, gP1, gB[:, 0].copy()


def terms(Ka, K, Kb0):
    """The longest run of non-zero cf terms a kernel loop adds up: over (a, b) for an output order k, over (b, k) for a, over
    (a, k) for b; and the same for the bias series (Kb0 orders)."""
    c = cf(Ka + K - 1, Ka, K) != 0
    cb = c[:Kb0 + K - 1, :Kb0]
    return dict(k=int(c.sum(axis=(1, 2)).max()), a=int(c.sum(axis=(0, 2)).max()), b=int(c.sum(axis=(0, 1)).max()),
                kb=int(cb.sum(axis=(1, 2)).max()), ab=int(cb.sum(axis=(0, 2)).max()), bb=int(cb.sum(axis=(0, 1)).max()))


def step_bounds(P0, B0, P1, B1, both=False):
    """(|P - model|, |B - model|).  series_elem: per non-zero cf term a chain of h fused multiply-adds, then one fused multiply-add
    into the running sum: h + T_k roundings on the longest chain.  bias_elem: the same + the add of B1; `both`: + the add of the
    two branches' series in the packed bias rows (the caller sums the two majorants)."""
    h = np.shape(P1)[-1]
    t = terms(np.shape(P0)[1], np.shape(P1)[1], np.shape(B0)[1])
    mP, mB = step_fwd(P0, B0, P1, B1, maj=True)
    return 2.0 * (h + t['k']) * U * mP, 2.0 * (h + t['kb'] + 1 + int(both)) * U * mB


def step_bwd_bounds(P0, B0, P1, gP, gB, summed=False):
    """Bounds of (gP0, gB0, gP1, gB1).  gP0, gB0: chains of h fused multiply-adds per term, T_a (T_ab) terms; gP1: chains of `in`,
    T_b terms, then T_bb bias terms of two roundings each (f B0 rounds, then the fused multiply-add); gB1 is a copy.  `summed`:
    the cotangent is the sum of two variants' gradients (PackedGrad: one more rounding per read -- the caller passes the summed
    majorant |gW1| + |gW0| -- and gB1 = that sum: one rounding)."""
    h, cin = np.shape(P1)[-1], np.shape(P0)[2]
    t = terms(np.shape(P0)[1], np.shape(P1)[1], np.shape(B0)[1])
    m0, mb0, m1, mb1 = step_bwd(P0, B0, P1, gP, gB, maj=True)
    s = int(summed)
    return (2.0 * (h + t['a'] + s) * U * m0, 2.0 * (h + t['ab'] + s) * U * mb0, 2.0 * (cin + t['b'] + 2 * t['bb'] + s) * U * m1,
            2.0 * s * U * mb1)


def packed(Mx, Mh, Bs, cin_pad, with_h, swap=False, pad_value=0.0):
    """The layout of k_compose2_fwd: rows k C + c with C = cin_pad (+ h with H) -- the x branch in columns c < cin, exact zeros in
    cin <= c < cin_pad, the h branch from cin_pad --, then ksp = pad4(Kbo) bias rows (zero beyond Kbo); columns gate-major."""
    _, K2, cin, h = Mx.shape
    Kbo = Bs.shape[1]
    C = cin_pad + (h if with_h else 0)
    W = np.zeros((K2, C, 4, h))
    W[:, cin:cin_pad] = pad_value
    if swap and with_h:                                   # (mutation: the h block first)
        W[:, :h] = Mh.transpose(1, 2, 0, 3)
        W[:, h:h + cin] = Mx.transpose(1, 2, 0, 3)
    else:
        W[:, :cin] = Mx.transpose(1, 2, 0, 3)
        if with_h:
            W[:, cin_pad:] = Mh.transpose(1, 2, 0, 3)
    rows = np.zeros((pad4(Kbo), 4, h))
    rows[:Kbo] = Bs.transpose(1, 0, 2)
    return np.concatenate([W.reshape(K2 * C, 4 * h), rows.reshape(-1, 4 * h)])


def unpack_grad(gW1, gW0, K2, Kbo, cin, cin_pad, h, maj=False, one_variant_bias=False):
    """(gMx (4, K2, cin, h), gMh (4, K2, h, h), gBs (4, Kbo, h)) as PackedGrad reads them: both variants' gradients summed, the h
    branch from gW1 only (zeros without it)."""
    gMx, gMh, gBs = np.zeros((4, K2, cin, h)), np.zeros((4, K2, h, h)), np.zeros((4, Kbo, h))
    for i, (gW, C) in enumerate(((gW1, cin_pad + h), (gW0, cin_pad))):
        if gW is None:
            continue
        gW = np.abs(f64(gW)) if maj else f64(gW)
        body = gW[:K2 * C].reshape(K2, C, 4, h)
        gMx += body[:, :cin].transpose(2, 0, 1, 3)
        if C > cin_pad:
            gMh += body[:, cin_pad:].transpose(2, 0, 1, 3)
        if not (one_variant_bias and i == 1 and gW1 is not None):
            gBs += gW[K2 * C:K2 * C + Kbo].reshape(Kbo, 4, h).transpose(1, 0, 2)
    return gMx, gMh, gBs


def compose2_fwd(x, hb, cin_pad, variants, **mut):
    """Packed matrices per variant and their bounds.  x = (Px0, Bx0, Px1, Bx1), hb likewise.  Mutations: second_term,
    b1_every_order (step_fwd), pad_value, swap (packed), bias_from_x_only."""
    fw = {k: mut.pop(k) for k in ('second_term', 'b1_every_order') if k in mut}
    only_x = mut.pop('bias_from_x_only', False)
    Mx, Bx = step_fwd(*x, **fw)
    Mh, Bh = step_fwd(*hb, **fw)
    ePx, eBx = step_bounds(*x, both=True)
    ePh, eBh = step_bounds(*hb, both=True)
    Ws = [packed(Mx, Mh, Bx if only_x else Bx + Bh, cin_pad, v, **mut) for v in variants]
    Es = [packed(ePx, ePh, eBx + eBh, cin_pad, v) for v in variants]
    return Ws, Es


def compose2_bwd(x, hb, cin_pad, gW1, gW0, one_variant_bias=False):
    """((gPx0, gBx0, gPx1, gBx1, gPh0, gBh0, gPh1, gBh1), bounds) under the packed cotangents gW1 / gW0 (either may be None)."""
    _, Ka, cin, h = np.shape(x[0])
    K2, Kbo = Ka + np.shape(x[2])[1] - 1, np.shape(x[1])[1] + np.shape(x[2])[1] - 1
    gMx, gMh, gBs = unpack_grad(gW1, gW0, K2, Kbo, cin, cin_pad, h, one_variant_bias=one_variant_bias)
    aMx, aMh, aBs = unpack_grad(gW1, gW0, K2, Kbo, cin, cin_pad, h, maj=True)
    both = gW1 is not None and gW0 is not None
    gx, gh = step_bwd(x[0], x[1], x[2], gMx, gBs), step_bwd(hb[0], hb[1], hb[2], gMh, gBs)
    ex = step_bwd_bounds(x[0], x[1], x[2], aMx, aBs, summed=both)
    eh = step_bwd_bounds(hb[0], hb[1], hb[2], aMh, aBs, summed=both)
    return gx + gh, ex + eh


def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds to float64 and then to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def emulate_step_fwd(P0, B0, P1, B1):
    """float32 emulation of series_elem / bias_elem with the kernel's fmaf order: per (a, b) with cf != 0 the dot product over o in
    order, then s = fmaf(cf, d, s) in (a, b) order."""
    P0, B0, P1, B1 = (np.asarray(a, F) for a in (P0, B0, P1, B1))
    _, Ka, cin, h = P0.shape
    Kb0, K = B0.shape[1], P1.shape[1]
    c = cf(Ka + K - 1, Ka, K)
    P, B = np.zeros((4, Ka + K - 1, cin, h), F), np.zeros((4, Kb0 + K - 1, h), F)
    for a in range(Ka):
        for b in range(K):
            d, db = np.zeros((4, cin, h), F), np.zeros((4, h), F)
            for o in range(h):
                d = _fma(P0[:, a, :, o, None], P1[:, b, o, None, :], d)
                if a < Kb0:
                    db = _fma(B0[:, a, o, None], P1[:, b, o, :], db)
            for k in np.nonzero(c[:, a, b])[0]:
                P[:, k] = _fma(F(c[k, a, b]), d, P[:, k])
                if a < Kb0 and k < Kb0 + K - 1:
                    B[:, k] = _fma(F(c[k, a, b]), db, B[:, k])
    B[:, 0] = B[:, 0] + B1
    return P, B


# Shapes (cin, cin_pad, h, K, L) of tests/test_gpu_pack_f64.py
SHAPES = [(4, 4, 8, 3, 2), (5, 8, 8, 3, 2), (1, 4, 16, 2, 2), (4, 4, 16, 1, 2), (8, 8, 16, 3, 3), (5, 8, 8, 2, 4), (4, 4, 8, 8, 5),
          (4, 4, 32, 3, 2), (4, 4, 64, 3, 2), (4, 4, 128, 3, 2)]
VARIANTS = [(True,), (False,), (True, False)]


def stages(K, L):
    """(Ka, Kb0) of every product of an L-layer stack: L - 2 natural-layout steps, then the packed one."""
    return [(K + i * (K - 1), 1 + i * (K - 1)) for i in range(L - 1)]


def ints(rng, *shape):
    return rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape).astype(F)


def draw(rng, *shape):
    return (rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))).astype(F)


def branch(gen, rng, Ka, Kb0, K, cin, h):
    return gen(rng, 4, Ka, cin, h), gen(rng, 4, Kb0, h), gen(rng, 4, K, h, h), gen(rng, 4, h)


# -------------------------------------------------------------------------------------------------------------------- Adam
ADAM_N = (1, 63, 255, 256, 257, 1023, 1025, 34513, 1000003)
ADAM_T = (1, 2, 10, 1000, 100000)
HYPER = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)


def f32(x):
    return float(np.float32(x))


def adam_step(p, g, m, v, t, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0, exact_hyper=False):
    """One step of clip + Adam in float64: dict(p, g, m, v, norm, coef, raw (the unclamped coefficient), upd).  t: the step number
    of THIS update (the device counter + 1).  Hyperparameters rounded to float32 (as the ABI passes them) unless exact_hyper."""
    if not exact_hyper:
        lr, beta1, beta2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
        max_norm = None if max_norm is None else f32(max_norm)
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    norm = float(np.sqrt((g * g).sum()))
    raw = coef = 1.0
    if max_norm is not None and max_norm > 0:
        raw = max_norm / (norm + (1e-6 if exact_hyper else f32(1e-6)))
        coef = min(raw, 1.0)
    g = g * coef
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    upd = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return dict(p=p - upd, g=g, m=m, v=v, norm=norm, coef=coef, raw=raw, upd=upd, bc=(bc1, bc2), hyper=(lr, beta1, beta2, eps))


def norm_count(n):
    """k_flat_sumsq: a thread adds ceil(n / 1024) squares in order (one more rounding for the square), the butterfly is 6 adds,
    the 16 wave sums are added in order."""
    return -(-n // 1024) + 1 + 6 + 16


def adam_bound(p0, g0, m0, v0, t, out, n=None, clip=True):
    """dict of bounds |kernel - adam_step| for p, g, m, v, norm, before any inherited error (the inputs are the float32 values the
    kernel reads).  First-order propagation of the counted roundings, doubled:
      norm   the sum of squares carries norm_count(n) roundings, the square root halves them and rounds once
      coef   + the add of 1e-6 and the division; clamped to 1 it is exact, and min is 1-Lipschitz at the threshold
      g      g coef rounds once:  r_g = e_coef / coef + u (relative)
      m      1 - beta1 rounds, the two products and the add round: 3 u of beta1 |m| + (1 - beta1) |g|, + g's error
      v      1 - beta2, two products (three with g's square), the product with beta2 and the add: 4 u v, + 2 r_g of its new term
      bc     1 - powf(beta, t): powf within POW_ULPS u beta^t and the subtraction's rounding: relative
             POW_ULPS u beta^t / (1 - beta^t) + u each -- for small t the subtraction cancels (1 - 0.999^t) and this term leads
      upd    lr / bc1 (1), its product with m (1), sqrt(v) (1), sqrt(bc2) (1), their quotient (1), the add of eps (1), the
             last quotient (1), each relative to the factor it rounds
      p      the store rounds once, of max(|p_old|, |p_new|)."""
    lr, b1, b2, eps = out['hyper']
    g0, m0, v0 = np.abs(f64(g0)), np.abs(f64(m0)), np.abs(f64(v0))
    n = np.size(g0) if n is None else n
    r_norm = (norm_count(n) / 2.0 + 1.0) * U
    e_coef = 0.0
    if clip and out['raw'] * (1.0 - 2.0 * (r_norm + 2.0 * U)) < 1.0:
        e_coef = out['raw'] * (r_norm + 2.0 * U)
    r_g = e_coef / out['coef'] + (U if clip else 0.0)
    g, m, v = np.abs(out['g']), out['m'], out['v']
    e_g = g * r_g
    e_m = (1.0 - b1) * e_g + 3.0 * U * (b1 * m0 + (1.0 - b1) * g)
    e_v = (1.0 - b2) * g * g * 2.0 * r_g + 4.0 * U * v
    bc1, bc2 = out['bc']
    r1, r2 = POW_ULPS * U * (1.0 - bc1) / bc1 + U, POW_ULPS * U * (1.0 - bc2) / bc2 + U
    sv = np.sqrt(v) / np.sqrt(bc2)
    D = sv + eps
    with np.errstate(invalid='ignore', divide='ignore'):
        r_v = np.where(v > 0, e_v / (2.0 * v), 0.0)
    r_D = sv / D * (r_v + r2 / 2.0 + 3.0 * U) + U
    e_u = np.abs(out['upd']) * (r1 + 3.0 * U + r_D) + (lr / bc1) * e_m / D
    e_p = e_u + U * np.maximum(np.abs(f64(p0)), np.abs(out['p']))
    return dict(p=2.0 * e_p, g=2.0 * e_g, m=2.0 * e_m, v=2.0 * e_v, norm=2.0 * r_norm * out['norm'])


def beta2_deviation(t, beta2=0.999):
    """Relative change of the update when beta2 is rounded to float32 before the bias correction sqrt(1 - beta2^t) (first order):
    t beta2^(t-1) |fl32(beta2) - beta2| / (2 (1 - beta2^t)); at t = 1: |fl32(beta2) - beta2| / (2 (1 - beta2)) ~ 6.4e-6."""
    return t * beta2 ** (t - 1) * abs(f32(beta2) - beta2) / (2.0 * (1.0 - beta2 ** t))


def emulate_adam(p, g, m, v, t, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0, eps_inside=False, no_bc2=False,
                 t_minus_1=False, no_writeback=False, no_min=False, drop_tail=False):
    """float32 emulation of k_flat_sumsq + k_flat_adam (powf in float64, rounded); the flags are the mutations."""
    p, g, m, v = (np.asarray(a, F).copy() for a in (p, g, m, v))
    lr, b1, b2, eps = F(lr), F(beta1), F(beta2), F(eps)
    n = g.size
    nn = n - n % 1024 if drop_tail else n
    sq = np.zeros(-(-max(nn, 1) // 1024) * 1024, F)
    sq[:nn] = g[:nn] * g[:nn]
    acc = np.zeros(1024, F)
    for row in sq.reshape(-1, 1024):
        acc = acc + row
    w = acc.reshape(16, 64)
    d = 32
    while d >= 1:                                         # xor butterfly, d = 32 .. 1
        w = w + w[:, np.arange(64) ^ d]
        d >>= 1
    s = F(0)
    for k in range(16):
        s = s + w[k, 0]
    norm = np.sqrt(s)
    coef = F(1)
    if max_norm is not None and max_norm > 0:
        coef = F(max_norm) / (norm + F(1e-6))
        if not no_min:
            coef = min(coef, F(1))
    tt = t - 1 if t_minus_1 else t
    with np.errstate(divide='ignore', invalid='ignore'):
        bc1 = F(1) - F(float(b1) ** tt)
        bc2 = F(1) if no_bc2 else F(1) - F(float(b2) ** tt)
        gi = g * coef
        mi = b1 * m + (F(1) - b1) * gi
        vi = b2 * v + (F(1) - b2) * gi * gi
        den = np.sqrt(vi / bc2 + eps) if eps_inside else np.sqrt(vi) / np.sqrt(bc2) + eps
        p = p - (lr / bc1) * mi / den
    return dict(p=p, g=g if no_writeback else gi, m=mi, v=vi, norm=float(norm))


def adam_gradient(rng, kind, n, max_norm=10.0):
    """The gradient families: 'clipped' randn 0.2 (scaled up for small n so that it is clipped), 'unclipped' randn 0.01, 'loguniform'
    magnitudes in 1e-9 .. 1, 'below' / 'above': norm one float32 ulp below / above max_norm, 'zeros': even entries exactly 0."""
    g = rng.standard_normal(n)
    if kind == 'clipped':
        g = g * max(0.2, 2.0 * max_norm / np.sqrt(n))
    elif kind == 'unclipped':
        g = g * min(0.01, 0.1 * max_norm / np.sqrt(n))
    elif kind == 'loguniform':
        g = np.sign(g) * 10.0 ** rng.uniform(-9, 0, n)
    elif kind in ('below', 'above'):
        g = g.astype(F)
        target = np.nextafter(F(max_norm), F(0) if kind == 'below' else F(np.inf))
        for _ in range(30):                               # scale until the float64 norm of the float32 vector sits at the target
            nrm = np.sqrt((g.astype(np.float64) ** 2).sum())
            g = (g.astype(np.float64) * (float(target) / nrm)).astype(F)
    elif kind == 'zeros':
        g = g * 0.01
        g[0::2] = 0.0
    return g.astype(F)


# ------------------------------------------------------------------------------------------------- whole stacks (compose_pack)
def stack_fwd(Ps, Bs, maj=False):
    """Fold layers 0 .. L-2 of one branch: [(P, B) before each product], the last pair being what the packed product reads."""
    P, B = (np.abs(f64(Ps[0])) if maj else f64(Ps[0])), (np.abs(f64(Bs[0])) if maj else f64(Bs[0]))[:, None]
    seq = [(P, B)]
    for Wl, bl in zip(Ps[1:-1], Bs[1:-1]):
        P, B = step_fwd(P, B, Wl, bl, maj=maj)
        seq.append((P, B))
    return seq


def stack_pack(Px, Bx, Ph, Bh, cin_pad, variants):
    """ops.compose_pack in float64: ([W per variant], the folded inputs of the last product per branch)."""
    sx, sh = stack_fwd(Px, Bx), stack_fwd(Ph, Bh)
    x, hb = (*sx[-1], f64(Px[-1]), f64(Bx[-1])), (*sh[-1], f64(Ph[-1]), f64(Bh[-1]))
    return compose2_fwd(x, hb, cin_pad, variants)[0], (sx, sh)


def stack_bwd(Px, Bx, Ph, Bh, cin_pad, gW1, gW0):
    """Gradients of stack_pack for every layer: (gPx [L], gBx [L], gPh [L], gBh [L])."""
    sx, sh = stack_fwd(Px, Bx), stack_fwd(Ph, Bh)
    x, hb = (*sx[-1], f64(Px[-1]), f64(Bx[-1])), (*sh[-1], f64(Ph[-1]), f64(Bh[-1]))
    g, _ = compose2_bwd(x, hb, cin_pad, gW1, gW0)
    out = []
    for seq, Ps, (gP, gB, gP1, gB1) in ((sx, Px, g[:4]), (sh, Ph, g[4:])):
        gPs, gBs = [gP1], [gB1]
        for l in range(len(Ps) - 2, 0, -1):
            P0, B0 = seq[l - 1]
            gP, gB, gP1, gB1 = step_bwd(P0, B0, Ps[l], gP, gB)
            gPs.insert(0, gP1)
            gBs.insert(0, gB1)
        out += [[gP] + gPs, [gB[:, 0]] + gBs]
    return out


def stack_exact(Px, Bx, Ph, Bh):
    """True when every partial sum of the stack on operands of {-2, -1, 1, 2} is exact in float32: the majorant of the last product,
    scaled by the 2^(L-1) its half-integer coefficients divide by, stays below 2^24 (a safe margin of 4 for the gradients' sums)."""
    L = len(Px)
    sx, sh = stack_fwd(Px, Bx, maj=True), stack_fwd(Ph, Bh, maj=True)
    top = max(step_fwd(*s[-1], np.abs(f64(P[-1])), np.abs(f64(B[-1])), maj=True)[0].max() for s, P, B in ((sx, Px, Bx), (sh, Ph, Bh)))
    return top * 2.0 ** (L - 1) * 4 < 2.0 ** 24
