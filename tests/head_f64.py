"""The decoder head's input in numpy float64: Za = relu(gamma xhat + beta) with xhat the LayerNorm of each row of O over its h
channels (eps 1e-5, variance / h), Zb = [concat | 0 ..], and the backward -- gO, gconcat and the parameter sums
[sum gy xhat | sum gy] (gy = the cotangent masked by the ReLU) -- as k_head_fwd<LPN> / k_head_bwd<LPN> (csrc/lstm.hip) compute
them.  part_slabs restates which rows workgroup b of k_head_bwd owns, so the per-workgroup slabs compare one by one.

The bounds live in the middle, each with the count of float32 roundings it stands for; emulate() is a float32 numpy emulation of
the kernels' arithmetic with the reduction trees of group_sum<LPN>, wave_strided_sum<LPN> and block_param_reduce (csrc/qt_cell.h),
and the mutations tests/test_head_f64_host.py measures.  CASES is the case table of tests/test_gpu_head_f64.py.
numpy only; nothing of qtmpnn."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
EPS = 1e-5
BLOCKS = 512            # qt_lstm_bwd_blocks: the backward grid's cap
HIDDEN = (8, 16, 32, 64, 128)
ROWS = (1, 37, 777, 70001)
KINK_SHARE = 1e-3       # at most this share of a case's entries may sit within the forward bound of the ReLU kink


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def log2i(n):
    return int(n).bit_length() - 1


def bwd_blocks(N, h):
    """qt_lstm_bwd_blocks: the grid of k_head_bwd over N rows (the capacity, not the valid count)."""
    return 0 if N <= 0 else min(-(-N * (h // 4) // 256), BLOCKS)


# ------------------------------------------------------------------------------------------------------------------- model
def stats(O, eps=EPS):
    x = f64(O)
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    return d, var, rstd, d * rstd


def forward(O, ln_o, concat, hp):
    """(Za (N, h), Zb (N, hp - h), pre (N, h)): pre = gamma xhat + beta, Za = relu(pre), Zb = [concat | 0 ..] (concat None: zeros)."""
    ln_o = f64(ln_o)
    N, h = np.shape(O)
    xh = stats(O)[3]
    pre = ln_o[0] * xh + ln_o[1]
    Zb = np.zeros((N, hp - h))
    if concat is not None and hp > h:
        Zb[:, 0] = f64(concat).reshape(N)
    return np.maximum(pre, 0.0), Zb, pre


def masked(gZa, O, ln_o):
    """gy: the cotangent of Za where the pre-activation is positive, else 0."""
    ln_o = f64(ln_o)
    return np.where(ln_o[0] * stats(O)[3] + ln_o[1] > 0, f64(gZa), 0.0)


def backward(gZa, gZb, O, ln_o):
    """(gO (N, h), gconcat (N,) = gZb[:, 0] or None, psum (2 h,) = [sum gy xhat | sum gy])."""
    ln_o = f64(ln_o)
    _, _, rstd, xh = stats(O)
    gy = masked(gZa, O, ln_o)
    gxh = gy * ln_o[0]
    gO = rstd * (gxh - gxh.mean(axis=1, keepdims=True) - xh * (gxh * xh).mean(axis=1, keepdims=True))
    gcat = None if gZb is None else f64(gZb)[:, 0].copy()
    return gO, gcat, np.concatenate([(gy * xh).sum(axis=0), gy.sum(axis=0)])


def _by_block(t, nblk, R):
    """(n, w) row terms -> (sweeps, nblk, R, w): workgroup b owns node = b R + r + j nblk R (r = tid / LPN, sweep j)."""
    n, w = t.shape
    span = nblk * R
    sweeps = max(-(-n // span), 1)
    pad = np.zeros((sweeps * span, w), t.dtype)
    pad[:n] = t
    return pad.reshape(sweeps, nblk, R, w)


def part_slabs(gZa, O, ln_o, nblk, lpn, n_valid=None):
    """The slabs of k_head_bwd: (slabs (nblk, 2 h), mag, inherit, count).  Workgroup b owns the rows node = b (256 / LPN) + tid / LPN
    + j nblk 256 / LPN below n_valid; slab b = [sum gy xhat | sum gy] over them (zeros when it owns none).  mag: the same sums of
    |gy xhat| and |gy|;  inherit: sum |gy| e_xhat (xhat's own error, xhat_bound, through the sum);  count (nblk,): roundings on the
    longest chain of slab b (slab_count)."""
    n = np.shape(O)[0] if n_valid is None else n_valid
    O, gZa = f64(O)[:n], f64(gZa)[:n]
    h, R = O.shape[1], 256 // lpn
    xh = stats(O)[3]
    gy = masked(gZa, O, ln_o)
    e_xh = xhat_bound(O)[0]
    red = lambda t: _by_block(t, nblk, R).sum(axis=(0, 2))
    slabs = red(np.concatenate([gy * xh, gy], axis=1))
    mag = red(np.abs(np.concatenate([gy * xh, gy], axis=1)))
    inherit = red(np.concatenate([np.abs(gy) * e_xh, np.zeros_like(gy)], axis=1))
    return slabs, mag, inherit, slab_count(n, nblk, lpn)


# ------------------------------------------------------------------------------------------------------------------ bounds
# House rule (tests/cheb_f64.py): a bound is TWICE a count of float32 roundings on the longest chain an entry's terms pass
# through, times 2^-24, times the majorant; the factor two is the only slack.  The LayerNorm is not a sum of products, so its
# bound is the first-order propagation of those counted roundings through the expression, doubled in the same way.
def xhat_bound(O):
    """(e_xhat (N, h), rho (N, 1)) before the doubling: the error of xhat and the relative error of rstd.

    mean   (x0 + x1) + (x2 + x3) per lane, then the butterfly of group_sum<LPN>: log2(h) adds deep, each rounding a partial sum of
           at most sum |x|;  times the exact 1 / h:  |dmean| <= delta = log2(h) u mean|x|.  A constant row sums exactly (c + c, 2c + 2c,
           ..): delta = 0, and with it d = 0 and xhat = 0 exactly.
    d      x - mean rounds once: e_d = delta + u |d|.  This is the LayerNorm's conditioning: the kernel is two-pass, so a common
           offset reaches xhat only through delta / sigma = log2(h) u mean|x| / sigma -- a shift of every d of a row by the same delta.
    var    that common shift moves sum d^2 / h by delta^2 only (sum d = 0); each d^2 carries 2 u from d's rounding, the sum is
           <= 4 per-lane fused or unfused multiply-adds + log2(LPN) butterfly adds + the add of eps:  c_v = 5 + log2(LPN) + 1 more.
    rstd   half of var's relative error in var + eps, + sqrt and division at <= 1 ulp = 2 roundings each:
           rho = (delta^2 + (c_v + 2) u var) / (2 (var + eps)) + 4 u.
    xhat   d rstd rounds once:  e_xhat = rstd e_d + |xhat| (rho + u)."""
    x = f64(O)
    h = x.shape[1]
    d, var, rstd, xh = stats(x)
    const = (x.max(axis=1, keepdims=True) == x.min(axis=1, keepdims=True))
    delta = np.where(const, 0.0, log2i(h) * U * np.abs(x).mean(axis=1, keepdims=True))
    c_v = 5 + log2i(h // 4) + 1
    rho = (delta * delta + (c_v + 2) * U * var) / (2.0 * (var + EPS)) + 4.0 * U
    return rstd * (delta + U * np.abs(d)) + np.abs(xh) * (rho + U), rho


def forward_bound(O, ln_o):
    """|Za - model| and |pre - model|: xhat's error through |gamma|; gamma xhat rounds once and the add of beta once (or one fused
    multiply-add): u (2 |gamma xhat| + |beta|); relu is 1-Lipschitz.  Doubled."""
    ln_o = f64(ln_o)
    xh = stats(O)[3]
    return 2.0 * (np.abs(ln_o[0]) * xhat_bound(O)[0] + U * (2.0 * np.abs(ln_o[0] * xh) + np.abs(ln_o[1])))


def near_kink(O, ln_o):
    """Entries whose float64 pre-activation lies within the forward bound of 0: the kernel's mask may differ there."""
    pre = forward(O, ln_o, None, np.shape(O)[1])[2]
    return np.abs(pre) <= forward_bound(O, ln_o)


def backward_bound(gZa, O, ln_o):
    """|gO - model| for a cotangent that is 0 at the near-kink entries.  With gxh = gy gamma (one rounding), S1 = mean|gxh|,
    S2 = mean|gxh xhat|, c_s = 4 + log2(LPN) adds per mean:
      s1  (c_s + 1) u S1            s2  (c_s + 2) u S2 + mean(|gxh| e_xhat)
      T = gxh - s1 - xhat s2, majorant M = |gxh| + S1 + |xhat| S2:
          u |gxh| + ds1 + e_xhat S2 + |xhat| ds2 + u |xhat| S2 (the product) + 2 u M (the two subtractions)
      gO = rstd T: rstd (dT + (rho + u) M).  Doubled."""
    ln_o = f64(ln_o)
    h = np.shape(O)[1]
    _, _, rstd, xh = stats(O)
    e_xh, rho = xhat_bound(O)
    gxh = np.abs(masked(gZa, O, ln_o) * ln_o[0])
    S1, S2 = gxh.mean(axis=1, keepdims=True), (gxh * np.abs(xh)).mean(axis=1, keepdims=True)
    c_s = 4 + log2i(h // 4)
    ds1, ds2 = (c_s + 1) * U * S1, (c_s + 2) * U * S2 + (gxh * e_xh).mean(axis=1, keepdims=True)
    M = gxh + S1 + np.abs(xh) * S2
    dT = U * gxh + ds1 + e_xh * S2 + np.abs(xh) * ds2 + U * np.abs(xh) * S2 + 2.0 * U * M
    return 2.0 * rstd * (dT + (rho + U) * M)


def slab_count(n, nblk, lpn):
    """Roundings on the longest chain of an entry of slab b: a thread adds one product per row it owns -- ceil((n - b R) / (nblk R))
    rows, one rounding for the product and one for the add --, wave_strided_sum<LPN> is log2(64 / LPN) adds, the four waves are
    added in order: 4."""
    R = 256 // lpn
    own = np.maximum(-(-(n - np.arange(nblk) * R) // (nblk * R)), 0)
    return own + 1 + log2i(64 // lpn) + 4


def slab_bound(mag, inherit, count):
    return 2.0 * (count[:, None] * U * mag + inherit)


def colsum_count(nblk):
    """qt_colsum over nblk slabs (tests/gemm_f64.py, wgrad_count): ceil(nblk / 32) + 2 + min(nblk, 32)."""
    return -(-nblk // 32) + 2 + min(nblk, 32)


def psum_bound(mag, inherit, count):
    """The parameter sums after qt_colsum: every slab's own bound, + the column sum's roundings of the summed majorants."""
    nblk = mag.shape[0]
    return slab_bound(mag, inherit, count).sum(axis=0) + 2.0 * colsum_count(nblk) * U * mag.sum(axis=0)


# --------------------------------------------------------------------------------------------------------------- emulation
F = np.float32


def _tree(v):
    """Sum over the last axis as the xor butterfly forms it: adjacent pairs, then pairs of pairs (float32, one rounding each)."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _ln32(x, eps=EPS, ddof=0):
    """layer_norm<LPN> in float32: (xhat (N, LPN, 4), rstd (N,))."""
    N, h = x.shape
    x4 = x.reshape(N, h // 4, 4)
    mean = _tree((x4[..., 0] + x4[..., 1]) + (x4[..., 2] + x4[..., 3])) * F(1.0 / h)
    d = x4 - mean[:, None, None]
    sq = np.zeros((N, h // 4), F)
    for k in range(4):
        sq = sq + d[..., k] * d[..., k]
    var = _tree(sq) * F(1.0 / (h - ddof))
    rstd = F(1.0) / np.sqrt(var + F(eps))
    return d * rstd[:, None, None], rstd


def emulate(O, ln_o, concat, hp, gZa=None, gZb=None, nblk=None, n_valid=None, prev=None, eps=EPS, ddof=0, mask_no_beta=False,
            no_xhat_term=False, count_capacity=False, drop_ragged=False, overwrite=False, gconcat_col=0):
    """float32 emulation of k_head_fwd / k_head_bwd on the (cap, h) input O with n_valid valid rows: dict(Za, Zb, gO, gconcat,
    slabs) over the valid rows.  prev: the slabs before the launch (accumulate = 1).  The keyword flags are the mutations."""
    O, ln_o = np.asarray(O, F), np.asarray(ln_o, F)
    cap, h = O.shape
    n = cap if n_valid is None else n_valid
    lpn = h // 4
    x = O[:n]
    xh, rstd = _ln32(x, eps, ddof)
    gm, bt = ln_o[0].reshape(lpn, 4), ln_o[1].reshape(lpn, 4)
    pre = gm * xh + bt
    out = dict(Za=np.maximum(pre, F(0)).reshape(n, h))
    Zb = np.zeros((n, hp - h), F)
    if concat is not None and hp > h:
        Zb[:, 0] = np.asarray(concat, F).reshape(-1)[:n]
    out['Zb'] = Zb
    if gZa is None:
        return out
    gZa = np.asarray(gZa, F)
    keep = (gm * xh if mask_no_beta else pre) > 0
    gy = np.where(keep, gZa[:n].reshape(n, lpn, 4), F(0))
    gxh = gy * gm
    s1, s2 = np.zeros((n, lpn), F), np.zeros((n, lpn), F)
    for k in range(4):
        s1 = s1 + gxh[..., k]
        s2 = s2 + gxh[..., k] * xh[..., k]
    s1, s2 = _tree(s1) * F(1.0 / h), _tree(s2) * F(1.0 / h)
    t = gxh - s1[:, None, None]
    if not no_xhat_term:
        t = t - xh * s2[:, None, None]
    out['gO'] = (rstd[:, None, None] * t).reshape(n, h)
    out['gconcat'] = None if gZb is None else np.asarray(gZb, F)[:n, gconcat_col].copy()
    # the parameter sums: per thread over its rows in sweep order, wave_strided_sum, then the four waves in order
    terms = np.concatenate([(gy * xh).reshape(n, h), gy.reshape(n, h)], axis=1)
    if count_capacity:          # rows from n_valid to the capacity counted as well, whatever they hold
        xc, _ = _ln32(O[n:], eps, ddof)
        gc = np.asarray(gZa, F)[n:].reshape(cap - n, lpn, 4)
        terms = np.concatenate([terms, np.concatenate([(gc * xc).reshape(cap - n, h), gc.reshape(cap - n, h)], axis=1)])
    R = 256 // lpn
    if drop_ragged:             # the last, incomplete group of 256 / LPN rows left out
        terms = terms[:(terms.shape[0] - 1) // R * R]
    with np.errstate(invalid='ignore'):
        sw = _by_block(terms, nblk, R)
        acc = np.zeros(sw.shape[1:], F)
        for j in range(sw.shape[0]):
            acc = acc + sw[j]
        waves = _tree(np.moveaxis(acc.reshape(nblk, 4, R // 4, 2 * h), 2, -1))           # (nblk, 4, 2 h)
        s = np.zeros((nblk, 2 * h), F)
        for w in range(4):
            s = s + waves[:, w]
    out['slabs'] = s if (prev is None or overwrite) else np.asarray(prev, F) + s
    return out


# ------------------------------------------------------------------------------------------------------------------- cases
FAMILIES = ('randn', 'small', 'offset', 'const')


def draw_rows(rng, family, N, h):
    """randn rows; rows of std 0.01 (eps = 1e-5 is 10 % of the variance); rows 1000 + randn; constant rows."""
    if family == 'randn':
        x = rng.standard_normal((N, h))
    elif family == 'small':
        x = 0.01 * rng.standard_normal((N, h))
    elif family == 'offset':
        x = 1000.0 + rng.standard_normal((N, h))
    else:
        x = np.repeat(rng.standard_normal((N, 1)), h, axis=1)
    return x.astype(np.float32)


def _case(h, N, family='randn', view=False, cap=None, concat=True, single=False, seed=0):
    name = f'h{h}-N{N}-{family}-{"view" if view else "dense"}-{"cap%d" % cap if cap else "exact"}-{"cat" if concat else "nocat"}' + ('-single' if single else '')
    return dict(name=name, h=h, N=N, family=family, view=view, cap=cap, concat=concat, single=single, hp=h + 4,
                seed=seed + 1000 * h + 7 * N + FAMILIES.index(family))


def _cases():
    out = []
    for i, h in enumerate(HIDDEN):
        for N in ROWS:                                     # every hidden size at every row count
            out.append(_case(h, N, view=N in (37, 70001), concat=N != 37))
        out.append(_case(h, 777, 'small', view=True))
        out.append(_case(h, 777, 'offset', cap=1100, view=i % 2 == 0))
        out.append(_case(h, 37, 'const', view=i % 2 == 1, concat=False))
        out.append(_case(h, 777, 'randn', cap=1100, view=i % 2 == 1, concat=i % 2 == 0))
    out.append(_case(16, 70001, 'randn', view=True, cap=70400))
    out.append(_case(16, 777, 'randn', single=True))
    out.append(_case(16, 777, 'randn', single=True, cap=1100, concat=False))
    return out


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def inputs(case):
    """The float32 inputs of a case over its valid rows: O, ln (2, h), concat (N, 1) or None, gZa, gZb (N, hp - h), and `near`, the
    entries left out at the ReLU kink -- gZa is 0 there."""
    rng = np.random.default_rng(case['seed'])
    h, N = case['h'], case['N']
    O = draw_rows(rng, case['family'], N, h)
    ln = np.stack([rng.choice([-1.0, 1.0], size=h) * (0.5 + rng.random(h)), 0.5 * rng.standard_normal(h)]).astype(np.float32)
    concat = rng.standard_normal((N, 1)).astype(np.float32) if case['concat'] else None
    gZa = rng.standard_normal((N, h)).astype(np.float32)
    gZb = rng.standard_normal((N, case['hp'] - h)).astype(np.float32)
    near = near_kink(O, ln)
    gZa[near] = 0.0
    return dict(O=O, ln=ln, concat=concat, gZa=gZa, gZb=gZb, near=near)
