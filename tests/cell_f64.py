"""The peephole LSTM cell of csrc/qt_cell.h in numpy float64, written from the definitions (tests/tcell_f64.py's docstring,
model/model.py's cell):

    I = sigmoid(g_i + w_ci C + b_i)     F = sigmoid(g_f + w_cf C + b_f)     T = tanh(g_c + b_c)        g = G (+ G2, added first)
    C'raw = F C + I T                   Og = sigmoid(g_o + w_co C'raw + b_o)    H'raw = Og tanh(C'raw)
    H' = gamma_h xhat(H'raw) + beta_h   C' = gamma_c xhat(C'raw) + beta_c    (ln (4, h) given; else H' = H'raw, C' = C'raw)

and its backward from the STORED float32 gate activations (I | F | T | Og), as k_lstm_bwd, k_dgrad_cell and k_cell_bwd_fused read
them: C'raw is recomputed from them, so the backward's error is its own.  The eleven parameter sums come in the kernels' order
w_c i, f, o | b i, f, c, o | gamma_h, beta_h, gamma_c, beta_c.  A None operand is what cell_bwd_load / cell_params make of a null
pointer: Cprev, gO, gHn, gCn, gHn2 zeros; ln: gamma = 1, beta = 0 and no LayerNorm at all.

Ownership of the per-workgroup `part` rows (owned()):
  k_lstm_bwd        head_f64._by_block: workgroup b owns node = b R + r + j nblk R (R = 256 / LPN), the grid of qt_lstm_bwd_blocks
  k_dgrad_cell      fixed: workgroup b owns the 128 rows [128 b, 128 b + 128), thread slot r = tid / LPN takes rows r, r + R, ..;
                    a workgroup whose first row is past the valid count returns before it writes its part row
  k_cell_bwd_fused  fixed: with ntiles = ceil(n / TR) tiles of TR rows (TR = 64 for <= 3 column tiles of the data gradient, else
                    128) workgroup b of `grid` owns the tiles [ntiles b / grid, ntiles (b + 1) / grid); the grid is
                    min(2 CUs, ceil(cap / 64)) resp. min(CUs, ceil(cap / 128)).  A workgroup without a tile writes zeros
                    (accumulate = 0) or nothing.  Its weight-gradient slab is A^T gG over the same rows.
All three are fixed functions of blockIdx, so `part` and `slab` compare workgroup by workgroup.

The bounds live in the middle, each with the count of float32 roundings it stands for; emulate_forward / emulate_backward are a
float32 numpy emulation of the kernels' arithmetic (fma where the kernel pins one, the trees of group_sum, wave_strided_sum and
block_param_reduce, v_exp_f32 / v_rcp_f32 as the correctly rounded value pushed by -1, 0 or +1 ulp) with the mutations
tests/test_cell_f64_host.py measures.  CASES is the case table of tests/test_gpu_cell_f64.py.  numpy only; nothing of qtmpnn."""
import numpy as np

import gemm_f64
from head_f64 import EPS, U, _by_block, _ln32, _tree, bwd_blocks, f64, log2i, slab_count, stats, xhat_bound

HIDDEN = (8, 16, 32, 64, 128)
TINY = 2.0 ** -126      # smallest normal float32: v_exp_f32 / v_rcp_f32 may flush what lies below it
THR = 0.125             # tanhf_: |x| < 1/8 takes the odd series
DGRAD_ROWS = 128        # BM of qt_gemm.h: the rows of a workgroup of k_dgrad_cell
F = np.float32


# ------------------------------------------------------------------------------------------------------------------- model
def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _quarters(a, h):
    return [a[:, k * h:(k + 1) * h] for k in range(4)]


def forward(G, G2, Cprev, wc, b, ln):
    """dict(I, F, T, Og, Cr, Hr, Hn, Cn, pre = (p_i, p_f, p_c, p_o)), each (N, h)."""
    G, wc, b = f64(G), f64(wc), f64(b)
    N, h = G.shape[0], G.shape[1] // 4
    g = G if G2 is None else f64(G2) + G
    cp = np.zeros((N, h)) if Cprev is None else f64(Cprev)
    gi, gf, gc, go = _quarters(g, h)
    pi, pf, pc = gi + wc[0] * cp + b[0], gf + wc[1] * cp + b[1], gc + b[2]
    I, Fg, T = sigmoid(pi), sigmoid(pf), np.tanh(pc)
    Cr = Fg * cp + I * T
    po = go + wc[2] * Cr + b[3]
    Og = sigmoid(po)
    Hr = Og * np.tanh(Cr)
    Hn, Cn = Hr, Cr
    if ln is not None:
        ln = f64(ln)
        Hn, Cn = ln[0] * stats(Hr)[3] + ln[1], ln[2] * stats(Cr)[3] + ln[3]
    return dict(I=I, F=Fg, T=T, Og=Og, Cr=Cr, Hr=Hr, Hn=Hn, Cn=Cn, pre=(pi, pf, pc, po))


def _ln_bwd(gy, gamma, xh, rstd):
    gxh = gy * gamma
    return rstd * (gxh - gxh.mean(axis=1, keepdims=True) - xh * (gxh * xh).mean(axis=1, keepdims=True))


def _bwd_operands(gates, Cprev, gO, gHn, gCn, gHn2):
    gates = f64(gates)
    N, h = gates.shape[0], gates.shape[1] // 4
    z = np.zeros((N, h))
    opt = lambda a: z if a is None else f64(a)
    gyh = opt(gHn) if gHn2 is None else opt(gHn) + f64(gHn2)
    return _quarters(gates, h), opt(Cprev), opt(gO), gyh, opt(gCn)


def backward_terms(gates, Cprev, gO, gHn, gCn, wc, ln, gHn2=None):
    """(gG (N, 4h), gCprev (N, h), terms (N, 11 h)): terms[:, a h + j] is row n's addend of parameter sum a, channel j."""
    (I, Fg, T, Og), cp, go, gyh, gyc = _bwd_operands(gates, Cprev, gO, gHn, gCn, gHn2)
    wc = f64(wc)
    Cr = Fg * cp + I * T
    tc = np.tanh(Cr)
    Hr = Og * tc
    xh, xc, gHr, gCr = 0.0 * Hr, 0.0 * Cr, gyh, gyc
    if ln is not None:
        ln = f64(ln)
        _, _, rh, xh = stats(Hr)
        _, _, rc, xc = stats(Cr)
        gHr, gCr = _ln_bwd(gyh, ln[0], xh, rh), _ln_bwd(gyc, ln[2], xc, rc)
    gOt = go + gHr * tc
    ggo = gOt * Og * (1.0 - Og)
    gc = gCr + gHr * Og * (1.0 - tc * tc) + ggo * wc[2]
    ggi, ggf, ggc = gc * T * I * (1.0 - I), gc * cp * Fg * (1.0 - Fg), gc * I * (1.0 - T * T)
    gcp = gc * Fg + ggi * wc[0] + ggf * wc[1]
    terms = np.concatenate([ggi * cp, ggf * cp, ggo * Cr, ggi, ggf, ggc, ggo, gyh * xh, gyh, gyc * xc, gyc], axis=1)
    return np.concatenate([ggi, ggf, ggc, ggo], axis=1), gcp, terms


def backward(gates, Cprev, gO, gHn, gCn, wc, ln, gHn2=None):
    """(gG (N, 4h), gCprev (N, h), psum (11 h,))."""
    gG, gcp, terms = backward_terms(gates, Cprev, gO, gHn, gCn, wc, ln, gHn2)
    return gG, gcp, terms.sum(axis=0)


# --------------------------------------------------------------------------------------------------------------- ownership
def fused_tile_rows(nt):
    """fused_tile_rows of gatecell.hip: nt = 32-column tiles of the data gradient."""
    return 64 if nt <= 3 else 128


def fused_grid(cap, nt, n_cu):
    return min(2 * n_cu, -(-cap // 64)) if fused_tile_rows(nt) == 64 else min(n_cu, -(-cap // 128))


def launch_bwd(cap, h):
    return dict(kind='bwd', nblk=bwd_blocks(cap, h), nw=4)


def launch_dgrad(cap, h):
    return dict(kind='dgrad', nblk=-(-cap // DGRAD_ROWS), nw=4)


def launch_fused(cap, h, nt, n_cu):
    tr = fused_tile_rows(nt)
    return dict(kind='fused', nblk=fused_grid(cap, nt, n_cu), tr=tr, nw=4 * tr // 64)


def row_index(launch, n, lpn):
    """(sweeps, nblk, slots) int: the row that thread slot r = tid / LPN of workgroup b takes in its j-th trip, or n for none."""
    nblk, kind = launch['nblk'], launch['kind']
    if kind == 'bwd':
        R = 256 // lpn
        sweeps = max(-(-n // (nblk * R)), 1)
        idx = np.arange(sweeps * nblk * R).reshape(sweeps, nblk, R)
    elif kind == 'dgrad':
        R = 256 // lpn
        idx = np.arange(nblk * DGRAD_ROWS).reshape(nblk, DGRAD_ROWS // R, R).transpose(1, 0, 2)
    else:
        tr = launch['tr']
        ntiles = -(-n // tr)
        t0 = [ntiles * b // nblk for b in range(nblk + 1)]
        sweeps = max(max(t0[b + 1] - t0[b] for b in range(nblk)), 1)
        idx = np.full((sweeps, nblk, 4 * tr // lpn), n, np.int64)          # 4 TR threads; the slots past TR stay idle
        for b in range(nblk):
            for j in range(t0[b + 1] - t0[b]):
                idx[j, b, :tr] = (t0[b] + j) * tr + np.arange(tr)
    return np.minimum(idx, n)


def written(launch, n):
    """(nblk,) bool: the workgroups that write their part row with accumulate = 0 (k_dgrad_cell returns early past the valid rows;
    k_cell_bwd_fused writes zeros without a tile; k_lstm_bwd always writes)."""
    b = np.arange(launch['nblk'])
    return b * DGRAD_ROWS < n if launch['kind'] == 'dgrad' else np.ones(launch['nblk'], bool)


def owned(t, launch, n, lpn):
    """(n, w) row terms -> (sweeps, nblk, slots, w) as row_index places them (zeros where there is no row)."""
    if launch['kind'] == 'bwd':
        return _by_block(t[:n], launch['nblk'], 256 // lpn)
    pad = np.concatenate([t[:n], np.zeros((1, t.shape[1]), t.dtype)])
    return pad[row_index(launch, n, lpn)]


def part_count(launch, n, lpn):
    """Roundings on the longest chain of an entry of part row b: one for the product, one add per row the thread owns, the
    log2(64 / LPN) adds of wave_strided_sum, the NW waves added in order (head_f64.slab_count, whose NW is 4)."""
    if launch['kind'] == 'bwd':
        return slab_count(n, launch['nblk'], lpn)
    own = (row_index(launch, n, lpn) < n).any(axis=2).sum(axis=0)
    return own + 1 + log2i(64 // lpn) + launch['nw']


# ------------------------------------------------------------------------------------------------------------------ bounds
# House rule (tests/cheb_f64.py, tests/head_f64.py): a bound is TWICE a count of float32 roundings on the longest chain, times
# 2^-24, times the majorant; expressions that are no sums get the first-order propagation of the counted roundings, doubled the
# same way.  The e_* below are the undoubled errors; the doubling happens where a bound leaves this file.
def sig_own(x, s):
    """|sigmoidf_(x) - sigmoid(x)| for an exact float32 x, absolute.  t = fl(-L x): the constant L = log2(e) and the product round
    once each, u |t| absolute in the exponent, which 2^t turns into ln 2 u |t| = u |x| relative: 2 |x| u.  v_exp_f32 is 1 ulp = 2 u:
    E = 2^t carries (2 |x| + 2) u relative.  D = 1 + E rounds once, and E's error weighs E / (1 + E) = 1 - s in it.  v_rcp_f32: 2 u.
    Relative (1 - s)(2 |x| + 2) u + 3 u, so absolute  u [s (1 - s)(2 |x| + 2) + 3 s]  (7 roundings), + TINY for a flushed result.
    Relative to s this grows as 2 |x| + 5 roundings for negative x: the bound is absolute on purpose."""
    return U * (s * (1.0 - s) * (2.0 * np.abs(x) + 2.0) + 3.0 * s) + TINY


def tanh_own(x, th, e_x):
    """|tanhf_(x') - tanh(x')| absolute, for the kernel's own argument x' within 2 e_x of x.
    |x| >= 1/8:  1 - 2 rcp(1 + exp2(fl(2L |x|))).  The exponent: constant and product, 2 (2 |x|) u relative in E, + 2 u of
      v_exp_f32; 1 + E rounds once, E's share is E / (1 + E) = (1 + th) / 2; rcp 2 u; q = 2 / (1 + E) = 1 - th carries
      (4 |x| + 2)(1 + th) / 2 u + 3 u; 1 - q rounds once, u th:   u [(1 - th^2)(2 |x| + 1) + 3 (1 - th) + th]   (8 roundings;
      <= 3.98 u = 2.4e-7, the most at |x| = 1/8).
    |x| < 1/8:   |x| P, P = 1 + x2 (c3 + x2 (c5 + x2 c7)), x2 = fl(x x).  Relative: the product and the last fma, 2 u; per
      coefficient its rounding, x2's rounding times its power and the fma that adds it: 3 |c3| x2 + 4 |c5| x2^2 + 5 |c7| x2^3;
      the series stops after x^7: the next term is 62 / 2835 |x|^9.
    Within 2 e_x of the threshold the kernel may take either branch: the larger of the two."""
    ax, x2, ta = np.abs(x), x * x, np.abs(th)
    big = U * ((1.0 - ta * ta) * (2.0 * ax + 1.0) + 3.0 * (1.0 - ta) + ta) + TINY
    small = ta * U * (2.0 + 3.0 * x2 / 3.0 + 4.0 * x2 * x2 * 2.0 / 15.0 + 5.0 * x2 ** 3 * 17.0 / 315.0) + 62.0 / 2835.0 * ax ** 9
    m = 2.0 * e_x
    return np.where(ax < THR - m, small, np.where(ax >= THR + m, big, np.maximum(small, big)))


def xhat_err(x, e_x):
    """(e_xhat, rho): head_f64.xhat_bound on the float64 x, + what an error e_x of x itself adds at first order:
    d moves by at most e_x + mean(e_x); rstd moves relatively by rstd mean(|xhat| |dd|)."""
    _, _, rstd, xh = stats(x)
    e0, rho = xhat_bound(x)
    ed = e_x + e_x.mean(axis=1, keepdims=True)
    r = rstd * (np.abs(xh) * ed).mean(axis=1, keepdims=True)
    return e0 + rstd * ed + np.abs(xh) * r, rho + r


def _ln_out_err(x, e_x, gamma, beta):
    """gamma xhat + beta: xhat's error through |gamma|, the product and the add round once each (head_f64.forward_bound)."""
    xh = stats(x)[3]
    return np.abs(gamma) * xhat_err(x, e_x)[0] + U * (2.0 * np.abs(gamma * xh) + np.abs(beta))


def forward_bounds(G, G2, Cprev, wc, b, ln):
    """dict of |kernel - model| per output (doubled): I, F, T, Og, Cr, Hr, Hn, Cn.
    pre-activation  g (+ g2) + w_c c + b: a product and two adds (+ 1 with G2): 3 (4) roundings of sum |terms|; the cell gate has
                    one add (2).  The output gate inherits |w_co| e_Cr.
    gates           sigma'(p) e_p + sig_own;  (1 - T^2) e_p + tanh_own
    C'raw           fma(F, c, fl(I T)): |c| e_F + |T| e_I + I e_T + u (|I T| + |C'raw|)           (2 roundings)
    H'raw           Og tanh(C'raw): |tc| e_Og + Og e_tc + u |H'raw|                                (1 rounding)"""
    m = forward(G, G2, Cprev, wc, b, ln)
    G, wc, b = f64(G), f64(wc), f64(b)
    N, h = G.shape[0], G.shape[1] // 4
    two = 0 if G2 is None else 1
    aG = np.abs(G) if G2 is None else np.abs(G) + np.abs(f64(G2))
    cp = np.zeros((N, h)) if Cprev is None else f64(Cprev)
    ai, af, ac, ao = _quarters(aG, h)
    pi, pf, pc, po = m['pre']
    I, Fg, T, Og, Cr, Hr = m['I'], m['F'], m['T'], m['Og'], m['Cr'], m['Hr']
    e_pi = (3 + two) * U * (ai + np.abs(wc[0] * cp) + np.abs(b[0]))
    e_pf = (3 + two) * U * (af + np.abs(wc[1] * cp) + np.abs(b[1]))
    e_pc = (1 + two) * U * (ac + np.abs(b[2]))
    e_I = I * (1.0 - I) * e_pi + sig_own(pi, I)
    e_F = Fg * (1.0 - Fg) * e_pf + sig_own(pf, Fg)
    e_T = (1.0 - T * T) * e_pc + tanh_own(pc, T, e_pc)
    e_Cr = np.abs(cp) * e_F + np.abs(T) * e_I + I * e_T + U * (np.abs(I * T) + np.abs(Cr))
    e_po = (3 + two) * U * (ao + np.abs(wc[2] * Cr) + np.abs(b[3])) + np.abs(wc[2]) * e_Cr
    e_Og = Og * (1.0 - Og) * e_po + sig_own(po, Og)
    tc = np.tanh(Cr)
    e_tc = (1.0 - tc * tc) * e_Cr + tanh_own(Cr, tc, e_Cr)
    e_Hr = np.abs(tc) * e_Og + Og * e_tc + U * np.abs(Hr)
    e_Hn, e_Cn = e_Hr, e_Cr
    if ln is not None:
        ln = f64(ln)
        e_Hn, e_Cn = _ln_out_err(Hr, e_Hr, ln[0], ln[1]), _ln_out_err(Cr, e_Cr, ln[2], ln[3])
    return {k: 2.0 * v for k, v in dict(I=e_I, F=e_F, T=e_T, Og=e_Og, Cr=e_Cr, Hr=e_Hr, Hn=e_Hn, Cn=e_Cn).items()}


def _ln_bwd_err(gy, e_gy, gamma, x, e_x):
    """layer_norm_bwd as head_f64.backward_bound counts it (c_s = 4 + log2(LPN) adds per mean), with an inherited error of gy
    and of x.  (e_gx, e_xhat)"""
    h = x.shape[1]
    _, _, rstd, xh = stats(x)
    e_xh, rho = xhat_err(x, e_x)
    mean = lambda a: a.mean(axis=1, keepdims=True)
    gxh = np.abs(gy * gamma)
    e_gxh = np.abs(gamma) * e_gy + U * gxh                                  # one product
    S1, S2 = mean(gxh), mean(gxh * np.abs(xh))
    c_s = 4 + log2i(h // 4)
    ds1 = c_s * U * S1 + mean(e_gxh)
    ds2 = (c_s + 1) * U * S2 + mean(e_gxh * np.abs(xh) + gxh * e_xh)
    M = gxh + S1 + np.abs(xh) * S2
    dT = e_gxh + ds1 + e_xh * S2 + np.abs(xh) * ds2 + U * np.abs(xh) * S2 + 2.0 * U * M
    return rstd * (dT + (rho + U) * M), e_xh


def backward_bounds(gates, Cprev, gO, gHn, gCn, wc, ln, gHn2=None):
    """dict(gG (N, 4h), gCprev (N, h)) doubled, and e_terms (N, 11 h) UNDOUBLED: the error each row's addend of a parameter sum
    carries before it is summed (the `inherit` of head_f64.slab_bound).  Statement by statement through cell_backward:
      Cr    fma(F, c, fl(I T)) of exact operands: u (|I T| + |Cr|)                                     2
      tc    (1 - tc^2) e_Cr + tanh_own;   Hr = Og tc: Og e_tc + u |Hr|                                1
      gyh   gHn + gHn2 rounds once (with a second gradient)                                           1
      gOt   go + gHr tc: |tc| e_gHr + |gHr| e_tc + 2 u (|go| + |gHr tc|)                              2
      w     1 - tc tc: 2 |tc| e_tc + u (tc^2 + |w|)                                                   2
      gc_a  gCr + (gHr Og) w: e_gCr + |Og w| e_gHr + |gHr Og| e_w + 2 u |gHr Og w| + u (|gCr| + |gHr Og w|)   3
      ggo   gOt Og (1 - Og): Og (1 - Og) e_gOt + 3 u |ggo|                                            3
      gc_   gc_a + ggo w_co: e_gc_a + |w_co| e_ggo + 2 u (|gc_a| + |ggo w_co|)                        2
      ggi   gc_ T I (1 - I): |T I (1 - I)| e_gc + 4 u |ggi|;   ggf the same with c for T              4
      ggc   gc_ I (1 - T T): |I w2| e_gc + |gc_ I| u (T^2 + |w2|) + 2 u |ggc|                         4
      gcp   gc_ F + ggi w_ci + ggf w_cf: F e_gc + |w_ci| e_ggi + |w_cf| e_ggf + 3 u (sum |terms|)     3"""
    (I, Fg, T, Og), cp, go, gyh, gyc = _bwd_operands(gates, Cprev, gO, gHn, gCn, gHn2)
    ws = f64(wc)
    wa, A = np.abs(ws), np.abs
    Cr = Fg * cp + I * T
    e_Cr = U * (A(I * T) + A(Cr))
    tc = np.tanh(Cr)
    e_tc = (1.0 - tc * tc) * e_Cr + tanh_own(Cr, tc, e_Cr)
    Hr = Og * tc
    e_Hr = Og * e_tc + U * A(Hr)
    z = 0.0 * Hr
    e_gyh = U * A(gyh) if gHn2 is not None else z
    xh, xc, gHr, gCr, e_gHr, e_gCr, e_xh, e_xc = z, z, gyh, gyc, e_gyh, z, z, z
    if ln is not None:
        ln = f64(ln)
        xh, xc = stats(Hr)[3], stats(Cr)[3]
        gHr, gCr = _ln_bwd(gyh, ln[0], xh, stats(Hr)[2]), _ln_bwd(gyc, ln[2], xc, stats(Cr)[2])
        e_gHr, e_xh = _ln_bwd_err(gyh, e_gyh, ln[0], Hr, e_Hr)
        e_gCr, e_xc = _ln_bwd_err(gyc, z, ln[2], Cr, e_Cr)
    gOt = go + gHr * tc
    e_gOt = A(tc) * e_gHr + A(gHr) * e_tc + 2.0 * U * (A(go) + A(gHr * tc))
    w = 1.0 - tc * tc
    e_w = 2.0 * A(tc) * e_tc + U * (tc * tc + A(w))
    pr = gHr * Og * w
    gca = gCr + pr
    e_gca = e_gCr + A(Og * w) * e_gHr + A(gHr * Og) * e_w + 2.0 * U * A(pr) + U * (A(gCr) + A(pr))
    ggo = gOt * Og * (1.0 - Og)
    e_ggo = Og * (1.0 - Og) * e_gOt + 3.0 * U * A(ggo)
    gc = gca + ggo * ws[2]
    e_gc = e_gca + wa[2] * e_ggo + 2.0 * U * (A(gca) + A(ggo * ws[2]))
    ggi, ggf = gc * T * I * (1.0 - I), gc * cp * Fg * (1.0 - Fg)
    e_ggi = A(T * I * (1.0 - I)) * e_gc + 4.0 * U * A(ggi)
    e_ggf = A(cp * Fg * (1.0 - Fg)) * e_gc + 4.0 * U * A(ggf)
    w2 = 1.0 - T * T
    ggc = gc * I * w2
    e_ggc = A(I * w2) * e_gc + A(gc * I) * U * (T * T + A(w2)) + 2.0 * U * A(ggc)
    e_gcp = Fg * e_gc + wa[0] * e_ggi + wa[1] * e_ggf + 3.0 * U * (A(gc * Fg) + A(ggi * ws[0]) + A(ggf * ws[1]))
    e_terms = np.concatenate([A(cp) * e_ggi, A(cp) * e_ggf, A(Cr) * e_ggo + A(ggo) * e_Cr, e_ggi, e_ggf, e_ggc, e_ggo,
                              A(xh) * e_gyh + A(gyh) * e_xh, e_gyh, A(gyc) * e_xc, z], axis=1)
    return dict(gG=2.0 * np.concatenate([e_ggi, e_ggf, e_ggc, e_ggo], axis=1), gCprev=2.0 * e_gcp, e_terms=e_terms)


def part_rows(terms, e_terms, launch, n, lpn):
    """(part (nblk, 11 h), bound): the model's part rows and their bound  2 (count u sum |terms| + sum e_terms)  (head_f64.slab_bound),
    over the rows each workgroup owns."""
    red = lambda t: owned(t, launch, n, lpn).sum(axis=(0, 2))
    count = part_count(launch, n, lpn)
    return red(terms), 2.0 * (count[:, None] * U * red(np.abs(terms)) + red(e_terms))


def wslab(A, gG, e_gG, launch, n):
    """The fused launch's weight-gradient slabs (nblk, Kt, 4h) = A^T gG over each workgroup's rows, and their bound: gemm_f64's
    wgrad rule -- the MFMA chain takes one fused multiply-add per row of the workgroup's tiles, in row order (TR per tile), and
    the result is added to the slab: TR tiles + 1 roundings of |A|^T |gG|, doubled -- + gG's own error through |A|^T."""
    tr, nblk = launch['tr'], launch['nblk']
    ntiles = -(-n // tr)
    out, bound = [], []
    for b in range(nblk):
        t0, t1 = ntiles * b // nblk, ntiles * (b + 1) // nblk
        rows = slice(min(t0 * tr, n), min(t1 * tr, n))
        s, mag = gemm_f64.wgrad(f64(A)[None], None, gG, rows)
        out.append(s)
        bound.append(2.0 * (((t1 - t0) * tr + 1) * U * mag + np.abs(f64(A)[rows]).T @ (0.5 * e_gG[rows])))
    return np.stack(out), np.stack(bound)


# --------------------------------------------------------------------------------------------------------------- emulation
L2E, L2E2 = F(1.4426950408889634), F(2.8853900817779268)
C3, C5, C7 = F(-1.0 / 3.0), F(2.0 / 15.0), F(-17.0 / 315.0)
PUSHES = [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]          # (v_exp_f32, v_rcp_f32) off the correctly rounded value, in ulp


def _push(true, k):
    """The float64 value rounded to float32 and moved k ulp; a value float32 holds exactly (2^0, 1 / 1, 1 / inf) stays as it is."""
    v = true.astype(F)
    if k == 0:
        return v
    ok = np.isfinite(v) & (v > 0) & (v.astype(np.float64) != true)
    return np.where(ok, np.nextafter(v, F(np.inf if k > 0 else -np.inf)), v).astype(F)


def _exp2(t, k):
    with np.errstate(over='ignore', under='ignore'):
        return _push(np.exp2(t.astype(np.float64)), k)


def _rcp(x, k):
    with np.errstate(over='ignore', under='ignore', divide='ignore'):
        return _push(1.0 / x.astype(np.float64), k)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def sig32(x, push=(0, 0)):
    return _rcp(F(1) + _exp2(-L2E * x, push[0]), push[1])


def tanh32(x, push=(0, 0), no_x5=False, thr=THR):
    ax, x2 = np.abs(x), x * x
    big = F(1) - F(2) * _rcp(F(1) + _exp2(L2E2 * ax, push[0]), push[1])
    small = ax * _fma(x2, _fma(x2, _fma(x2, C7, F(0) if no_x5 else C5), C3), F(1))
    return np.copysign(np.where(ax < F(thr), small, big), x).astype(F)


def _ln(x, eps):
    xh, rstd = _ln32(x, eps)
    return xh.reshape(x.shape), rstd[:, None]


def _f32(a):
    return None if a is None else np.asarray(a, F)


def emulate_forward(G, G2, Cprev, wc, b, ln, push=(0, 0), eps=EPS, o_reads_c=False, no_g2=False, no_x5=False, thr=THR):
    """float32 emulation of k_lstm_fwd: dict(I, F, T, Og, Hn, Cn).  The keyword flags are the mutations."""
    G, wc, b = _f32(G), _f32(wc), _f32(b)
    N, h = G.shape[0], G.shape[1] // 4
    g = G if (G2 is None or no_g2) else G + _f32(G2)
    cp = np.zeros((N, h), F) if Cprev is None else _f32(Cprev)
    gi, gf, gc, go = _quarters(g, h)
    I = sig32(gi + wc[0] * cp + b[0], push)
    Fg = sig32(gf + wc[1] * cp + b[1], push)
    T = tanh32(gc + b[2], push, no_x5, thr)
    Cr = _fma(Fg, cp, I * T)
    Og = sig32(go + wc[2] * (cp if o_reads_c else Cr) + b[3], push)
    Hr = Og * tanh32(Cr, push, no_x5, thr)
    Hn, Cn = Hr, Cr
    if ln is not None:
        ln = _f32(ln)
        Hn, Cn = ln[0] * _ln(Hr, eps)[0] + ln[1], ln[2] * _ln(Cr, eps)[0] + ln[3]
    return dict(I=I, F=Fg, T=T, Og=Og, Hn=Hn, Cn=Cn)


def _ln_bwd32(gy, gamma, xh, rstd):
    N, h = gy.shape
    gxh = gy * gamma
    g4, x4 = gxh.reshape(N, h // 4, 4), xh.reshape(N, h // 4, 4)
    s1, s2 = np.zeros((N, h // 4), F), np.zeros((N, h // 4), F)
    for k in range(4):
        s1 = s1 + g4[..., k]
        s2 = s2 + g4[..., k] * x4[..., k]
    s1, s2 = (_tree(s1) * F(1.0 / h))[:, None], (_tree(s2) * F(1.0 / h))[:, None]
    return rstd * (gxh - s1 - xh * s2)


def _cell_bwd32(gates, cp, go, gyh, gyc, wc, ln, push, eps, no_wco, tc_lin, no_wcf, no_x5, thr):
    I, Fg, T, Og = _quarters(gates, gates.shape[1] // 4)
    Cr = _fma(Fg, cp, I * T)
    tc = tanh32(Cr, push, no_x5, thr)
    Hr = Og * tc
    xh, xc, gHr, gCr = np.zeros_like(Hr), np.zeros_like(Cr), gyh, gyc
    if ln is not None:
        xh, rh = _ln(Hr, eps)
        xc, rc = _ln(Cr, eps)
        gHr, gCr = _ln_bwd32(gyh, ln[0], xh, rh), _ln_bwd32(gyc, ln[2], xc, rc)
    gOt = go + gHr * tc
    gc = gCr + gHr * Og * (F(1) - (tc if tc_lin else tc * tc))
    ggo = gOt * Og * (F(1) - Og)
    if not no_wco:
        gc = gc + ggo * wc[2]
    ggi, ggf, ggc = gc * T * I * (F(1) - I), gc * cp * Fg * (F(1) - Fg), gc * I * (F(1) - T * T)
    gcp = gc * Fg + ggi * wc[0]
    if not no_wcf:
        gcp = gcp + ggf * wc[1]
    terms = np.concatenate([ggi * cp, ggf * cp, ggo * Cr, ggi, ggf, ggc, ggo, gyh * xh, gyh, gyc * xc, gyc], axis=1)
    return np.concatenate([ggi, ggf, ggc, ggo], axis=1), gcp, terms


def emulate_backward(gates, Cprev, gO, gHn, gCn, wc, ln, gHn2=None, launch=None, n_valid=None, prev=None, push=(0, 0), eps=EPS,
                     no_wco=False, tc_lin=False, no_wcf=False, no_x5=False, thr=THR, drop_ragged=False, count_capacity=False,
                     overwrite=False):
    """float32 emulation of a backward launch on (cap, ..) operands with n_valid valid rows: dict(gG, gCprev, part) -- gG and
    gCprev over the valid rows, part (nblk, 11 h) as `launch` (launch_bwd / launch_dgrad / launch_fused) owns the rows: per thread
    the running sum over its rows in trip order, the pair tree of wave_strided_sum, the NW waves in order.  prev: the part rows
    before the launch (accumulate = 1).  The keyword flags are the mutations."""
    gates, wc, ln = _f32(gates), _f32(wc), _f32(ln)
    cap, h = gates.shape[0], gates.shape[1] // 4
    n = cap if n_valid is None else n_valid
    z = np.zeros((cap, h), F)
    opt = lambda a: z if a is None else _f32(a)
    gyh = opt(gHn) if gHn2 is None else opt(gHn) + _f32(gHn2)
    with np.errstate(invalid='ignore'):
        gG, gcp, terms = _cell_bwd32(gates, opt(Cprev), opt(gO), gyh, opt(gCn), wc, ln, push, eps, no_wco, tc_lin, no_wcf, no_x5, thr)
    out = dict(gG=gG[:n], gCprev=gcp[:n])
    if launch is None:
        return out
    lpn = h // 4
    m = cap if count_capacity else n                   # rows from n_valid to the capacity counted as well, whatever they hold
    if drop_ragged:                                    # the last, incomplete group of a workgroup's thread slots left out
        R = 256 // lpn if launch['kind'] != 'fused' else launch['tr']
        m = (m - 1) // R * R
    with np.errstate(invalid='ignore'):
        sw = owned(terms, launch, m, lpn)
        acc = np.zeros(sw.shape[1:], F)
        for j in range(sw.shape[0]):
            acc = acc + sw[j]
        nblk, R, W = acc.shape
        nw = launch['nw']
        waves = _tree(np.moveaxis(acc.reshape(nblk, nw, R // nw, W), 2, -1))
        s = np.zeros((nblk, W), F)
        for k in range(nw):
            s = s + waves[:, k]
        if prev is not None:
            wr = written(launch, n)[:, None] if launch['kind'] == 'dgrad' else True
            s = np.where(wr, s if overwrite else _f32(prev) + s, _f32(prev))
    out['part'] = s
    return out


# ------------------------------------------------------------------------------------------------------------------- cases
KINDS = ('live', 'sat', 'branch', 'const')
SWEEP2 = {h: 512 * 256 // (h // 4) + 37 for h in HIDDEN}          # the 512-workgroup grid's second sweep, its last group ragged


def draw(rng, *shape):
    """sign (0.5 + U[0, 1)) as float32: no term of a sum is small against its neighbours."""
    return (rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))).astype(F)


def branch_grid():
    """The 40 float32 values on each side of +-0.125, +-0.125 themselves and +-0: 164 tanh arguments."""
    up = [np.float32(THR)]
    for _ in range(40):
        up.append(np.nextafter(up[-1], F(1)))
    dn = [np.float32(THR)]
    for _ in range(40):
        dn.append(np.nextafter(dn[-1], F(0)))
    v = np.array(dn[:0:-1] + up, F)
    return np.concatenate([v, -v, np.array([0.0, -0.0], F)])


def _case(h, N, kind='live', g2=False, cprev=True, ln=True, go=True, gcn=True, view=False, cap=None, seed=0):
    f = lambda flag, s: s if flag else 'no' + s
    name = f'h{h}-N{N}-{kind}-{f(g2, "g2")}-{f(cprev, "c")}-{f(ln, "ln")}-{f(go, "go")}-{f(gcn, "gcn")}-{"view" if view else "dense"}-{"cap%d" % cap if cap else "exact"}'
    return dict(name=name, h=h, N=N, kind=kind, g2=g2, cprev=cprev, ln=ln, go=go, gcn=gcn, view=view, cap=cap,
                seed=seed + 1000 * h + 7 * N + 131 * KINDS.index(kind) + 17 * g2 + 3 * cprev + 5 * ln)


def _cases():
    out = []
    for i, h in enumerate(HIDDEN):
        out.append(_case(h, 1, g2=False, cprev=False, ln=False, go=False, gcn=False))
        out.append(_case(h, 37, g2=True, view=True, cap=107))
        out.append(_case(h, 777))
        out.append(_case(h, 777, g2=True, cprev=i % 2 == 0, ln=i % 2 == 1, go=False, gcn=i % 2 == 1, view=True, cap=1100))
        out.append(_case(h, 777, cprev=i % 2 == 1, ln=i % 2 == 0, gcn=i % 2 == 0, view=i % 2 == 1))
        out.append(_case(h, SWEEP2[h], view=i % 2 == 0))
    for h in (8, 32, 128):
        out.append(_case(h, 96, 'sat', g2=h == 32, view=h == 32))
        out.append(_case(h, 83, 'branch', cap=120 if h == 8 else None))
        out.append(_case(h, 37, 'const', view=h == 128))
    return out


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the fused launches (hidden 8 / 16): rows are the counts of tests/test_gpu_gate_cell_bits.py, the capacity is rows + 70
DGRAD_ROWS_CASES = (1, 127, 129, 300)
FUSED_ROWS_CASES = (1, 63, 65, 129)


def inputs(case):
    """The float32 operands of a case over its valid rows: G, G2, Cprev, wc (3, h), b (4, h), ln (4, h) (None where the case has
    none), the cotangents gO, gHn, gCn, gHn2, and gates (N, 4h): the model's gate activations rounded to float32, the stored
    operands of the backward."""
    rng = np.random.default_rng(case['seed'])
    h, N, kind = case['h'], case['N'], case['kind']
    wc, b = (0.5 * rng.standard_normal((3, h))).astype(F), (0.3 * rng.standard_normal((4, h))).astype(F)
    ln = np.stack([1 + 0.3 * rng.standard_normal(h), 0.3 * rng.standard_normal(h), 1 + 0.3 * rng.standard_normal(h),
                   0.3 * rng.standard_normal(h)]).astype(F)
    sd = 1.4 / np.sqrt(2.0) if case['g2'] else 1.4       # with w_c c + b: pre-activations of N(0, 1.5^2)
    G = (sd * rng.standard_normal((N, 4 * h))).astype(F)
    G2 = (sd * rng.standard_normal((N, 4 * h))).astype(F) if case['g2'] else None
    cp = rng.standard_normal((N, h)).astype(F)
    if kind == 'sat':                                   # the first half of the rows saturates every gate
        G[:N // 2] = rng.choice(np.array([20, -20, 90, -90, 200, -200], F), size=(N // 2, 4 * h))
    elif kind == 'branch':
        b[2] = 0                                        # g_c + 0 is exact: the tanh argument IS the grid value
        grid = branch_grid()
        G[:, 2 * h:3 * h] = grid[(np.arange(N * h) * 7) % grid.size].reshape(N, h)
        wc[:2, :h // 2] = 0                             # I, F of these channels do not read C, so C steers C'raw to the grid too:
        m = forward(G, G2, cp, wc, b, None)             # F c + I T = target
        tgt = grid[(np.arange(N * h) * 11 + 5) % grid.size].reshape(N, h)
        cp[:, :h // 2] = ((tgt - m['I'] * m['T']) / m['F'])[:, :h // 2].astype(F)
    elif kind == 'const':
        G = np.repeat((1.4 * rng.standard_normal((N, 4))).astype(F), h, axis=1)
        cp = np.repeat(rng.standard_normal((N, 1)).astype(F), h, axis=1)
        wc, b, ln = (np.repeat(a[:, :1], h, axis=1) for a in (wc, b, ln))
    Cprev = cp if case['cprev'] else None
    lnp = ln if case['ln'] else None
    m = forward(G, G2, Cprev, wc, b, lnp)
    while kind == 'live' and lnp is not None:           # near-constant rows are not drawn (assert_live): such a row is drawn again
        bad = np.minimum(stats(m['Hr'])[1], stats(m['Cr'])[1])[:, 0] < 2e-3
        if not bad.any():
            break
        G[bad] = (sd * rng.standard_normal((int(bad.sum()), 4 * h))).astype(F)
        m = forward(G, G2, Cprev, wc, b, lnp)
    gates = np.concatenate([m['I'], m['F'], m['T'], m['Og']], axis=1).astype(F)
    gates[np.abs(gates) < TINY] = 0                     # (no subnormal operands: their roundings are absolute, not relative)
    return dict(G=G, G2=G2, Cprev=Cprev, wc=wc, b=b, ln=lnp, gates=gates, gO=draw(rng, N, h) if case['go'] else None,
                gHn=draw(rng, N, h), gCn=draw(rng, N, h) if case['gcn'] else None, gHn2=draw(rng, N, h))


def assert_live(case, x):
    """Live in the sense of tests/test_gpu_cell_oracle.py's _assert_live -- pre-activations of a moderate spread, most sigmoids
    away from 0 and 1 -- and, with a LayerNorm, no row of H'raw / C'raw of variance below 1e-3 (rstd amplifies by < 32)."""
    m = forward(x['G'], x['G2'], x['Cprev'], x['wc'], x['b'], x['ln'])
    pre = np.concatenate([p.reshape(-1) for p in m['pre']])
    sd = pre.std() if pre.size > 1 else np.abs(pre).max()
    assert 0.25 <= sd <= 4.0 or case['N'] == 1, (case['name'], sd)
    sig = np.concatenate([m[k].reshape(-1) for k in ('I', 'F', 'Og')])
    assert ((sig < 0.02) | (sig > 0.98)).mean() < 0.5, case['name']
    if x['ln'] is not None:
        for k in ('Hr', 'Cr'):
            assert stats(m[k])[1].min() >= 1e-3, (case['name'], k, stats(m[k])[1].min())
