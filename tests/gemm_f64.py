"""The dense half of ops.cheb_poly in numpy float64: the product Y = act(drop (.) [T_0 .. T_{K-1} | S] W) (+ res) with its second
product U = [Y | 1 0 0 0] W2, and every adjoint the backward pass launches -- the data gradient, the weight gradient, the
activation backward and the decoder head's backward -- each with the majorant sum |a| |b| of the sums it forms.

The planes need not be Chebyshev planes: `planes` is any (K, N, C) array (C = Ca + Cab when the operand comes in two parts),
S any (N, Ks) block, and the design matrix is A = [planes[0] | .. | planes[K-1] | S] (N, Kred), Kred = K C + Ks.  W's rows follow
that order, its columns the order (output plane j, [Cb | Cbb]).

Layout helpers turn model arrays into what the C ABI of csrc/gemm.hip reads and back (pack_operand / unpack_operand,
slice_major / row_major, unpack_planes).  dispatch() restates qt_dense2's choice of kernel by shape.  The bounds live at the end,
each with the count of float32 roundings it stands for.  numpy only; nothing of qtmpnn.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
ACT_NONE, ACT_RELU, ACT_TANH_RES, ACT_RELU_BWD = 0, 1, 2, 3
WGRAD_ROWS = 512        # node rows per z-block of the weight-gradient launches
MAXQ = 128              # quads of the reduction the kernels' tables hold: Kred <= 512


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------------- model
def design(planes, S=None):
    """A = [planes[0] | .. | planes[K-1] | S] (N, K C + Ks)."""
    planes = f64(planes)
    cols = [planes[k] for k in range(planes.shape[0])]
    if S is not None:
        cols.append(f64(S))
    return np.concatenate(cols, axis=1)


def forward(planes, S, W, Kb=1, Cb=None, Cbb=0, act=ACT_NONE, res=None, drop=None, W2=None):
    """(Y, U, majorants).  Y (Kb, N, Cb + Cbb): output plane j = columns [j (Cb + Cbb), (j + 1) (Cb + Cbb)) of
    act(drop (.) (A W)) (+ res[:, 0] on every column, ACT_TANH_RES only); act applies with Kb == 1.  ACT_RELU_BWD: Y = A W where
    res > 0 (res (N, NB): the forward output whose ReLU gradient this is), else 0.  U (N, 4) = [Y | 1 0 0 0] W2 or None.
    majorants: pre = A W (N, NB), mag = |A| |W|, Kred, and for U magU = [|Y| | 1 0 0 0] |W2|."""
    A, W = design(planes, S), f64(W)
    N, Kred = A.shape
    NB = W.shape[1]
    Cb = NB // Kb - Cbb if Cb is None else Cb
    assert W.shape[0] == Kred and NB == Kb * (Cb + Cbb), (W.shape, Kred, Kb, Cb, Cbb)
    pre, mag = A @ W, np.abs(A) @ np.abs(W)
    d = np.ones(N) if drop is None else f64(drop).reshape(N)
    v = pre
    if act == ACT_RELU:
        v = np.maximum(d[:, None] * pre, 0.0)
    elif act == ACT_TANH_RES:
        v = np.tanh(d[:, None] * pre) + f64(res).reshape(N, -1)[:, :1]
    elif act == ACT_RELU_BWD:
        v = np.where(f64(res)[:, :NB] > 0, pre, 0.0)
    else:
        assert drop is None and res is None
    maj = dict(pre=pre, mag=mag, Kred=Kred, drop=d)
    Um = None
    if W2 is not None:
        W2 = f64(W2)
        one = np.zeros((N, 4))
        one[:, 0] = 1.0
        Um = np.concatenate([v, one], axis=1) @ W2
        maj['magU'] = np.concatenate([np.abs(v), one], axis=1) @ np.abs(W2)
        maj['W2'] = W2
    Y = v.reshape(N, Kb, Cb + Cbb).transpose(1, 0, 2).copy()
    return Y, Um, maj


def dgrad(G, W, K, C):
    """The data gradient of Y = [T_0 .. T_{K-1} | S] W: planes (K, N, C) = G W[:K C]^T, and its majorant |G| |W|^T."""
    G, Wb = f64(G), f64(W)[:K * C]
    N = G.shape[0]
    P, mag = G @ Wb.T, np.abs(G) @ np.abs(Wb).T
    return P.reshape(N, K, C).transpose(1, 0, 2).copy(), mag.reshape(N, K, C).transpose(1, 0, 2).copy()


def wgrad(planes, S, G, rows=None):
    """(A^T G, |A|^T |G|) over the node rows `rows` (a slice or index array; None: all): (Kred, Co)."""
    A, G = design(planes, S), f64(G)
    if rows is not None:
        A, G = A[rows], G[rows]
    return A.T @ G, np.abs(A).T @ np.abs(G)


def wgrad_blocks(planes, S, G, nv, cap):
    """The slabs of qt_wgrad: (ceil(cap / 512), Kred, Co), slab z = A^T G over the valid rows of [512 z, 512 z + 512) -- zeros for
    a block that lies wholly beyond the nv valid rows."""
    nblk = -(-cap // WGRAD_ROWS) if cap > 0 else 0
    return np.stack([wgrad(planes, S, G, slice(min(z * WGRAD_ROWS, nv), min((z + 1) * WGRAD_ROWS, nv)))[0] for z in range(nblk)])


def act_bwd(gY, Y, act, res=None, drop=None, gY2=None):
    """(G, gres, majorant parts) of qt_act_bwd.  g = gY + gY2.  ACT_RELU: G = drop g where Y > 0 else 0.  ACT_TANH_RES:
    t = Y - res[:, 0], G = g (1 - t^2) drop; gres (N, rs): column 0 = g[:, 0], the rest 0."""
    gY, Y = f64(gY), f64(Y)
    N = Y.shape[0]
    g = gY if gY2 is None else gY + f64(gY2)
    mg = np.abs(gY) if gY2 is None else np.abs(gY) + np.abs(f64(gY2))
    d = (np.ones(N) if drop is None else f64(drop).reshape(N))[:, None]
    if act == ACT_RELU:
        return np.where(Y > 0, g * d, 0.0), None, dict(mg=mg, d=d)
    r = f64(res).reshape(N, -1)
    t = Y - r[:, :1]
    gres = np.zeros_like(r)
    gres[:, 0] = g[:, 0]
    return g * (1.0 - t * t) * d, gres, dict(mg=mg, d=d, t=t, two=gY2 is not None)


def head_bwd(gU, W2, Y, W1, K, C):
    """The decoder head's backward: G = relu'(Y) (.) (gU W2[:16]^T) (N, 16), planes (K, N, C) = G W1[:K C]^T, with majorants
    (magG, magP) and |G|."""
    gU, Y, Wb2 = f64(gU), f64(Y), f64(W2)[:Y.shape[1]].T            # Wb2 (4, Co)
    pre, magG = gU @ Wb2, np.abs(gU) @ np.abs(Wb2)
    G = np.where(Y > 0, pre, 0.0)
    P, magP = dgrad(G, W1, K, C)
    return G, P, dict(magG=np.where(Y > 0, magG, 0.0), magP=magP, W1=np.abs(f64(W1)[:K * C]), K=K, C=C)


# ----------------------------------------------------------------------------------------------------------------- layouts
def slice_major(P):
    """(Km, N, C) row-major planes -> the same shape holding (Km, C / 4, N, 4): what qt_cheb_clip_fwd writes, planes_sm reads."""
    Km, N, C = P.shape
    return np.ascontiguousarray(P.reshape(Km, N, C // 4, 4).transpose(0, 2, 1, 3)).reshape(Km, N, C)


def row_major(P):
    """Inverse of slice_major."""
    Km, N, C = P.shape
    return np.ascontiguousarray(P.reshape(Km, C // 4, N, 4).transpose(0, 2, 1, 3)).reshape(Km, N, C)


def pack_operand(planes, Ca, cap=None, lda=(0, 0), off=(4, 8), sm=False, junk=None, dtype=np.float32):
    """What the C ABI reads of an operand (K, N, Ca + Cab): per part i in (a, b) a dict with
         wide  (cap, ld) the matrix plane 0 lives in (ld = lda[i], or the part's width when lda[i] == 0), its other columns `junk`
         off   first column of plane 0 inside `wide` (0 when dense)
         rest  (K - 1, cap, w) planes 1.., slice-major when sm;  None when K == 1
       Rows from N to cap are NaN.  Returns [part a] or [part a, part b]."""
    planes = np.asarray(planes)
    K, N, C = planes.shape
    cap = N if cap is None else cap
    junk = np.float64(3.0) if junk is None else junk
    out, c0 = [], 0
    for i, w in enumerate((Ca, C - Ca)):
        if w == 0:
            continue
        ld = lda[i] if lda[i] else w
        o = off[i] if lda[i] else 0
        assert o + w <= ld and o % 4 == 0 and ld % 4 == 0
        wide = np.full((cap, ld), np.nan, dtype)
        wide[:N] = junk if np.ndim(junk) == 0 else junk[:N, :ld]
        wide[:N, o:o + w] = planes[0, :, c0:c0 + w]
        rest = None
        if K > 1:
            rest = np.full((K - 1, cap, w), np.nan, dtype)
            rest[:, :N] = planes[1:, :, c0:c0 + w]
            if sm:
                rest = slice_major(rest)
        out.append(dict(wide=wide, off=o, rest=rest, w=w))
        c0 += w
    return out


def unpack_operand(parts, N, sm=False):
    """Inverse of pack_operand: (K, N, Ca + Cab)."""
    cols = []
    for p in parts:
        p0 = p['wide'][None, :, p['off']:p['off'] + p['w']]
        rest = p['rest']
        if rest is not None:
            p0 = np.concatenate([p0, row_major(rest) if sm else rest])
        cols.append(p0[:, :N])
    return np.concatenate(cols, axis=2)


def unpack_planes(out, outb=None, sm=False):
    """Output planes as the kernels write them -- out (Kb, cap, Cb), outb (Kb, cap, Cbb) or None, planes 1.. slice-major when sm
    (plane 0 stays row-major) -- as the model's (Kb, cap, Cb + Cbb)."""
    parts = []
    for o in (out, outb):
        if o is None:
            continue
        o = np.asarray(o)
        if sm and o.shape[0] > 1:
            o = np.concatenate([o[:1], row_major(o[1:])])
        parts.append(o)
    return np.concatenate(parts, axis=2)


def split_kred(Kred):
    """(Ka, Ca, Cab, Ks) with Ka (Ca + Cab) + Ks == Kred: the operand shape the tests give a reduction length."""
    table = {4: (1, 4, 0, 0), 20: (1, 16, 0, 4), 32: (2, 4, 8, 8), 36: (2, 16, 0, 4), 60: (3, 4, 16, 0), 64: (3, 4, 16, 4),
             68: (2, 16, 16, 4), 104: (5, 4, 16, 4), 124: (5, 8, 16, 4), 128: (2, 28, 32, 8), 132: (2, 32, 32, 4),
             256: (3, 20, 64, 4), 260: (4, 48, 16, 4), 512: (4, 64, 60, 16)}
    Ka, Ca, Cab, Ks = table[Kred]
    assert Ka * (Ca + Cab) + Ks == Kred
    return table[Kred]


def split_nb(NB):
    """(Kb, Cb, Cbb) with Kb (Cb + Cbb) == NB."""
    table = {4: (1, 4, 0), 8: (2, 4, 0), 12: (3, 4, 0), 16: (1, 16, 0), 20: (1, 4, 16), 60: (3, 4, 16), 64: (1, 64, 0),
             96: (3, 16, 16), 100: (5, 4, 16), 128: (2, 64, 0), 280: (5, 40, 16)}
    Kb, Cb, Cbb = table[NB]
    assert Kb * (Cb + Cbb) == NB
    return table[NB]


def gemm_nt(NB):
    """qt_dense2's tile width of a plain product: the fewest 32-column MFMA tiles over all column blocks, ties to the wider."""
    best, cost = 4, -(-NB // 128) * 4
    for nt in (3, 2):
        c = -(-NB // (32 * nt)) * nt
        if c < cost:
            best, cost = nt, c
    return 2 if NB <= 64 else best


def dispatch(Kred, NB, Kb=1, Cbb=0, act=ACT_NONE, has_W=True):
    """The kernel qt_dense2 launches for a shape (csrc/gemm.hip, default switches)."""
    if NB <= 16 and has_W:
        if NB <= 4:
            return 'k_gemm_skinny<256>'
        if NB == 16 and Kb == 1 and Cbb == 0 and act != ACT_TANH_RES and Kred <= 256:
            return 'k_gemm_row16'
        return 'k_gemm_skinny<64>'
    return f'k_gemm_fwd<{gemm_nt(NB)}>'


# The forward dispatch cases of tests/test_gpu_gemm_f64.py: (Kred, NB, (Kb, Cb, Cbb) or None = split_nb, kernel)
DISPATCH = [
    (4, 4, None, 'k_gemm_skinny<256>'), (20, 4, None, 'k_gemm_skinny<256>'),
    (64, 16, None, 'k_gemm_row16'), (256, 16, None, 'k_gemm_row16'),
    (260, 16, None, 'k_gemm_skinny<64>'), (64, 8, None, 'k_gemm_skinny<64>'), (64, 12, None, 'k_gemm_skinny<64>'),
    (64, 16, (2, 8, 0), 'k_gemm_skinny<64>'), (64, 16, (4, 4, 0), 'k_gemm_skinny<64>'),
    (64, 20, None, 'k_gemm_fwd<2>'), (124, 60, None, 'k_gemm_fwd<2>'), (128, 64, None, 'k_gemm_fwd<2>'), (132, 64, None, 'k_gemm_fwd<2>'),
    (104, 96, None, 'k_gemm_fwd<3>'), (64, 280, None, 'k_gemm_fwd<3>'),
    (60, 128, None, 'k_gemm_fwd<4>'), (68, 100, None, 'k_gemm_fwd<4>'), (512, 128, None, 'k_gemm_fwd<4>'),
]
ROWS = {'k_gemm_skinny<256>': (255, 256, 257), 'k_gemm_row16': (1, 63, 64, 65), 'k_gemm_skinny<64>': (1, 63, 64, 65)}
ROWS_MFMA = (1, 127, 128, 129, 257)
# real-valued shapes: (family, Kred or M, width, N)
REAL_FORWARD = [(64, 16), (260, 16), (64, 64), (104, 64), (104, 96), (68, 100)]        # the plain product (Kred, NB), N = 129: every kernel
# but skinny<256> (the tanh cases).  (512, 128) is exact only: at Kred = 512 a bound of 2 x 512 roundings cannot tell a bf16 operand.
REAL_TANH = [(20, 4, 129), (64, 4, 257)]                       # QT_ACT_TANH_RES: Kb == 1, NB = 4 (skinny<256>) ...
REAL_TANH_WIDE = [(64, 16, 65), (104, 64, 129)]                # ... NB = 16 (skinny<64>: tanh is not on row16) and the MFMA kernel
REAL_HEAD = [((4, 16), 65), ((20, 0), 200)]                    # qt_head_dgrad: (Cb, Cbb), N;  K = 3
REAL_ACT = [(4, 1, 65), (16, 4, 257)]                          # qt_act_bwd tanh: Co, residual stride, N
# qt_wgrad + qt_colsum: M, Co, N.  N = 33 on every tile form (FW 1 / 2 / 4 x CT 1 / 2, Co = 128: a second blockIdx.y tile), several
# passes at FW 2 / 4, and two and three z-blocks at FW = 1, where the longest chain is 128 rows: the shapes at which the bound
# tells a bf16 operand (tests/test_gemm_f64_host.py); (104, 128, 513) would not (547 roundings at their worst against a random walk)
REAL_WGRAD = [(20, 16, 33), (64, 36, 33), (104, 16, 33), (104, 128, 33), (64, 36, 129), (104, 128, 129), (32, 128, 513), (32, 128, 1025)]
WGRAD_M = (20, 32, 36, 64, 68, 104, 512)
WGRAD_CO = (4, 16, 20, 32, 36, 64, 68, 128)
WGRAD_N = (1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1025)


def wgrad_pairs():
    """Every M with Co in {16, 128}, every Co with M in {20, 104}."""
    pairs = [(M, Co) for M in WGRAD_M for Co in (16, 128)] + [(M, Co) for Co in WGRAD_CO for M in (20, 104)]
    return sorted(set(pairs))


# ------------------------------------------------------------------------------------------------------------------ bounds
# House rule (tests/cheb_f64.py): a bound is TWICE a count of float32 roundings on the longest chain an entry's terms pass
# through, times 2^-24, times the majorant; the factor two is the only slack.  An entry whose majorant is 0 must be exact.
def product_bound(mag, Kred, extra=0):
    """A sum of Kred products formed by fused multiply-adds, one rounding each (k_gemm_fwd's v_mfma_f32_32x32x2_f32 is a k-ordered
    chain of them, k_gemm_skinny / k_gemm_row16 / k_head_dgrad are fmaf chains): Kred roundings, + `extra` epilogue operations."""
    return 2.0 * (Kred + extra) * U * np.asarray(mag, np.float64)


def forward_bound(maj, act, Y2d, res=None):
    """|Y - model| (N, NB).  NONE, RELU without drop, RELU_BWD: the product alone (max and select are exact and 1-Lipschitz).
    RELU with drop: one more product.  TANH_RES: the product's error e passes d tanh' <= d; then d * acc rounds once (of
    d |pre|), tanhf is within 2 ulp = 4 roundings of |tanh| (the allowance of test_scalar_cheb3_forward_and_gradients) and the
    add of res rounds once (of |y|)."""
    Kred, mag, d = maj['Kred'], maj['mag'], maj['drop'][:, None]
    if act == ACT_TANH_RES:
        pre = maj['pre']
        return d * product_bound(mag, Kred) + 2.0 * U * (d * np.abs(pre) + 4.0 * np.abs(np.tanh(d * pre)) + np.abs(Y2d))
    if act == ACT_RELU:
        return d * product_bound(mag, Kred, 0 if (d == 1).all() else 1)
    return product_bound(mag, Kred)


def post_bound(maj, ybound):
    """|U - model| (N, 4): a chain of 20 fused multiply-adds over [Y | 1 0 0 0] (five quads), plus Y's own error through |W2|."""
    return product_bound(maj['magU'], 20) + np.asarray(ybound) @ np.abs(maj['W2'][:np.shape(ybound)[1]])


def act_bwd_bound(parts, G):
    """|G - model| of qt_act_bwd, ACT_TANH_RES, from the float32 inputs themselves (no inherited error).  With mg = |gY| + |gY2|:
    t = y - res rounds once (U |t|); t t doubles that and rounds once: 3 roundings of t^2; 1 - t^2 rounds once, the sum gY + gY2
    once (when there is a second gradient), the two products once each: <= 4 roundings of |G|'s majorant mg |1 - t^2| d."""
    t, d, mg = parts['t'], parts['d'], parts['mg']
    return 2.0 * U * d * mg * (3.0 * t * t + 4.0 * np.abs(1.0 - t * t))


def head_bounds(parts):
    """(|G - model|, |planes - model|): G is a chain of 4 fused multiply-adds (the select is exact); a plane entry a chain of 16,
    plus G's error through |Wb1|."""
    eG = product_bound(parts['magG'], 4)
    K, C = parts['K'], parts['C']
    eP = (eG @ parts['W1'].T).reshape(-1, K, C).transpose(1, 0, 2)
    return eG, product_bound(parts['magP'], 16) + eP


def wgrad_fw(M):
    return 1 if M <= 32 else (2 if M <= 64 else 4)


def wgrad_count(N, M, nblk=None, accumulate=False):
    """Roundings on the longest chain of one entry of the summed weight gradient -- the depth of the summation tree, not the
    number of rows -- read off csrc/gemm.hip (an add of an exact +0 rounds nothing):
      wgrad_body   a z-block holds <= 512 rows, walked in passes of 32; the RG = 4 / FW row groups share every pass, row group rg
                   taking its rows [32 rg / RG, 32 (rg + 1) / RG) (mfma_pass: ks = rg KS + k, rows 2 ks + half), and an accumulator
                   takes one v_mfma_f32_32x32x2_f32 term per row of its group, in row order: <= ceil(min(N, 512) / 32) 32 / RG
                   fused multiply-adds (rows past the end load as zeros);  the row groups' partial tiles are added in order:
                   RG - 1 adds;  accumulate: + 1 add into the slab
      k_colsum     a thread's four running sums take every 128th slab each (<= ceil(nblk / 128) adds) and a0 the tail (<= 3 more),
                   together <= ceil(nblk / 32);  (a0 + a1) + (a2 + a3): 2;  the 32 row groups in order, of which only
                   min(nblk, 32) hold a slab: min(nblk, 32)."""
    nblk = -(-N // WGRAD_ROWS) if nblk is None else nblk
    rg = 4 // wgrad_fw(M)
    chain = -(-min(N, WGRAD_ROWS) // 32) * 32 // rg
    return chain + (rg - 1) + int(accumulate) + (-(-nblk // 32) + 2 + min(nblk, 32))


def wgrad_bound(mag, N, M, nblk=None, accumulate=False):
    return 2.0 * wgrad_count(N, M, nblk, accumulate) * U * np.asarray(mag, np.float64)


# -------------------------------------------------------------------------------------------------------------- emulation
def emulate_sum(terms, order=None):
    """float32 sum of terms (T, ...) along axis 0, one rounding per add, in the given order of the T terms."""
    terms = np.asarray(terms, np.float32)
    order = range(terms.shape[0]) if order is None else order
    acc = np.zeros(terms.shape[1:], np.float32)
    for k in order:
        acc = (acc + terms[k]).astype(np.float32)
    return acc


def emulate_product(A, W, order=None):
    """float32 A W: every product rounded to float32, summed by emulate_sum in `order` over the reduction index -- at most two
    roundings per term where a fused multiply-add has one: the emulation is the looser implementation."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    terms = (A.T[:, :, None] * W[:, None, :]).astype(np.float32)           # (Kred, N, NB)
    return emulate_sum(terms, order)


def bf16(a):
    """Round to bfloat16 (nearest even), returned as float32: the reduced-precision operand of the mutation tests."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = ((b >> 16) & 1) + 0x7FFF
    return ((b + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def draw(rng, *shape):
    """sign * (0.5 + U[0, 1)) as float32 (tests/test_gpu_cheb_f64.py's draw)."""
    return (rng.choice([-1.0, 1.0], size=shape) * (0.5 + rng.random(shape))).astype(np.float32)


def ints(rng, *shape):
    """Entries of {-2, -1, 1, 2} as float32: every product and partial sum of the tests' shapes is an integer below 2^24."""
    return rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape).astype(np.float32)
