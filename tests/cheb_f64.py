"""The mesh Laplacian and the Chebyshev recurrences of ChebConv, in numpy float64, from a label map alone.

Input: `labels` (B, n, m) integers, the clip-global node row of every pixel, < 0 where a pixel has no node, and `resolution`.
No cell record, level, CSR array or tile enters: a node IS the set of pixels that carry its label.

  node       centroid = mean (column, row) of its pixels, times `resolution`
  adjacency  ordered pairs (i, j), i != j, of labels >= 0 on 4-adjacent pixels of the SAME clip
  w_ij       Euclidean distance of the two centroids
  deg_i      sum_j w_ij;   dis_i = deg_i^-1/2, 0 where deg_i = 0
  L^_ij      -dis_i w_ij dis_j          (PyG ChebConv, normalization='sym', lambda_max = 2: L^ = -D^-1/2 W D^-1/2)

A pixelwise mesh (every unmasked pixel a node) needs no case of its own: qtmpnn.mesh.build_pixel_mesh documents that its CSR
carries "the uniform pixel distance" where the reference passes unit weights, "which gives the same L^ because the symmetric
normalisation is scale invariant" -- and the centroid distance of two 4-adjacent one-pixel nodes is exactly `resolution`.

Every operation returns (value, majorant): the majorant has the value's shape and is the same recurrence on absolute values,
A_0 = |Z|, A_1 = |L^| A_0, A_k = 2 |L^| A_{k-1} + A_{k-2}; for axpby |alpha| |L^| |x| + |beta| |p| + |gamma| |q|.  The GPU tests
bound |kernel - value| by a multiple of 2^-24 times it.  Vectorised numpy (np.add.at / np.bincount); nothing of qtmpnn, no scipy.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


class Lap:
    """L^ as a sorted edge list: row, col (E,) int64 in (row, col) order, w, val = L^_ij (E,), deg, dis (N,), xy (N, 2) centroids
    (column, row) * resolution, rowlen (N,) edges per row."""

    def __init__(self, N, row, col, w, xy):
        order = np.lexsort((col, row))
        self.N, self.row, self.col, self.w, self.xy = int(N), row[order], col[order], np.asarray(w, np.float64)[order], xy
        self.deg = np.bincount(self.row, weights=self.w, minlength=N)[:N]
        with np.errstate(divide='ignore'):
            self.dis = np.where(self.deg > 0, self.deg ** -0.5, 0.0)
        self.val = -(self.dis[self.row] * self.w * self.dis[self.col])
        self.rowlen = np.bincount(self.row, minlength=N)[:N]

    @property
    def E(self):
        return self.row.shape[0]

    def with_val(self, val):
        """A copy with other entries (same pattern): the tests' perturbed operators."""
        other = Lap.__new__(Lap)
        other.__dict__.update(self.__dict__)
        other.val = np.asarray(val, np.float64)
        return other

    def neighbours(self):
        """{(i, j)}: the adjacency as a set of ordered pairs."""
        return set(zip(self.row.tolist(), self.col.tolist()))


def centroids(labels, N, resolution=0.25):
    """(N, 2) mean (column, row) of every node's pixels, times resolution (0 for a label nobody carries)."""
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 3, 'labels: (B, n, m)'
    _, rr, cc = np.meshgrid(np.arange(lab.shape[0]), np.arange(lab.shape[1]), np.arange(lab.shape[2]), indexing='ij')
    ok = lab >= 0
    cnt = np.bincount(lab[ok], minlength=N).astype(np.float64)[:N]
    sx = np.bincount(lab[ok], weights=cc[ok].astype(np.float64), minlength=N)[:N]
    sy = np.bincount(lab[ok], weights=rr[ok].astype(np.float64), minlength=N)[:N]
    return np.stack([sx, sy], axis=1) / np.maximum(cnt, 1.0)[:, None] * resolution


def pairs(labels, N):
    """Ordered pairs (row, col) of distinct labels >= 0 on 4-adjacent pixels of the same clip, each once."""
    lab = np.asarray(labels).astype(np.int64)
    keys = []
    for a, b in ((lab[:, :-1, :], lab[:, 1:, :]), (lab[:, :, :-1], lab[:, :, 1:])):
        a, b = a.reshape(-1), b.reshape(-1)
        ok = (a >= 0) & (b >= 0) & (a != b)
        keys += [a[ok] * N + b[ok], b[ok] * N + a[ok]]
    key = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    return key // max(N, 1), key % max(N, 1)


def laplacian(labels, resolution=0.25, N=None, xy=None):
    """The model's L^ of a label map (xy: other centroids than the pixel means -- the tests' wrong-centroid operator)."""
    lab = np.asarray(labels).astype(np.int64)
    if N is None:
        N = int(lab.max()) + 1 if lab.size and lab.max() >= 0 else 0
    row, col = pairs(lab, N)
    if xy is None:
        xy = centroids(lab, N, resolution)
    d = xy[row] - xy[col]
    return Lap(N, row, col, np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2), xy)


def _2d(x):
    x = np.asarray(x, np.float64)
    return x[:, None] if x.ndim == 1 else x


def apply(L, x, transpose=False):
    """(L^ x, |L^| |x|) for x (N, C) or (N,); transpose: L^T x (the same in exact arithmetic only when `val` is symmetric)."""
    x2 = _2d(x)
    src, dst = (L.row, L.col) if transpose else (L.col, L.row)
    out, mag = np.zeros_like(x2), np.zeros_like(x2)
    np.add.at(out, dst, L.val[:, None] * x2[src])
    np.add.at(mag, dst, np.abs(L.val)[:, None] * np.abs(x2[src]))
    shape = np.shape(x)
    return out.reshape(shape), mag.reshape(shape)


def planes(L, Z, K, transpose=False):
    """(T, A), each (K, N, C): T_0 = Z, T_1 = L^ Z, T_k = 2 L^ T_{k-1} - T_{k-2}, and the majorants A_k."""
    Z = np.asarray(Z, np.float64)
    T, A = [Z], [np.abs(Z)]
    for k in range(1, K):
        t, _ = apply(L, T[-1], transpose)
        _, a = apply(L, A[-1], transpose)
        if k == 1:
            T.append(t)
            A.append(a)
        else:
            T.append(2.0 * t - T[-2])
            A.append(2.0 * a + A[-2])
    return np.stack(T), np.stack(A)


def axpby(L, x, alpha, p=None, beta=0.0, q=None, gamma=0.0):
    """(alpha L^ x + beta p + gamma q, |alpha| |L^| |x| + |beta| |p| + |gamma| |q|); p / q may be None."""
    v, a = apply(L, x)
    v, a = alpha * v, abs(alpha) * a
    for s, t in ((beta, p), (gamma, q)):
        if t is not None:
            t = np.asarray(t, np.float64)
            v, a = v + s * t, a + abs(s) * np.abs(t)
    return v, a


def clenshaw(L, G, K):
    """The adjoint of planes: (sum_k T_k(L^)^T G_k, sum_k A_k(|L^|^T, |G_k|)) for G (K, N, C) -- computed as that sum, one
    transposed recurrence per plane, not by the Clenshaw recurrence the kernels run."""
    G = np.asarray(G, np.float64)
    assert G.shape[0] == K
    out, mag = np.zeros_like(G[0]), np.zeros_like(G[0])
    for k in range(K):
        T, A = planes(L, G[k], k + 1, transpose=True)
        out += T[k]
        mag += A[k]
    return out, mag


def ones(L, ks):
    """([1, L^ 1, T_2(L^) 1, ...] (N, ks), its majorant)."""
    T, A = planes(L, np.ones(L.N), ks)
    return T.T.copy(), A.T.copy()


# ------------------------------------------------------------------------------------------------------------------ bounds
# What a float32 implementation may differ from the model by.  Each bound is TWICE a count of float32 roundings (each <= U
# relative: products, sums, sqrtf and the division are correctly rounded) times the majorant; the factor two is the only slack.
def w_bound(L):
    """|w - model| per edge.  Centroids ((float)col + 0.5 (extent - 1)) * 0.25 and their differences are exact for resolution 0.25.
    s = dx^2 + dy^2: each square rounds once, but on its own positive term, so both together move s by <= 1 U; the add 1 U;
    the square root halves those 2 U to 1 U and rounds once itself: 2 roundings.  Bound 4 U w."""
    return 4.0 * U * L.w


def dis_bound(L):
    """|dis - model| per row of d edges.  deg = sum of d positive w (2 U each, above) by d - 1 adds: (d + 1) U relative; the
    power -1/2 halves it; sqrtf and the division round once each: (d + 1) / 2 + 2 roundings.  Bound (d + 5) U dis."""
    return (L.rowlen + 5.0) * U * L.dis


def nrm_bound(L):
    """|nrm - model| per edge (i, j).  dis_i ((d_i + 5) / 2 roundings), w (2), dis_j ((d_j + 5) / 2), two products (2):
    (d_i + d_j) / 2 + 9.  Bound (d_i + d_j + 18) U |L^_ij|."""
    return (L.rowlen[L.row] + L.rowlen[L.col] + 18.0) * U * np.abs(L.val)


def hop_factor(L):
    """The per-hop factor of the recurrence bounds: d_max + 24, d_max the longest row of the mesh.
    One hop computes y_i = alpha sum_j n_ij x_j + beta p_i + gamma q_i.  Worst-case count for one entry: n_ij carries
    (d_i + d_j) / 2 + 9 roundings (nrm_bound), the row's chain of fused multiply-adds d_i, the epilogue 3 (alpha acc, then one
    fused multiply-add per addend): <= 2 d_max + 12, all relative to sum_j |n_ij| |x_j| + |beta p_i| + |gamma q_i|, which the
    majorant holds.  Twice that, 4 d_max + 24, assumes that every rounding of the longest row and of both degree sums
    is at its worst and of one sign; the tests hold the kernels to the stricter d_max + 24 (one row sum over terms the majorant
    already bounds, plus 24 for the entries of L^ and the epilogue)."""
    return float(L.rowlen.max()) + 24.0 if L.N else 24.0


def plane_bound(L, k, A):
    """|T_k - model| <= k (d_max + 24) U A_k.  With e_k the error of plane k and c = d_max + 24: the hop's own roundings are
    <= c U (2 |L^| |T_{k-1}| + |T_{k-2}|) <= c U A_k, the errors it inherits obey the recurrence, |e_k| <= 2 |L^| |e_{k-1}| +
    |e_{k-2}| + c U A_k, and |e_j| <= j c U A_j for j < k gives |e_k| <= c U ((k - 1) (2 |L^| A_{k-1} + A_{k-2}) + A_k) = k c U A_k.
    The same form serves axpby (k = 1) and, with the adjoint's majorant and k = K - 1 hops, the Clenshaw backward."""
    return k * hop_factor(L) * U * np.asarray(A, np.float64)
