// Attention coefficients of the TransformerConv edge softmax (attn.hip), written out: what PyG returns for
// return_attention_weights=True.  Forward only, before dropout, no autograd.
//
//   alpha_ij = exp(s_ij - max_j s_ij) / (sum_j exp(s_ij - max_j s_ij) + 1e-16),   s_ij = q_i . (k_j + e_ij) / sqrt(c_real)
//
// Operands are those of qt_attn_fwd for G groups on one mesh (a convolution, a head, or a convolution x head): group g reads
// proj + g hs with q / k blocks ps apart and rows ld apart, and We[g] (C, 2).  The per-node softmax runs in two passes over the
// node's edges -- running max and sum, then the coefficients -- so nothing of the forward (its stats) is needed.  One node per
// group of C/4 lanes (float4 each), as k_attn_fwd; only q_i and the k_j rows are read (no v, no skip).
// Outputs: alpha_e (G, E): the coefficient of the message col[e] -> row(e), stored at rev[e] (the transposed entry), so that
// alpha_e follows the CSR order of the pairs (src = row, dst = col); alpha_s (G, Ncap): the coefficient of node i's self pair,
// 0 where the node has none.  Rows beyond n_dev are not touched.  No atomics, no random numbers.
#include "qt_attn.h"

namespace {
using namespace qtattn;

constexpr int AW_BS = 64;       // one wave per workgroup, as k_attn_fwd
constexpr int LPN_MAX = 8;      // C = 4 .. 32

struct WArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const float* eattr;     // (E, 2) [angle, dist] of the message col[e] -> row(e)
    const float* selfloop;  // (N) > 0 where the node carries a self pair, or NULL
    const float* proj;      // q block of group 0; k block at + ps; group g at + g hs
    const float* We;        // (G, C, 2)
    const int32_t* rev;     // (E) position of the transposed entry
    const int32_t* n_dev;
    float* alpha_e;         // (G, E)
    float* alpha_s;         // (G, Ncap)
    int64_t ps, hs;
    int ld, C, Ncap, E;
    float scale;
};

// The scores of EPT consecutive edges eb .. eb + EPT - 1 of node i (the self pair after the stored edges); jj[u] < 0 past the end.
// Its own trip, not qt_attn.h's Trip: through that one the compiler fuses another product of w0 angle + w1 dist (other bits).
template <int LPN>
__device__ __forceinline__ void scores(const WArgs& a, const float* __restrict__ kb, const F4& q, const F4& w0, const F4& w1, int i,
                                       uint32_t j0, int eb, int e1, int eend, int* jj, float* s) {
    F4 kk[EPT];
    float2 ea[EPT];
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        const int e = eb + u;
        jj[u] = e < e1 ? a.col[e] : (e < eend ? i : -1);
    }
#pragma unroll
    for (int u = 0; u < EPT; ++u)
        if (jj[u] >= 0) {
            kk[u] = ld4(kb + ((uint32_t)jj[u] * (uint32_t)a.ld + j0));
            ea[u] = eb + u < e1 ? *reinterpret_cast<const float2*>(a.eattr + 2 * (uint32_t)(eb + u)) : make_float2(0.0f, 0.0f);
        }
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        if (jj[u] < 0) break;                      // (uniform over the node's lane group)
        F4 kj = kk[u];
#pragma unroll
        for (int c = 0; c < 4; ++c) kj.v[c] += w0.v[c] * ea[u].x + w1.v[c] * ea[u].y;
        s[u] = group_sum<LPN>(dot4(q, kj)) * a.scale;
    }
}

template <int LPN>
__global__ __launch_bounds__(AW_BS) void k_attn_weights(WArgs a) {
    const int hd = blockIdx.y;
    const float* __restrict__ qb = a.proj + hd * a.hs;
    const float* __restrict__ kb = qb + a.ps;
    const float* __restrict__ We = a.We + (int64_t)hd * 2 * a.C;
    float* __restrict__ alpha_e = a.alpha_e + (int64_t)hd * a.E;
    float* __restrict__ alpha_s = a.alpha_s + (int64_t)hd * a.Ncap;
    const int rows = qt_rows(a.n_dev, a.Ncap);
    const int blk = xcd_block(rows, AW_BS / LPN);
    if (blk < 0) return;
    const int i = blk * (AW_BS / LPN) + (int)threadIdx.x / LPN;
    if (i >= rows) return;
    const uint32_t j0 = ((uint32_t)threadIdx.x % LPN) * 4;
    const F4 q = ld4(qb + ((uint32_t)i * (uint32_t)a.ld + j0));
    F4 w0, w1;
    we_columns(We, j0, &w0, &w1);
    const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const int extra = (a.selfloop && a.selfloop[i] > 0.0f) ? 1 : 0;
    const int eend = e1 + extra;
    // pass 1: running max and sum (the forward's m, l)
    float m = -INFINITY, l = 0.0f;
    for (int eb = e0; eb < eend; eb += EPT) {
        int jj[EPT];
        float s[EPT];
        scores<LPN>(a, kb, q, w0, w1, i, j0, eb, e1, eend, jj, s);
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            if (jj[u] < 0) break;
            const float mn = fmaxf(m, s[u]);
            l = l * __expf(m - mn) + __expf(s[u] - mn);
            m = mn;
        }
    }
    // pass 2: the coefficients, one lane of the group writes
    const float inv = 1.0f / (l + 1e-16f);
    for (int eb = e0; eb < eend; eb += EPT) {
        int jj[EPT];
        float s[EPT];
        scores<LPN>(a, kb, q, w0, w1, i, j0, eb, e1, eend, jj, s);
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            if (jj[u] < 0) break;
            if (j0 == 0) {
                const float al = __expf(s[u] - m) * inv;
                if (eb + u < e1)
                    alpha_e[a.rev[eb + u]] = al;
                else
                    alpha_s[i] = al;
            }
        }
    }
    if (j0 == 0 && !extra) alpha_s[i] = 0.0f;
}

}  // namespace

extern "C" int qt_attn_weights(const int32_t* rowptr, const int32_t* col, const float* eattr, const float* selfloop, const float* proj,
                               int ld, int64_t ps, int64_t hs, const float* We, int C, int c_real, int G, int N, const int32_t* n_dev,
                               const int32_t* rev, int E, float* alpha_e, float* alpha_s, void* stream) {
    QT_ARG(rowptr && col && eattr && proj && We && rev && alpha_e && alpha_s, "null pointer");
    QT_ARG(c_ok(C, LPN_MAX) && c_real >= 1 && c_real <= C, "bad channel count (the kernels are built for C = 4, 8, 16, 32)");
    QT_ARG(G >= 1 && G <= 64, "bad group count (1 .. 64)");
    if (ps == 0) ps = C;
    if (hs == 0) hs = 4 * C;
    QT_ARG(ld >= C && ld % 4 == 0 && ps % 4 == 0 && hs % 4 == 0 && ((uintptr_t)proj & 15) == 0,
           "bad row / block / group stride or misaligned proj (multiples of 4 floats)");
    QT_ARG(N >= 0 && E >= 0 && (int64_t)N * ld < (1ll << 31), "a group's rows must span fewer than 2^31 floats");
    if (N <= 0) return QT_OK;
    WArgs a;
    a.rowptr = rowptr; a.col = col; a.eattr = eattr; a.selfloop = selfloop; a.proj = proj; a.We = We; a.rev = rev; a.n_dev = n_dev;
    a.alpha_e = alpha_e; a.alpha_s = alpha_s; a.ps = ps; a.hs = hs; a.ld = ld; a.C = C; a.Ncap = N; a.E = E;
    a.scale = 1.0f / sqrtf((float)c_real);
    const int grid = (qt_cdiv((int64_t)N * (C / 4), AW_BS) + 7) & ~7;      // whole rounds over the 8 XCDs (xcd_block)
    QT_ATTN_LAUNCH(C, LPN_MAX, k_attn_weights, dim3(grid, G), AW_BS, stream, a);
    QT_LAUNCHED();
    return QT_OK;
}
