// Multi-head attention convolution of the reference's MHTransformerConv (model/model.py:26-37): PyG TransformerConv with
// heads = H, concat = True, beta = False, edge_dim = 2, root_weight = True, followed by the head merge lin: (H C -> C).
//
//   cat_i = concat_g( sum_{j -> i} d_ij^g alpha_ij^g (v_j^g + e_ij^g) ) + skip_i,   alpha^g = softmax_j(q_i^g . (k_j^g + e_ij^g) / sqrt(C))
//   y_i   = Wlin cat_i + blin
//
// Operands are those of the G-head launch of attn.hip with G = H: proj rows (N, H 4C) = [q | k | v | skip] per head, head-major;
// We (H, C, 2).  Forward: ONE launch for the attention of all heads and the merge.  The H heads of a node share its edge loop: the
// node's lanes are 4 groups of C/4 (one per head, the last idle when H = 3), they walk the node's edges together (col / eattr are
// the same addresses for all groups: one request per wave instruction) and keep one online softmax per group.  The merge runs in
// the epilogue: every head group multiplies its own C columns of cat with its C rows of Wlin^T (staged in LDS), and the partial
// rows of the four groups are summed with two xor shuffles.
// Backward: k_mh_merge_bwd gives gcat = g Wlin (per row) and per-block partials of dWlin / dblin (summed by qt_colsum: fixed
// order, no atomics); the attention gradient is then qt_attn_bwd with G = H on gcat, with the cat plane as its `out`.
// The per-head body is qt_attn.h's node_forward, the one k_attn_fwd runs, with head_seed per head: the fused launch draws exactly
// the mask of qt_attn_fwd with G = H for the same seed / seed_dev (tests/test_gpu_mh.py compares the two with dropout on).
#include "qt_attn.h"

namespace {
using namespace qtattn;

constexpr int MH_BS = 256;
constexpr int MH_MAX_HEADS = 4;
constexpr int LPN_MAX = 8;      // C = 4 .. 32: four head groups of a node fit a wave, Wlin^T fits LDS

struct MhArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const float* eattr;     // (E, 2) [angle, dist] of the message col[e] -> row(e)
    const float* selfloop;  // (N) > 0 where the node carries a self pair, or NULL
    const float* proj;      // (N, H 4C)
    const float* We;        // (H, C, 2)
    const float* Wt;        // (H C, C): Wlin^T, zero rows / columns above c_real
    const float* blin;      // (C)
    int heads, Ncap;
    const int32_t* n_dev;
    float scale, keep;
    uint32_t seed;
    const uint32_t* seed_dev;
    float* y;               // (N, C)
    float* stats;           // (H, N, 2)
    float* cat;             // (N, H C) or NULL
};

template <int LPN>
__global__ __launch_bounds__(MH_BS) void k_mh_fwd(MhArgs a) {
    constexpr int C = 4 * LPN, TPN = 4 * LPN, NPB = MH_BS / TPN;
    __shared__ float4 sW[MH_MAX_HEADS * C * LPN];          // Wlin^T: row k (= head g, channel c) is LPN float4s
    const int H = a.heads, HC = H * C;
    for (int t = threadIdx.x; t < HC * LPN; t += MH_BS) sW[t] = reinterpret_cast<const float4*>(a.Wt)[t];
    __syncthreads();
    const int rows = qt_rows(a.n_dev, a.Ncap);
    const int blk = xcd_block(rows, NPB);
    if (blk < 0) return;
    const int i = blk * NPB + (int)threadIdx.x / TPN;
    if (i >= rows) return;                                  // (the node's whole lane group)
    const int slot = (int)threadIdx.x % TPN, hd = slot / LPN, l = slot % LPN;
    const uint32_t j0 = (uint32_t)l * 4, ld = 4u * C * H;
    const bool live = hd < H;
    F4 o = {{0, 0, 0, 0}};
    if (live) {
        const float* __restrict__ qb = a.proj + hd * 4 * C;      // k_attn_fwd's node at ld = 4CH, ps = C, hs = 4C
        const NodeOut r = node_forward<LPN>(a.rowptr, a.col, a.eattr, a.selfloop, qb, qb + C, qb + 2 * C, qb + 3 * C, ld,
                                            a.We + hd * 2 * C, i, j0, a.scale, a.keep, head_seed(a.seed, a.seed_dev, hd));
        o = r.o;
        if (a.cat) st4(a.cat + ((uint32_t)i * (uint32_t)HC + hd * C + j0), o);
        put_stats(a.stats + (int64_t)hd * 2 * a.Ncap, i, j0, r);
    }
    // head merge: this group's partial of y_i[j0 .. j0 + 3] = sum_c cat_i[hd C + c] Wt[hd C + c][j0 .. j0 + 3]
    F4 p = {{0, 0, 0, 0}};
    if (live) {
        const int src = ((int)threadIdx.x & 63) - l;        // lane of channel block 0 of this head group
#pragma unroll
        for (int c4 = 0; c4 < LPN; ++c4)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = __shfl(o.v[e], src + c4, 64);
                const float4 w = sW[(hd * C + 4 * c4 + e) * LPN + l];
                p.v[0] += v * w.x;
                p.v[1] += v * w.y;
                p.v[2] += v * w.z;
                p.v[3] += v * w.w;
            }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        p.v[c] += __shfl_xor(p.v[c], LPN, 64);              // heads (0 + 1), (2 + 3) ...
        p.v[c] += __shfl_xor(p.v[c], 2 * LPN, 64);          // ... then their sum
    }
    if (hd == 0) {
        const F4 b = ld4(a.blin + j0);
#pragma unroll
        for (int c = 0; c < 4; ++c) p.v[c] += b.v[c];
        st4(a.y + ((uint32_t)i * C + j0), p);
    }
}

// Backward of the merge, NB rows per trip: gcat_i = Wlin^T-transposed g_i (gcat[k] = sum_o Wt[k][o] g_i[o]) for every row, and
// this block's partial sums of dWt[k][o] = sum_i cat_i[k] g_i[o] and dblin[o] = sum_i g_i[o] (part row blockIdx.x).
constexpr int MB_NB = 32;
template <int LPN>
__global__ __launch_bounds__(MH_BS) void k_mh_merge_bwd(const float* __restrict__ g, int ld_g, const float* __restrict__ Wt,
                                                       const float* __restrict__ cat, int heads, int Ncap, const int32_t* __restrict__ n_dev,
                                                       float* __restrict__ gcat, float* __restrict__ part, int accumulate) {
    constexpr int C = 4 * LPN, CP = C + 1, R = (MH_MAX_HEADS * C * C + C + MH_BS - 1) / MH_BS;
    __shared__ float sW[MH_MAX_HEADS * C * CP];             // rows padded by one: consecutive rows fall in different banks
    __shared__ float sg[MB_NB * C];
    __shared__ float sc[MB_NB * MH_MAX_HEADS * C];
    const int HC = heads * C, nw = HC * C, nent = nw + C;
    for (int t = threadIdx.x; t < nw; t += MH_BS) sW[(t / C) * CP + t % C] = Wt[t];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    const int rows = qt_rows(n_dev, Ncap);
    for (int n0 = blockIdx.x * MB_NB; n0 < rows; n0 += gridDim.x * MB_NB) {
        __syncthreads();
        for (int t = threadIdx.x; t < MB_NB * C; t += MH_BS) {
            const int node = n0 + t / C;
            sg[t] = node < rows ? g[(int64_t)node * ld_g + t % C] : 0.0f;
        }
        for (int t = threadIdx.x; t < MB_NB * HC; t += MH_BS) {
            const int node = n0 + t / HC;
            sc[t] = node < rows ? cat[(int64_t)node * HC + t % HC] : 0.0f;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < MB_NB * HC; t += MH_BS) {
            const int r = t / HC, k = t % HC;
            if (n0 + r >= rows) break;
            float s = 0.0f;
#pragma unroll
            for (int o = 0; o < C; ++o) s += sW[k * CP + o] * sg[r * C + o];
            gcat[(int64_t)(n0 + r) * HC + k] = s;
        }
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int e = (int)threadIdx.x + rr * MH_BS;
            if (e < nw) {
                const int k = e / C, o = e % C;
                float s = acc[rr];
                for (int r = 0; r < MB_NB; ++r) s += sc[r * HC + k] * sg[r * C + o];
                acc[rr] = s;
            } else if (e < nent) {
                const int o = e - nw;
                float s = acc[rr];
                for (int r = 0; r < MB_NB; ++r) s += sg[r * C + o];
                acc[rr] = s;
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int e = (int)threadIdx.x + rr * MH_BS;
        if (e < nent) {
            float* pp = part + (int64_t)blockIdx.x * nent + e;
            *pp = (accumulate & 1) ? *pp + acc[rr] : acc[rr];
        }
    }
}

}  // namespace

extern "C" int qt_mhattn_blocks(int N, int C, int heads) {
    if (N <= 0 || !c_ok(C, LPN_MAX) || heads < 1 || heads > MH_MAX_HEADS) return 0;
    const int need = qt_cdiv(N, MB_NB);
    return need < 256 ? need : 256;
}

extern "C" int qt_mhattn_fwd(const int32_t* rowptr, const int32_t* col, const float* eattr, const float* selfloop, const float* proj,
                             const float* We, const float* Wt, const float* blin, int C, int c_real, int heads, int N,
                             const int32_t* n_dev, float keep, uint32_t seed, const uint32_t* seed_dev, float* y, float* stats,
                             float* cat, void* stream) {
    QT_ARG(rowptr && col && eattr && proj && We && Wt && blin && y && stats, "null pointer");
    QT_ARG(c_ok(C, LPN_MAX) && c_real >= 1 && c_real <= C, "bad channel count (C = 4, 8, 16 or 32, 1 <= c_real <= C)");
    QT_ARG(heads >= 1 && heads <= MH_MAX_HEADS, "bad head count (1 .. 4)");
    QT_ARG(N >= 0 && (int64_t)N * 4 * C * heads < (1ll << 31), "the proj rows must span fewer than 2^31 floats");
    QT_ARG((((uintptr_t)proj | (uintptr_t)Wt | (uintptr_t)blin | (uintptr_t)y | (uintptr_t)cat) & 15) == 0, "operands must be 16-byte aligned");
    if (N == 0) return QT_OK;
    MhArgs a;
    a.rowptr = rowptr; a.col = col; a.eattr = eattr; a.selfloop = selfloop; a.proj = proj; a.We = We; a.Wt = Wt; a.blin = blin;
    a.heads = heads; a.Ncap = N; a.n_dev = n_dev; a.scale = 1.0f / sqrtf((float)c_real); a.keep = keep; a.seed = seed;
    a.seed_dev = seed_dev; a.y = y; a.stats = stats; a.cat = cat;
    const int npb = MH_BS / C;                                                  // 4 head groups of C / 4 lanes per node
    const int grid = (qt_cdiv(N, npb) + 7) & ~7;                                // whole rounds over the 8 XCDs (xcd_block)
    QT_ATTN_LAUNCH(C, LPN_MAX, k_mh_fwd, grid, MH_BS, stream, a);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_mhattn_bwd_merge(const float* g, int ld_g, const float* Wt, const float* cat, int C, int heads, int N,
                                   const int32_t* n_dev, float* gcat, float* part, int accumulate, void* stream) {
    QT_ARG(g && Wt && cat && gcat && part, "null pointer");
    QT_ARG(c_ok(C, LPN_MAX) && heads >= 1 && heads <= MH_MAX_HEADS, "bad channel / head count");
    QT_ARG(ld_g >= C && N >= 0 && (int64_t)N * heads * C < (1ll << 31) && (int64_t)N * ld_g < (1ll << 31), "bad row stride / size");
    if (N == 0) return QT_OK;
    const int grid = qt_mhattn_blocks(N, C, heads);
    QT_ATTN_LAUNCH(C, LPN_MAX, k_mh_merge_bwd, grid, MH_BS, stream, g, ld_g, Wt, cat, heads, N, n_dev, gcat, part, accumulate);
    QT_LAUNCHED();
    return QT_OK;
}
