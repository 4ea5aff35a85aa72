// Edge-softmax attention of TransformerConv(heads=1, concat=False, beta=False, edge_dim=2, root_weight=True), the
// convolution the reference's sea-ice scripts hard-code (model/model.py:51, ice_exp.py:48; PyG 2.2.0, restated in
// oracle/qt_oracle.py:transformer_conv).  SURVEY.md 8(f) row 1.
//
//   out_i = sum_{j -> i} d_ij alpha_ij (v_j + e_ij) + skip_i,   alpha_i. = softmax_j( q_i . (k_j + e_ij) / sqrt(C) )
//   e_ij  = We [angle(j -> i), dist(j, i)]          (lin_edge has no bias)
//
// q | k | v | skip are the four column blocks of ONE projection GEMM (proj, row stride ld).  Incoming edges of i are
// row i of the mesh CSR (the quadtree adjacency is symmetric) plus the self pair (i, i) that get_adj emits for
// multi-pixel cells (attrs (0, 0)); edge attributes come from the node centroids, once per mesh (qt_attn_edge_attrs).
// One node per group of C/4 lanes (float4 each), online softmax, dot products reduced with xor shuffles: the lane-group
// primitives, the dropout rule, the trip over a node's pairs and the forward's node body are qt_attn.h's, shared with mhattn.hip
// and attnw.hip.  Here: the operand views of a G-head launch, the forward kernel around node_forward, and the backward in gather
// form, no atomics: pass A per target (dq_i + the messages' coefficients), pass B per source (dk_j, dv_j, dWe partials).
#include "qt_attn.h"

namespace {
using namespace qtattn;

struct AttnArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const float* eattr;     // (E, 2) [angle, dist] of the message col[e] -> row(e) (qt_attn_edge_attrs)
    const float* selfloop;  // (N) > 0 where the node carries a self pair, or NULL
    const float* proj;      // (N, ld): q | k | v | skip, C columns each
    const float* We;        // (C, 2)
    int ld, C, Ncap;
    const int32_t* n_dev;
    float scale;            // 1 / sqrt(real channel count)
    float keep;             // 1 - dropout p (1 = no dropout)
    const int32_t* rev;     // (E) position of the transposed entry (row col[e], column row(e)), with coef: see k_attn_bwd_source
    float* coef;            // (E + N, 2) backward scratch: (ds, alpha d) of the message whose transposed entry is stored at the slot, then of the self pairs
    int E;
    int ld_g;               // backward: row stride of g (a column block of a wider gradient is read in place)
    int accumulate;         // backward: add the We partials into `part` (several uses of one convolution share the slab)
    uint32_t seed;
    const uint32_t* seed_dev;   // optional step counter on the device, mixed into the seed (head_seed)
    // G convolutions on the same mesh in one launch (blockIdx.y = head): head g reads the column block [g 4C, (g+1) 4C) of the
    // proj rows (ld >= G 4C), We[g], writes the column block g C of the out rows (ld_o) and its own stats / coef / part
    // slabs.  gmod: head g reads the column block (g % gmod) C of the incoming gradient (a sum of head groups downstream).
    int ld_o, gmod;
    // strides in floats: ps between the q / k / v / skip blocks of a proj (and gproj) row, hs between heads of proj, hs_o of out,
    // hs_g of g.  Rows side by side (one (N, G 4C) matrix): ld = G 4C, ps = C, hs = 4C; one dense (N, C) plane per block and head:
    // ld = C, ps = N C, hs = 4 N C -- gathered k / v rows are then whole 128-byte lines of a contiguous array.
    int64_t ps, hs, hs_o, hs_g;
};

// Per-head views of the operands (a single convolution is head 0 of 1); returns the head of this workgroup.
// Last in, first out over the heads: an 8-head operand is 510 MB, the memory-side cache 256 MB, so a launch should start with
// the heads its predecessor touched last.  The grouped projection writes heads 0..7 -> the forward pass walks 7..0; in the
// backward the target pass walks 7..0, the source pass 0..7 (it re-reads the q planes the target pass just read), and the data
// gradient after it takes its groups 7..0 (qt_proj_group, reverse).  cfg4t: 47.1 ms per step with every launch ascending,
// 46.6 with the three passes descending, 46.2 with this order.
static constexpr int QT_ATTN_DESC = 3;      // bit 0 / 1 / 2: the forward / target / source pass walks the heads from the last to the first
template <int PASS>
__device__ __forceinline__ int head_setup(AttnArgs& a) {
    const int hd = (QT_ATTN_DESC >> PASS) & 1 ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
    if (hd) {
        a.proj += hd * a.hs;
        a.We += (int64_t)hd * 2 * a.C;
        if (a.coef) a.coef += (int64_t)hd * 2 * ((int64_t)a.E + a.Ncap);
    }
    return hd;
}

// [angle, dist] of the message j -> i from (dx, dy) = xy_j - xy_i (graph_functions.py:358-370): atan2(dx, dy) mod 2pi / 2pi
__device__ __forceinline__ void edge_attr_xy(float dx, float dy, float* ang, float* dst) {
    float a = atan2f(dx, dy);
    if (a < 0.0f) a += 6.283185307179586f;
    *ang = a / 6.283185307179586f;
    *dst = sqrtf(dy * dy + dx * dx);
}

static constexpr int QT_ATTN_BS = 64;      // one wave per workgroup (forward 32.4 -> 31.0 us at the cfg4 shapes; 128: 31.3)
// Addresses: the block bases (head, q / k / v / skip block) are uniform, so a row is reached as base + a 32-bit element offset
// (one VGPR per address instead of a 64-bit pair; the host checks that a head's rows span < 2^31 floats).
template <int LPN>
__global__ __launch_bounds__(QT_ATTN_BS) void k_attn_fwd(AttnArgs a, float* __restrict__ out, float* __restrict__ stats) {
    const int hd = head_setup<0>(a);
    out += hd * a.hs_o;
    stats += (int64_t)hd * 2 * a.Ncap;
    const int rows = qt_rows(a.n_dev, a.Ncap);
    const int blk = xcd_block(rows, QT_ATTN_BS / LPN);
    if (blk < 0) return;
    const int i = blk * (QT_ATTN_BS / LPN) + (int)threadIdx.x / LPN;
    if (i >= rows) return;
    const uint32_t j0 = ((uint32_t)threadIdx.x % LPN) * 4;
    const NodeOut r = node_forward<LPN>(a.rowptr, a.col, a.eattr, a.selfloop, a.proj, a.proj + a.ps, a.proj + 2 * a.ps, a.proj + 3 * a.ps,
                                        a.ld, a.We, i, j0, a.scale, a.keep, head_seed(a.seed, a.seed_dev, hd));
    st4(out + ((uint32_t)i * (uint32_t)a.ld_o + j0), r.o);
    put_stats(stats, i, j0, r);
}

// pass A: per target i -- dq_i = scale * sum_e alpha_e (t_e - D_i)(k_j + e), t_e = d_e g_i.(v_j + e), D_i = sum_e alpha_e t_e.
// D_i needs no edge loop of its own: sum_e alpha_e d_e (v_j + e) is the forward's attention output out_i - skip_i, so
// D_i = g_i . (out_i - skip_i) is known BEFORE the loop, and the loop can hand every message's final coefficients
// (ds_e, ad_e) = (scale alpha_e (t_e - D_i), alpha_e d_e) to the SOURCE of the message: they are written at rev[e], the slot of the
// transposed entry (row j, column i), which pass B then reads in row order -- no gather of coefficients, softmax statistics or D_i
// over there, only the q_i / g_i rows.
template <int LPN>
__global__ __launch_bounds__(QT_ATTN_BS) void k_attn_bwd_target(AttnArgs a, const float* __restrict__ g, const float* __restrict__ stats,
                                                         const float* __restrict__ outf, float* __restrict__ gproj) {
    const int hd = head_setup<1>(a);
    g += (hd % a.gmod) * a.hs_g;
    stats += (int64_t)hd * 2 * a.Ncap;
    gproj += hd * a.hs;
    outf += hd * a.hs_o;
    const int rows = qt_rows(a.n_dev, a.Ncap);
    const int blk = xcd_block(rows, QT_ATTN_BS / LPN);
    if (blk < 0) return;
    const int i = blk * (QT_ATTN_BS / LPN) + (int)threadIdx.x / LPN;
    if (i >= rows) return;
    const uint32_t j0 = ((uint32_t)threadIdx.x % LPN) * 4, ld = a.ld;
    const uint32_t oi = (uint32_t)i * ld + j0;
    const float* __restrict__ kb = a.proj + a.ps;
    const float* __restrict__ vb = a.proj + 2 * a.ps;
    const F4 q = ld4(a.proj + oi), gi = ld4(g + ((uint32_t)i * (uint32_t)a.ld_g + j0));
    float D;
    {
        const F4 sk = ld4(a.proj + 3 * a.ps + oi), of = ld4(outf + ((uint32_t)i * (uint32_t)a.ld_o + j0));
        F4 att;
#pragma unroll
        for (int c = 0; c < 4; ++c) att.v[c] = of.v[c] - sk.v[c];
        D = group_sum<LPN>(dot4(gi, att));
    }
    F4 w0, w1;
    we_columns(a.We, j0, &w0, &w1);
    const float m = stats[2 * i], l = stats[2 * i + 1];
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const int extra = (a.selfloop && a.selfloop[i] > 0.0f) ? 1 : 0;
    F4 dq = {{0, 0, 0, 0}};
    const uint32_t seed = head_seed(a.seed, a.seed_dev, hd);
    const int eend = e1 + extra;
    // A target with ONE pair has alpha = 1 and t = D: its score gradient is an exact zero.  D is taken from the stored output,
    // (v_j + e + skip_i) - skip_i, which has lost what the forward's rounding took, so t - D would leave g . skip x 2^-24 of noise
    // in dq_i / dk_j where the exact gradient (and any evaluation that forms D from the same products as t) is 0.
    const bool one_pair = eend - e0 == 1;
    for (int eb = e0; eb < eend; eb += EPT) {
        int rv[EPT];                    // where pair u's coefficients go: the transposed entry's slot, E + i for the self pair
#pragma unroll
        for (int u = 0; u < EPT; ++u) rv[u] = eb + u < e1 ? a.rev[eb + u] : a.E + i;
        Trip tr;
        tr.gather(a.col, a.eattr, kb, vb, ld, j0, i, eb, e1, eend);
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            if (tr.jj[u] < 0) break;
            const int j = tr.jj[u];
            const float ang = tr.ea[u].x, dst = tr.ea[u].y;
            F4 kj = tr.kk[u], vj = tr.vv[u];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float ee = w0.v[c] * ang + w1.v[c] * dst;
                kj.v[c] += ee;
                vj.v[c] += ee;
            }
            const float s = group_sum<LPN>(dot4(q, kj)) * a.scale;
            const float alpha = __expf(s - m) * inv;
            const float d = drop_mult(seed, i, j, a.keep);
            const float t = d * group_sum<LPN>(dot4(gi, vj));
            const float ds = one_pair ? 0.0f : alpha * (t - D) * a.scale;
            if (j0 == 0) *reinterpret_cast<float2*>(a.coef + 2 * (uint32_t)rv[u]) = make_float2(ds, alpha * d);
#pragma unroll
            for (int c = 0; c < 4; ++c) dq.v[c] += ds * kj.v[c];
        }
    }
    st4(gproj + oi, dq);
    if (!(a.accumulate & 2)) st4(gproj + 3 * a.ps + oi, gi);          // skip branch: identity (bit 1: g IS that block already)
}

// pass B: per source j over its outgoing messages j -> i (i runs over row j: the adjacency is symmetric).  Row j stores i -> j;
// the coefficients of j -> i were left at this row's own slots by pass A:
//   dk_j = sum_i ds q_i,  dv_j = sum_i ad g_i,  dWe = sum_edges (dk + dv terms) [angle, dist]
template <int LPN>
__global__ __launch_bounds__(256) void k_attn_bwd_source(AttnArgs a, const float* __restrict__ g, float* __restrict__ gproj,
                                                         float* __restrict__ part) {
    __shared__ float sm[4 * LPN * 2 * 4];
    const int hd = head_setup<2>(a);
    g += (hd % a.gmod) * a.hs_g;
    gproj += hd * a.hs;
    const uint32_t lj = threadIdx.x % LPN, j0 = lj * 4, ld = a.ld, ldg = a.ld_g;
    const int N = qt_rows(a.n_dev, a.Ncap);
    float acc[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[0][c] = acc[1][c] = 0.0f;
    // XCD x sweeps the contiguous eighth [x * per, (x + 1) * per) of the nodes with its share of the workgroups
    const bool split = gridDim.x >= 8;                      // (a handful of workgroups: plain sweep)
    const int xcd = split ? blockIdx.x & 7 : 0, wg = split ? blockIdx.x >> 3 : blockIdx.x;
    const int nwg = split ? (gridDim.x + 7 - xcd) >> 3 : gridDim.x;
    const int per = split ? (N + 7) >> 3 : N;
    const int jlo = xcd * per, jhi = jlo + per < N ? jlo + per : N;
    const int stride = nwg * (256 / LPN);
    for (int j = jlo + wg * (256 / LPN) + (int)threadIdx.x / LPN; j < jhi; j += stride) {
        F4 dk = {{0, 0, 0, 0}}, dv = {{0, 0, 0, 0}};
        const int e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
        const int extra = (a.selfloop && a.selfloop[j] > 0.0f) ? 1 : 0;
        const int eend = e1 + extra;
        for (int eb = e0; eb < eend; eb += EPT) {
            int ii[EPT];
            F4 qq[EPT], gg[EPT];
            float2 cf[EPT], ea[EPT];
#pragma unroll
            for (int u = 0; u < EPT; ++u) {
                const int e = eb + u;
                ii[u] = e < e1 ? a.col[e] : (e < eend ? j : -1);
            }
#pragma unroll
            for (int u = 0; u < EPT; ++u)
                if (ii[u] >= 0) {
                    const int e = eb + u;
                    const uint32_t slot = e < e1 ? e : a.E + j;
                    qq[u] = ld4(a.proj + ((uint32_t)ii[u] * ld + j0));
                    gg[u] = ld4(g + ((uint32_t)ii[u] * ldg + j0));
                    cf[u] = *reinterpret_cast<const float2*>(a.coef + 2 * slot);
                    ea[u] = e < e1 ? *reinterpret_cast<const float2*>(a.eattr + 2 * (uint32_t)e) : make_float2(0.0f, 0.0f);
                }
#pragma unroll
            for (int u = 0; u < EPT; ++u) {
                if (ii[u] < 0) break;
                float ang = 0.0f, dst = 0.0f;
                if (ii[u] != j) {                        // row j holds the attributes of i -> j: same distance, opposite direction
                    ang = ea[u].x + 0.5f;
                    if (ang >= 1.0f) ang -= 1.0f;
                    dst = ea[u].y;
                }
                const float ds = cf[u].x, ad = cf[u].y;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float dkc = ds * qq[u].v[c], dvc = ad * gg[u].v[c];
                    dk.v[c] += dkc;
                    dv.v[c] += dvc;
                    acc[0][c] += (dkc + dvc) * ang;      // d We[:, 0]
                    acc[1][c] += (dkc + dvc) * dst;      // d We[:, 1]
                }
            }
        }
        const uint32_t oj = (uint32_t)j * ld + j0;
        st4(gproj + a.ps + oj, dk);
        st4(gproj + 2 * a.ps + oj, dv);
    }
    // block reduction of the We partials (same scheme as the LSTM parameter gradients): [2][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = acc[k][c];
#pragma unroll
            for (int dd = LPN; dd < 64; dd <<= 1) v += __shfl_xor(v, dd, 64);
            acc[k][c] = v;
        }
    if (lane < LPN)
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) sm[(wave * LPN + lane) * 8 + k * 4 + c] = acc[k][c];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * a.C; idx += 256) {
        const int k = idx / a.C, ch = idx % a.C;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += sm[(w * LPN + (ch >> 2)) * 8 + k * 4 + (ch & 3)];
        float* pp = part + ((int64_t)blockIdx.x * gridDim.y + hd) * 2 * a.C + idx;     // (block, head)[k][channel]; the host transposes to (C, 2)
        *pp = (a.accumulate & 1) ? *pp + s : s;
    }
}

// [angle, dist] of every stored edge, once per mesh (the convolutions of a cell, forward and backward, and every time step on
// the same mesh reuse it)
__global__ void k_attn_edge_attrs(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                  const float* __restrict__ xy, int Ncap, const int32_t* __restrict__ n_dev,
                                  float* __restrict__ eattr, int32_t* __restrict__ rev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= qt_rows(n_dev, Ncap)) return;
    const float xi = xy[2 * i], yi = xy[2 * i + 1];
    for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int j = col[e];
        float ang = 0.0f, dst = 0.0f;
        if (j != i) edge_attr_xy(xy[2 * j] - xi, xy[2 * j + 1] - yi, &ang, &dst);
        eattr[2 * e] = ang;
        eattr[2 * e + 1] = dst;
        if (rev) {                              // the adjacency is symmetric: (j, i) is in row j (itself when absent)
            int r = e;
            for (int f = rowptr[j]; f < rowptr[j + 1]; ++f)
                if (col[f] == i) {
                    r = f;
                    break;
                }
            rev[e] = r;
        }
    }
}

constexpr int LPN_MAX = 32;       // C = 4 .. 128

void fill_args(AttnArgs* a, const int32_t* rowptr, const int32_t* col, const float* eattr, const float* selfloop, const float* proj,
               int ld, const float* We, int C, int c_real, int N, const int32_t* n_dev, float keep, uint32_t seed,
               const uint32_t* seed_dev) {
    a->rowptr = rowptr; a->col = col; a->eattr = eattr; a->selfloop = selfloop; a->proj = proj; a->We = We;
    a->ld = ld; a->C = C; a->Ncap = N; a->n_dev = n_dev; a->scale = 1.0f / sqrtf((float)c_real); a->keep = keep; a->seed = seed; a->seed_dev = seed_dev;
}

}  // namespace

extern "C" int qt_attn_blocks(int N, int C) {
    if (N <= 0 || !c_ok(C, LPN_MAX)) return 0;
    const int need = qt_cdiv((int64_t)N * (C / 4), 256);
static constexpr int QT_ATTN_BLOCKS = 4096;
    return need < QT_ATTN_BLOCKS ? need : QT_ATTN_BLOCKS;     // (512 left two waves per SIMD for a gather-latency-bound sweep)
}

extern "C" int qt_attn_edge_attrs(const int32_t* rowptr, const int32_t* col, const float* xy, int N, const int32_t* n_dev,
                                  float* eattr, int32_t* rev, void* stream) {
    QT_ARG(rowptr && col && xy && eattr, "null pointer");
    if (N <= 0) return QT_OK;
    hipLaunchKernelGGL(k_attn_edge_attrs, dim3(qt_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, xy, N, n_dev, eattr, rev);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_attn_fwd(const int32_t* rowptr, const int32_t* col, const float* xy, const float* eattr, const float* selfloop,
                           const float* proj, int ld, const float* We, int C, int c_real, int N, const int32_t* n_dev,
                           float keep, uint32_t seed, const uint32_t* seed_dev, float* out, float* stats, int G, int ld_o, int64_t ps, int64_t hs,
                           int64_t hs_o, void* stream) {
    QT_ARG(rowptr && col && eattr && proj && We && out && stats, "null pointer");
    if (G <= 0) G = 1;
    if (ps == 0) ps = C;
    if (hs == 0) hs = 4 * C;
    if (hs_o == 0) hs_o = C;
    if (ld_o == 0) ld_o = G * C;
    QT_ARG(c_ok(C, LPN_MAX) && ld >= C && ld % 4 == 0 && c_real >= 1 && c_real <= C, "bad channel count / row stride");
    QT_ARG(G <= 64 && ld_o >= C && ld_o % 4 == 0 && ps % 4 == 0 && hs % 4 == 0 && hs_o % 4 == 0, "bad head count / strides");
    QT_ARG((int64_t)N * ld < (1ll << 31) && (int64_t)N * ld_o < (1ll << 31), "a head's rows must span fewer than 2^31 floats");
    if (N <= 0) return QT_OK;
    AttnArgs a;
    fill_args(&a, rowptr, col, eattr, selfloop, proj, ld, We, C, c_real, N, n_dev, keep, seed, seed_dev);
    a.ld_g = C; a.accumulate = 0; a.rev = nullptr; a.coef = nullptr; a.E = 0; a.ld_o = ld_o; a.gmod = G;
    a.ps = ps; a.hs = hs; a.hs_o = hs_o; a.hs_g = C;
    const int grid = (qt_cdiv((int64_t)N * (C / 4), QT_ATTN_BS) + 7) & ~7;      // whole rounds over the 8 XCDs (xcd_block)
    QT_ATTN_LAUNCH(C, LPN_MAX, k_attn_fwd, dim3(grid, G), QT_ATTN_BS, stream, a, out, stats);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_attn_bwd(const int32_t* rowptr, const int32_t* col, const float* xy, const float* eattr, const float* selfloop,
                           const float* proj, int ld, const float* We, int C, int c_real, int N, const int32_t* n_dev,
                           float keep, uint32_t seed, const uint32_t* seed_dev, const float* g, int ld_g, const float* stats,
                           const float* out, int ld_o, float* gproj, float* part, int accumulate, const int32_t* rev, float* coef, int E,
                           int G, int gmod, int64_t ps, int64_t hs, int64_t hs_g, int64_t hs_o, void* stream) {
    QT_ARG(rowptr && col && xy && eattr && proj && We && g && stats && out && gproj && part && rev && coef, "null pointer");
    if (G <= 0) G = 1;
    if (gmod <= 0) gmod = G;
    if (ps == 0) ps = C;
    if (hs == 0) hs = 4 * C;
    if (hs_g == 0) hs_g = C;
    if (hs_o == 0) hs_o = C;
    if (ld_o == 0) ld_o = G * C;
    QT_ARG(c_ok(C, LPN_MAX) && ld >= C && ld % 4 == 0 && c_real >= 1 && c_real <= C, "bad channel count / row stride");
    if (ld_g == 0) ld_g = gmod * C;
    QT_ARG(G <= 64 && gmod <= G && ld_g >= C && ld_g % 4 == 0 && ((uintptr_t)g & 15) == 0 && ps % 4 == 0 && hs % 4 == 0 && hs_g % 4 == 0 &&
           ld_o >= C && ld_o % 4 == 0 && hs_o % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)coef & 7) == 0 && E >= 0,
           "bad head count / strides / alignment");
    QT_ARG((int64_t)N * ld < (1ll << 31) && (int64_t)N * ld_o < (1ll << 31) && (int64_t)N * ld_g < (1ll << 31) && (int64_t)E + N < (1ll << 30),
           "a head's rows must span fewer than 2^31 floats");
    if (N <= 0) return QT_OK;
    AttnArgs a;
    fill_args(&a, rowptr, col, eattr, selfloop, proj, ld, We, C, c_real, N, n_dev, keep, seed, seed_dev);
    a.ld_g = ld_g; a.accumulate = accumulate; a.rev = rev; a.coef = coef; a.E = E; a.ld_o = ld_o; a.gmod = gmod;
    a.ps = ps; a.hs = hs; a.hs_o = hs_o; a.hs_g = hs_g;
    const int grid = (qt_cdiv((int64_t)N * (C / 4), QT_ATTN_BS) + 7) & ~7;
    QT_ATTN_LAUNCH(C, LPN_MAX, k_attn_bwd_target, dim3(grid, G), QT_ATTN_BS, stream, a, g, stats, out, gproj);
    const int gridB = qt_attn_blocks(N, C);
    QT_ATTN_LAUNCH(C, LPN_MAX, k_attn_bwd_source, dim3(gridB, G), 256, stream, a, g, gproj, part);
    QT_LAUNCHED();
    return QT_OK;
}
