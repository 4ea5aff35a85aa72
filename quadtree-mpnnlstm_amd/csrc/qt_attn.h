// What the edge-softmax attention kernels share: attn.hip (TransformerConv, forward and backward), mhattn.hip (the fused
// multi-head forward) and attnw.hip (the coefficients written out).  One node per group of LPN = C/4 lanes (float4 each); the
// dropout rule; the gathers of a trip over EPT pairs of a node; the forward's online softmax; the LPN dispatch.
// Sums of two products (e_ij, dot4, the acc update) are left to the compiler's contraction, and which product the fma takes
// follows how the vectoriser paired the channels: the per-pair arithmetic therefore stays where it has always been compiled
// (node_forward, k_attn_bwd_target, attnw.hip's scores), each with the bits it has always produced.
#pragma once
#include "qt_cell.h"
#include <math.h>

namespace qtattn {

using qtcell::F4;
using qtcell::ld4;
using qtcell::st4;

// Sum over the node's lane group with xor shuffles.  Not qtcell::group_sum (DPP): the same bits but another instruction stream.
template <int LPN>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int d = 1; d < LPN; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float dot4(const F4& a, const F4& b) {
    return (a.v[0] * b.v[0] + a.v[1] * b.v[1]) + (a.v[2] * b.v[2] + a.v[3] * b.v[3]);
}

// Workgroups are dealt round-robin to the 8 XCDs, each with a private L2: XCD x gets the contiguous node range
// [x * chunk, (x + 1) * chunk) (chunk from the VALID rows), so a node's neighbours -- close in the mesh's node order -- sit in
// the L2 that gathers them (the same mapping as k_spmm).  Returns the node-group index of this workgroup or -1.
__device__ __forceinline__ int xcd_block(int rows, int nodes_per_block) {
    const int nblk = (rows + nodes_per_block - 1) / nodes_per_block;
    const int chunk = (nblk + 7) >> 3;
    const int bid = blockIdx.x;
    if ((bid >> 3) >= chunk) return -1;
    return (bid & 7) * chunk + (bid >> 3);
}

// Inverted-dropout multiplier of the attention coefficient of the pair (j -> i): a counter hash, so the forward (single- or
// multi-head, fused or not) and both backward passes draw the same mask from the same seed.
__device__ __forceinline__ float drop_mult(uint32_t seed, int i, int j, float keep) {
    if (keep >= 1.0f) return 1.0f;
    uint32_t h = seed ^ ((uint32_t)i * 0x9E3779B1u) ^ ((uint32_t)j * 0x85EBCA77u);
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return ((h >> 8) * (1.0f / 16777216.0f)) < keep ? 1.0f / keep : 0.0f;
}
// The seed of head hd: every head draws its own mask; seed_dev is an optional step counter on the device, so that a captured
// launch (fixed `seed` argument) still draws a new mask at every replay.
__device__ __forceinline__ uint32_t head_seed(uint32_t seed, const uint32_t* seed_dev, int hd) {
    const uint32_t s = seed + (uint32_t)hd * 0x632BE5ABu;
    return seed_dev ? s ^ (*seed_dev * 0x9E3779B9u) : s;
}

// this lane's four rows of We (C, 2), by column: e_ij = w0 angle + w1 dist
__device__ __forceinline__ void we_columns(const float* We, uint32_t j0, F4* w0, F4* w1) {
    *w0 = F4{{We[2 * j0], We[2 * j0 + 2], We[2 * j0 + 4], We[2 * j0 + 6]}};
    *w1 = F4{{We[2 * j0 + 1], We[2 * j0 + 3], We[2 * j0 + 5], We[2 * j0 + 7]}};
}

// Pairs per trip (their gathers are issued together).  8 heads at the cfg4 shapes, forward / target / source pass:
// 1: 178 / 258 / 194 us, 2: 158 / 266 / 181, 4: 202 / 313 / 231 -- fewer registers, more waves
constexpr int EPT = 2;

// The gathers of one trip over the pairs eb .. eb + EPT - 1 of target i, issued together: stored edges [.., e1), then the self
// pair when eend = e1 + 1 (source i, attributes (0, 0)).  kb / vb are the k / v block bases of the head, rows ld floats apart,
// reached by 32-bit offsets.  The caller then takes the pairs in edge order.
struct Trip {
    int jj[EPT];            // source of pair u; < 0 past the node's last pair
    F4 kk[EPT], vv[EPT];
    float2 ea[EPT];

    __device__ __forceinline__ void gather(const int32_t* col, const float* eattr,
                                           const float* kb, const float* vb, uint32_t ld, uint32_t j0,
                                           int i, int eb, int e1, int eend) {
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            const int e = eb + u;
            jj[u] = e < e1 ? col[e] : (e < eend ? i : -1);
        }
#pragma unroll
        for (int u = 0; u < EPT; ++u)
            if (jj[u] >= 0) {
                const uint32_t off = (uint32_t)jj[u] * ld + j0;
                kk[u] = ld4(kb + off);
                vv[u] = ld4(vb + off);
                ea[u] = eb + u < e1 ? *reinterpret_cast<const float2*>(eattr + 2 * (uint32_t)(eb + u)) : make_float2(0.0f, 0.0f);
            }
    }
};

// Forward of one node and head: online softmax with dropout over the node's pairs in edge order, then
// o = sum_j d_ij alpha_ij (v_j + e_ij) + skip_i for this lane's four channels.  qb / kb / vb / sb: the head's q | k | v | skip
// block bases; stats: the head's (N, 2) rows, written (m, l) by lane 0 of the group.
struct NodeOut {
    F4 o;
    float m, l;         // softmax statistics: running max, sum of exp(s - m) before dropout
};
template <int LPN>
__device__ __forceinline__ NodeOut node_forward(const int32_t* rowptr, const int32_t* col,
                                           const float* eattr, const float* selfloop,
                                           const float* qb, const float* kb, const float* vb,
                                           const float* sb, uint32_t ld, const float* We, int i, uint32_t j0,
                                           float scale, float keep, uint32_t seed) {
    const F4 q = ld4(qb + ((uint32_t)i * ld + j0));
    F4 w0, w1;
    we_columns(We, j0, &w0, &w1);
    float m = -INFINITY, l = 0.0f;
    F4 acc = {{0, 0, 0, 0}};
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const int eend = e1 + ((selfloop && selfloop[i] > 0.0f) ? 1 : 0);
    for (int eb = e0; eb < eend; eb += EPT) {
        Trip t;
        t.gather(col, eattr, kb, vb, ld, j0, i, eb, e1, eend);
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            if (t.jj[u] < 0) break;                     // (uniform over the node's lane group)
            const int j = t.jj[u];
            const float ang = t.ea[u].x, dst = t.ea[u].y;       // stored per edge: no atan2 / sqrt in the loop
            F4 kj = t.kk[u], vj = t.vv[u];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float ee = w0.v[c] * ang + w1.v[c] * dst;
                kj.v[c] += ee;
                vj.v[c] += ee;
            }
            const float s = group_sum<LPN>(dot4(q, kj)) * scale;
            const float mn = fmaxf(m, s);
            const float r = __expf(m - mn), p = __expf(s - mn);       // m = -inf on the first pair: r = 0
            const float pd = p * drop_mult(seed, i, j, keep);
            l = l * r + p;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc.v[c] = acc.v[c] * r + pd * vj.v[c];
            m = mn;
        }
    }
    const F4 sk = ld4(sb + ((uint32_t)i * ld + j0));
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    F4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o.v[c] = acc.v[c] * inv + sk.v[c];
    return NodeOut{o, m, l};
}
// (m, l) of node i into the head's stats rows, by lane 0 of the group
__device__ __forceinline__ void put_stats(float* stats, int i, uint32_t j0, const NodeOut& r) {
    if (j0 == 0) {
        stats[2 * i] = r.m;
        stats[2 * i + 1] = r.l;
    }
}

// channel counts the kernels are built for: 4 lanes_max >= C = 4 LPN, LPN a power of two
inline bool c_ok(int C, int lanes_max) { return C >= 4 && C <= 4 * lanes_max && (C & (C - 1)) == 0; }

}  // namespace qtattn

// Launches KERNEL<LPN> for LPN = C / 4 in {1, 2, 4, .., LPN_MAX}: only those are instantiated (the entry's c_ok check comes first).
#define QT_ATTN_LAUNCH_(L, LPN_MAX, KERNEL, grid, BS, stream, ...) \
    hipLaunchKernelGGL(KERNEL<((L) < (LPN_MAX) ? (L) : (LPN_MAX))>, dim3(grid), dim3(BS), 0, (hipStream_t)stream, __VA_ARGS__)
#define QT_ATTN_LAUNCH(C, LPN_MAX, KERNEL, grid, BS, stream, ...)                           \
    switch ((C) / 4) {                                                                      \
        case 1: QT_ATTN_LAUNCH_(1, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break;  \
        case 2: QT_ATTN_LAUNCH_(2, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break;  \
        case 4: QT_ATTN_LAUNCH_(4, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break;  \
        case 8: QT_ATTN_LAUNCH_(8, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break;  \
        case 16: QT_ATTN_LAUNCH_(16, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break; \
        default: QT_ATTN_LAUNCH_(32, LPN_MAX, KERNEL, grid, BS, stream, __VA_ARGS__); break; \
    }
