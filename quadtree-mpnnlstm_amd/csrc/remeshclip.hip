// Clip-resident mesh -> mesh state transfer (the re-mesh of model/seq2seq.py:434-491: unflatten on the old mesh + flatten on
// the new one, :440-442 + :474-477, fused; its backward is the same op with the meshes swapped).
//
//   out[new node i] = (mean ? 1 / npix[i] : 1) * sum over the pixels p of node i of  S[src_label[p]] (* 1 / src_npix[..] if src_inv)
//
// The general kernels (transfer.hip: k_pool_nodes for nodes up to 4 x 4 pixels, k_pool for the bigger ones) walk
// index -> label -> row chains through L2 / HBM for every node and channel chunk, 41 - 52 us per transfer of the benchmark's
// 68 state channels.  Here one workgroup owns one 32 x 32 pixel QUADRANT of one 64 x 64 tile (= base cell) of a clip and one
// COLUMN GROUP: up to four consecutive float4 chunks (64 bytes) that lie in one source part and in one output part -- for the
// dense 16-wide state parts (H and C of a layer) a group is the whole 64-byte row, so four neighbouring lanes load / store one
// row and a wave instruction moves 16 whole rows (1 KB, contiguous while staging):
//   * lane t & 3 owns one float4 chunk of the group, lanes t >> 2 enumerate the quadrant's 256 2 x 2 pixel blocks (Morton order);
//   * the source rows of the quadrant's pixels are found by the workgroup itself (min / max of its valid source labels); labels
//     are in depth-first order, so for quadtree meshes that range has at most 1024 rows = 64 KB of LDS and is staged once
//     (pre-scaled by 1 / src_npix for the backward).  Any other mesh (preset order, pixelwise: the range can be the whole clip)
//     is walked in windows of 1024 rows: a pixel takes its value in the window that holds its source row -- an assignment, not
//     a sum, so the bits do not depend on the windows;
//   * a sum pyramid over the quadrant: level 1 in registers, levels 2 and 3 by lane shuffles (a wave is one 8 x 8 entry),
//     levels 4 and 5 from the 16 waves' level-3 sums through 1 KB of LDS -- a quadtree leaf of level L is exactly one level-L
//     entry, so every destination node is written once, deterministically, by the lanes that own its head pixel.  A node of
//     level 6 (a whole tile) is formed by the tile's quadrant-0 workgroup, which walks all four quadrants.
// No per-node cell record, no direct-index side array, no pixel loops of data-dependent length, no atomics.  Summation order:
// (top-left + top-right) + (bottom-left + bottom-right) at every level.
#include "qt_transfer.h"
#include <type_traits>

namespace {
using namespace qttransfer;

constexpr int RC_T = 1024;          // threads of a workgroup: 256 2 x 2 pixel blocks of a quadrant x 4 float4 chunks
constexpr int RC_ROWS = 4096;       // source rows of a clip that fit (qt_remesh_clip_rows: a 64 x 64 frame's pixels)
constexpr int RC_WIN = 1024;        // source rows staged at a time (64 bytes each)
constexpr int RC_GROUPS = 256;      // column groups of one launch

struct RcArgs {
    PartTable<const float> sparts;  // the source state and
    PartTable<float> oparts;        // the result, each as up to 8 matrices side by side
    const int32_t* src_labels;      // (B, n, m) source mesh
    const float* src_npix;
    const int32_t* labels;          // (B, n, m) destination mesh
    const uint8_t* level;
    const float* npix;
    int src_inv, mean, B, n, m, tiles_c, tiles;
    // the decoder's next input assembled by the transfer itself (model/seq2seq.py:484-487: [transferred output value | position,
    // size]): float4 chunk 0 of the result is written as (value.x, posfeat[node]) when posfeat != NULL -- and in the transposed
    // transfer only column 0 of chunk 0 of the SOURCE counts (src_first_only): the gradient of that assembly
    const float* posfeat;
    int src_first_only;
    int ride;                       // 1: chunk 0 is the decoder input's scalar (posfeat or src_first_only, and more chunks follow): it has no
                                    // column group of its own, the workgroups of the first group carry its column 0 along
    int ngroups;
    unsigned grp[RC_GROUPS];        // column group g = float4 chunks [grp & 0xffff, + (grp >> 16)), 1 .. 4 of them
};

__device__ __forceinline__ unsigned compact_bits(unsigned v) {       // even bits of v -> low half
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    return v;
}

// quad_add over four lanes: the lanes hold child 0 .. child 3 of an entry (Morton order, child = row bit | col bit << 1)
// 1 << sh lanes apart -> every one of them gets (c0 + c2) + (c1 + c3) (a + b = b + a bit for bit, so the four lanes hold the
// same bits; in two shuffles, where quad_add itself would take three).  sh = log2 of the distance between the children: 2 and
// 4 for levels 2 and 3.
__device__ __forceinline__ float quad_sum(float v, int sh) {
    const float a = v + __shfl_xor(v, 2 << sh, 64);
    return a + __shfl_xor(a, 1 << sh, 64);
}
__device__ __forceinline__ float4 quad_sum4(float4 v, int sh) {
    return make_float4(quad_sum(v.x, sh), quad_sum(v.y, sh), quad_sum(v.z, sh), quad_sum(v.w, sh));
}

// 64 KB + 4 KB + 1.5 KB of LDS and <= 64 registers: TWO workgroups per CU; the benchmark's 32 clips x 4 quadrants x 4 groups
// (H0, C0, H1, C1; the decoder input's scalar chunk RIDES with the first: ride) = 512 workgroups, all resident at once.
__global__ __launch_bounds__(RC_T, 8) void k_remesh_clip(RcArgs a) {
    __shared__ float4 A[RC_WIN * 4];              // a window of source rows of the group: row r, chunk k at A[4 r + k]
    __shared__ float A0[RC_WIN];                  // the rider: column 0 of chunk 0 of the same rows
    __shared__ float4 S3[16 * 4];                 // the 16 waves' level-3 sums (8 x 8 pixels), per chunk
    __shared__ float S30[16];
    __shared__ float4 S5[4 * 4];                  // level-6 walk: the four quadrants' level-5 sums (read back by their writers)
    __shared__ float S50[4];
    __shared__ int smin[16], smax[16];
    const int t = threadIdx.x;
    const int k = t & 3, j = t >> 2, w = t >> 6;
    const int b = (int)blockIdx.x % a.B;
    int rest = (int)blockIdx.x / a.B;
    const int tile = rest % a.tiles;
    rest /= a.tiles;
    const int qd = rest & 3, g = rest >> 2;
    const unsigned grp = a.grp[g];
    const int ch0 = (int)(grp & 0xffffu), nch = (int)(grp >> 16);
    const int ch = ch0 + k;                       // this lane's float4 chunk
    const bool mine = k < nch;                    // (groups narrower than four chunks: the spare lanes move nothing)
    const bool ride = a.ride && g == 0;           // (workgroup-uniform) this workgroup also transfers column 0 of chunk 0
    const int R0 = (tile / a.tiles_c) * 64, C0 = (tile % a.tiles_c) * 64;
    const int P = a.n * a.m;
    // row 0 of the group's first chunk = the group's base in its source / output part, with that part's row stride (a group
    // lies inside one part); rows and the lane's chunk are added where they are used
    int lds, ldd;
    // (uniform base + a small per-lane offset: the spare lanes of a narrow group read its last chunk again)
    const float* src = part_chunk(a.sparts, 0, ch0, &lds);
    const int ksrc = 4 * min(k, nch - 1);
    float* dst = part_chunk(a.oparts, 0, ch0, &ldd);         // (uniform; + 4 k per lane)
    const float* src0 = a.sparts.p[0];
    const int lds0 = a.sparts.ld[0];
    const bool first_only = a.src_first_only && ch == 0;       // (the scalar chunk on its own: a transfer of that chunk alone)
    const bool dec = a.posfeat != nullptr;          // chunk 0 of the result = [value | position, size] of the node
    float* dst0 = a.oparts.p[0];
    const int ldd0 = a.oparts.ld[0];
    auto put = [&](int node, float4 v) {
        if (dec && ch == 0) {
            const float* pf = a.posfeat + 3 * (int64_t)node;
            v.y = pf[0]; v.z = pf[1]; v.w = pf[2];
        }
        *reinterpret_cast<float4*>(dst + ((int64_t)node * ldd + 4 * k)) = v;
    };
    auto put0 = [&](int node, float v) {            // the rider's result row: (value, position, size) or (gradient, 0, 0, 0)
        float4 o = make_float4(v, 0.0f, 0.0f, 0.0f);
        if (dec) {
            const float* pf = a.posfeat + 3 * (int64_t)node;
            o.y = pf[0]; o.z = pf[1]; o.w = pf[2];
        }
        *reinterpret_cast<float4*>(dst0 + (int64_t)node * ldd0) = o;
    };
    // a tile that is ONE destination node (level 6; its head pixel is the tile's first): the quadrant-0 workgroup walks the four
    // quadrants, the other three have nothing to write
    bool walk = false;
    {
        const int64_t p0 = (int64_t)b * P + (int64_t)R0 * a.m + C0;
        walk = a.labels[p0] >= 0 && a.level[p0] >= 6;
    }
    if (walk && qd != 0) return;
    int node6 = -1;
    float oscale6 = 1.0f;

    // one quadrant: WALK = it is one of the four of a level-6 node (nothing is written, its level-5 sum is kept)
    auto quadrant = [&](int qq, auto walk_c) {
        constexpr bool WALK = decltype(walk_c)::value;
        int jq = j, wq = w;
        if (WALK) asm volatile("" : "+v"(jq), "+v"(wq));      // (the walk recomputes its per-lane indices in every quadrant: nothing held across)
        const int br = (int)compact_bits((unsigned)jq), bc = (int)compact_bits((unsigned)jq >> 1);     // jq = spread(br) | spread(bc) << 1
        const int rq = 32 * (qq & 1) + 2 * br, cq = 32 * (qq >> 1) + 2 * bc;     // this block's first pixel inside the tile
        // ---- the labels / levels of this lane's 2 x 2 pixels, and the range of the quadrant's source rows
        int lab[4], sl[4];
        unsigned lv = 0;                            // the four pixels' levels, one byte each
        int lo = 0x7fffffff, hi = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = R0 + rq + (q >> 1), c = C0 + cq + (q & 1);
            lab[q] = sl[q] = -1;
            if (r < a.n && c < a.m) {
                const int64_t p = (int64_t)b * P + (int64_t)r * a.m + c;
                lab[q] = a.labels[p];
                sl[q] = a.src_labels[p];
                lv |= (unsigned)a.level[p] << (8 * q);
            }
            if (lab[q] < 0) sl[q] = -1;           // (a pixel counts when both meshes hold it)
            if (sl[q] >= 0) {
                lo = min(lo, sl[q]);
                hi = max(hi, sl[q]);
            }
        }
        const int L = lab[0] >= 0 ? (int)(lv & 255u) : 0;      // a node of level >= 1 has its head at a block's first pixel
        float oscale = 1.0f;
        if (L >= 1 && a.mean) oscale = 1.0f / a.npix[lab[0]];          // (requested before the pyramid, used after it)
#pragma unroll
        for (int d = 4; d < 64; d <<= 1) {          // (the four lanes of a block hold the same labels)
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
        if ((t & 63) == 0) {
            smin[wq] = lo;
            smax[wq] = hi;
        }
        qt_lds_barrier();                              // (also: the previous quadrant's gathers and S3 reads are done)
        lo = smin[t & 15];
        hi = smax[t & 15];
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
        lo = __builtin_amdgcn_readfirstlane(lo);    // (the same in every lane: the window loop is uniform)
        hi = __builtin_amdgcn_readfirstlane(hi);
        // ---- pixel values: stage a window of source rows, gather.  Quadtree meshes: the first window is the whole range
        // (4 rows per lane, loads first); the windows after it (any other mesh) go row by row
        float4 v[4];
        float v0[4];
        auto stage = [&](int wb, int nr, int u0, int u1, float4* x, float* x0, float* sc) {
            const float* srcw = src + (int64_t)wb * lds;           // (uniform)
            const float* srcw0 = src0 + (int64_t)wb * lds0;
            const float* npixw = a.src_npix + wb;
            for (int u = u0; u < u1; ++u) {
                const int lr = min(jq + 256 * u, nr - 1);          // (rows past the window: its last row again, not kept)
                x[u - u0] = *reinterpret_cast<const float4*>(srcw + (unsigned)(lr * lds + ksrc));
                x0[u - u0] = 0.0f;
                sc[u - u0] = 1.0f;
                if (ride) x0[u - u0] = srcw0[(unsigned)(lr * lds0)];
                if (a.src_inv) sc[u - u0] = npixw[(unsigned)lr];
            }
            for (int u = u0; u < u1; ++u) {
                float4 xx = x[u - u0];
                if (first_only) xx.y = xx.z = xx.w = 0.0f;
                const int lr = jq + 256 * u;
                if (lr < nr) {
                    const float inv = a.src_inv ? 1.0f / sc[u - u0] : 1.0f;
                    A[4 * lr + k] = a.src_inv ? mul4(xx, inv) : xx;
                    if (ride) A0[lr] = a.src_inv ? x0[u - u0] * inv : x0[u - u0];          // (four lanes, one value)
                }
            }
        };
        const bool any = lo <= hi;                  // (uniform; no valid pixel, e.g. a masked quadrant: nothing to stage, no window)
        const int wb0 = any ? lo & ~1 : 0;          // (even first row: whole 128-byte lines)
        if (any) {
            float4 x[4];
            float x0[4], sc[4];
            stage(wb0, min(hi - wb0 + 1, RC_WIN), 0, 4, x, x0, sc);
        }
        qt_lds_barrier();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned lr = (unsigned)(sl[q] - wb0);
            const bool in = sl[q] >= 0 && lr < (unsigned)RC_WIN;
            v[q] = A[in ? 4 * lr + k : k];
            v0[q] = ride ? A0[in ? lr : 0] : 0.0f;
            if (!in) {
                v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                v0[q] = 0.0f;
            }
        }
#pragma nounroll
        for (int wb = wb0 + RC_WIN; any && wb <= hi; wb += RC_WIN) {
            const int nr = min(hi - wb + 1, RC_WIN);
            qt_lds_barrier();                          // the previous window's gathers are done
#pragma nounroll
            for (int u = 0; u < 4; ++u) {
                float4 x[1];
                float x0[1], sc[1];
                stage(wb, nr, u, u + 1, x, x0, sc);
            }
            qt_lds_barrier();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned lr = (unsigned)(sl[q] - wb);
                if (sl[q] >= 0 && lr < (unsigned)RC_WIN) {        // (every pixel has one source row: it is in one window)
                    v[q] = A[4 * lr + k];
                    if (ride) v0[q] = A0[lr];
                }
            }
        }
        // ---- single-pixel nodes
        if (!WALK) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (lab[q] >= 0 && ((lv >> (8 * q)) & 255u) == 0) {
                    if (mine) put(lab[q], v[q]);
                    if (ride && k == 0) put0(lab[q], v0[q]);
                }
        }
        // ---- sum pyramid, (top-left + top-right) + (bottom-left + bottom-right) at every level: level 1 in registers, levels 2
        // and 3 between lanes 4 / 8 and 16 / 32 apart, the waves' level-3 sums through LDS
        const float4 s1 = quad_add(v[0], v[1], v[2], v[3]);
        const float4 s2 = quad_sum4(s1, 2), s3 = quad_sum4(s2, 4);
        float r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
        if (ride) {
            r1 = quad_add(v0[0], v0[1], v0[2], v0[3]);
            r2 = quad_sum(r1, 2); r3 = quad_sum(r2, 4);
        }
        if ((t & 63) < 4) {
            S3[4 * wq + k] = s3;
            if (k == 0) S30[wq] = r3;
        }
        qt_lds_barrier();
        // levels 4 and 5: the first wave of every level-4 entry sums its four waves' entries (wave 0: lanes 4 e + k take entry e,
        // so that its lanes 0 .. 15 hold the quadrant's four level-4 sums and two more shuffles give level 5)
        float4 s4 = s3, s5 = s3;
        float r4 = r3, r5 = r3;
        if ((w & 3) == 0) {                         // (wave-uniform)
            const int e = w == 0 ? (j & 3) : w >> 2;
            s4 = quad_add(S3[16 * e + k], S3[16 * e + 8 + k], S3[16 * e + 4 + k], S3[16 * e + 12 + k]);
            if (ride) r4 = quad_add(S30[4 * e], S30[4 * e + 2], S30[4 * e + 1], S30[4 * e + 3]);
            if (w == 0) {
                s5 = quad_sum4(s4, 2);
                if (ride) r5 = quad_sum(r4, 2);
            }
        }
        if (WALK) {
            // the quadrant's level-5 sum, kept by the four lanes that write the node in the end
            if (t < 4) {
                S5[4 * qq + k] = s5;
                if (ride && k == 0) S50[qq] = r5;
                if (qq == 0) {
                    node6 = lab[0];
                    oscale6 = oscale;
                }
            }
            return;
        }
        // ---- every node of level >= 1 is written by the lanes that own its head pixel (the block's first pixel, aligned to 2^L)
        if (L >= 1 && (rq & ((1 << L) - 1)) == 0 && (cq & ((1 << L) - 1)) == 0) {
            float4 s;
            float r;
            switch (L) {
                case 1: s = s1; r = r1; break;
                case 2: s = s2; r = r2; break;
                case 3: s = s3; r = r3; break;
                case 4: s = s4; r = r4; break;
                default: s = s5; r = r5; break;     // (level 5: the quadrant)
            }
            if (mine) put(lab[0], mul4(s, oscale));
            if (ride && k == 0) put0(lab[0], r * oscale);
        }
    };
    if (!walk) {
        quadrant(qd, std::false_type());
        return;
    }
#pragma nounroll
    for (int qq = 0; qq < 4; ++qq) quadrant(qq, std::true_type());
    if (t < 4 && node6 >= 0) {
        const float4 s = quad_add(S5[k], S5[8 + k], S5[4 + k], S5[12 + k]);
        if (mine) put(node6, mul4(s, oscale6));
        if (ride && k == 0) put0(node6, quad_add(S50[0], S50[2], S50[1], S50[3]) * oscale6);
    }
}

// The same pyramid for image -> mesh pooling of scalar channels (flatten, model/graph_functions.py:391-419: the encoder's input
// frames, the decoder's concat layer, the loss targets): one workgroup per (clip, frame, channel); a pixel's value comes straight
// from the image, so nothing is staged.  img (B, S, n*m, C) with clip stride img_clip_stride; out[(s * N + node) * out_stride +
// out_coff + c].
struct PcArgs {
    const float* img;
    int64_t img_clip_stride;
    int S, C;
    const int32_t* labels;
    const uint8_t* level;
    const float* npix;
    int mean, B, n, m, N, tiles_c, tiles;
    float* out;
    int out_stride, out_coff;
};

__global__ __launch_bounds__(RC_T) void k_pool_clip(PcArgs a) {
    __shared__ float L1[1024], L2[256], L3[64], L4[16], L5[4], L6[1];
    const int t = threadIdx.x;
    const int b = (int)blockIdx.x % a.B;
    const int rest = (int)blockIdx.x / a.B;
    const int tile = rest % a.tiles, sc_ = rest / a.tiles;
    const int R0 = (tile / a.tiles_c) * 64, C0 = (tile % a.tiles_c) * 64;
    const int s = sc_ / a.C, c = sc_ - s * a.C;
    const int P = a.n * a.m;
    const float* img = a.img + (int64_t)b * a.img_clip_stride + (int64_t)s * P * a.C + c;
    float* out = a.out + (int64_t)s * a.N * a.out_stride + a.out_coff + c;
    const int br = (int)compact_bits((unsigned)t), bc = (int)compact_bits((unsigned)t >> 1);
    int lab[4], lv[4];
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = R0 + 2 * br + (q >> 1), cc = C0 + 2 * bc + (q & 1);
        lab[q] = -1;
        lv[q] = 0;
        v[q] = 0.0f;
        if (r < a.n && cc < a.m) {
            const int p = r * a.m + cc;
            lab[q] = a.labels[(int64_t)b * P + p];
            lv[q] = a.level[(int64_t)b * P + p];
            v[q] = img[(int64_t)p * a.C];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (lab[q] < 0) v[q] = 0.0f;
        else if (lv[q] == 0) out[(int64_t)lab[q] * a.out_stride] = v[q];
    }
    const float s1 = quad_add(v[0], v[1], v[2], v[3]);
    const int L = lab[0] >= 0 ? lv[0] : 0;
    float oscale = 1.0f;
    if (L >= 1 && a.mean) oscale = 1.0f / a.npix[lab[0]];
    L1[t] = s1;
    qt_lds_barrier();
    if (t < 256) L2[t] = quad_add(L1[4 * t], L1[4 * t + 2], L1[4 * t + 1], L1[4 * t + 3]);
    qt_lds_barrier();
    if (t < 64) L3[t] = quad_add(L2[4 * t], L2[4 * t + 2], L2[4 * t + 1], L2[4 * t + 3]);
    qt_lds_barrier();
    if (t < 16) L4[t] = quad_add(L3[4 * t], L3[4 * t + 2], L3[4 * t + 1], L3[4 * t + 3]);
    qt_lds_barrier();
    if (t < 4) L5[t] = quad_add(L4[4 * t], L4[4 * t + 2], L4[4 * t + 1], L4[4 * t + 3]);
    qt_lds_barrier();
    if (t < 1) L6[0] = quad_add(L5[0], L5[2], L5[1], L5[3]);
    qt_lds_barrier();
    if (L >= 1 && ((2 * br) & ((1 << L) - 1)) == 0 && ((2 * bc) & ((1 << L) - 1)) == 0) {
        float sum;
        switch (L) {
            case 1: sum = s1; break;
            case 2: sum = L2[t >> 2]; break;
            case 3: sum = L3[t >> 4]; break;
            case 4: sum = L4[t >> 6]; break;
            case 5: sum = L5[t >> 8]; break;
            default: sum = L6[0]; break;
        }
        out[(int64_t)lab[0] * a.out_stride] = sum * oscale;
    }
}

}  // namespace

extern "C" int qt_remesh_clip_rows(void) { return RC_ROWS; }

extern "C" int qt_remesh_clip(const float* const* src_parts, const int* widths, const int* lds, int nparts,
                              const int32_t* src_labels, const float* src_npix, int src_inv, const int32_t* src_cell_off,
                              const int32_t* labels, const uint8_t* level, const float* npix, int mean, int B, int n, int m,
                              float* const* out_parts, const int* out_widths, int nout, const float* posfeat, int src_first_only,
                              void* stream) {
    QT_ARG(src_parts && widths && lds && nparts >= 1 && nparts <= 8 && src_labels && src_cell_off && labels && level && B > 0,
           "bad arguments");
    QT_ARG(n >= 1 && m >= 1, "empty frame");
    QT_ARG(out_parts && out_widths && nout >= 1 && nout <= 8, "bad output parts");
    QT_ARG(!mean || npix, "mean pooling needs npix");
    QT_ARG(!src_inv || src_npix, "src_inv needs src_npix");
    RcArgs a = {};
    const int c4 = fill_parts(__func__, "source parts must be 16-byte aligned with widths / strides that are multiples of 4", src_parts,
                              widths, lds, nparts, a.sparts);
    if (c4 < 0) return QT_E_ARG;
    const int o4 = fill_parts(__func__, "output parts must be 16-byte aligned with widths that are multiples of 4", out_parts, out_widths,
                              nullptr, nout, a.oparts);
    if (o4 < 0) return QT_E_ARG;
    QT_ARG(o4 == c4, "the output parts must add up to the source width");
    QT_ARG(c4 < (1 << 16), "state too wide");
    a.src_labels = src_labels;
    a.src_npix = src_npix;
    a.tiles_c = qt_cdiv(m, 64);
    a.tiles = qt_cdiv(n, 64) * a.tiles_c;
    a.labels = labels;
    a.level = level;
    a.npix = npix;
    a.src_inv = src_inv;
    a.mean = mean;
    a.B = B;
    a.n = n;
    a.m = m;
    a.posfeat = posfeat;
    a.src_first_only = src_first_only;
    a.ride = (posfeat || src_first_only) && c4 > 1 && widths[0] == 4 && out_widths[0] == 4 ? 1 : 0;
    // column groups: runs of up to four chunks inside one source part and one output part (the rider's chunk 0 has none)
    int sp = 0, op = 0;
    for (int c = a.ride; c < c4;) {
        while (c >= a.sparts.end[sp]) ++sp;
        while (c >= a.oparts.end[op]) ++op;
        const int e = std::min(std::min(a.sparts.end[sp], a.oparts.end[op]), c + 4);
        QT_ARG(a.ngroups < RC_GROUPS, "too many column groups for one launch");
        a.grp[a.ngroups++] = (unsigned)c | (unsigned)(e - c) << 16;
        c = e;
    }
    QT_ARG((int64_t)B * a.tiles * 4 * a.ngroups < ((int64_t)1 << 31), "grid too large");
    hipLaunchKernelGGL(k_remesh_clip, dim3(B * a.tiles * 4 * a.ngroups), dim3(RC_T), 0, (hipStream_t)stream, a);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_pool_clip(const float* img, int S, int64_t img_clip_stride, int C, const int32_t* labels, const uint8_t* level,
                            const float* npix, int mean, int B, int n, int m, int N, float* out, int out_stride, int out_coff,
                            void* stream) {
    QT_ARG(img && labels && level && out && S >= 1 && C >= 1 && B > 0, "bad arguments");
    QT_ARG(n >= 1 && m >= 1, "empty frame");
    QT_ARG(!mean || npix, "mean pooling needs npix");
    QT_ARG(out_stride >= out_coff + C, "output row too short");
    if (N <= 0) return QT_OK;
    const int tiles_c = qt_cdiv(m, 64), tiles = qt_cdiv(n, 64) * tiles_c;
    QT_ARG((int64_t)B * tiles * S * C < ((int64_t)1 << 31), "grid too large");
    PcArgs a = {img, img_clip_stride > 0 ? img_clip_stride : (int64_t)S * n * m * C, S, C, labels, level, npix, mean, B, n, m, N,
                tiles_c, tiles, out, out_stride, out_coff};
    hipLaunchKernelGGL(k_pool_clip, dim3(B * tiles * S * C), dim3(RC_T), 0, (hipStream_t)stream, a);
    QT_LAUNCHED();
    return QT_OK;
}
