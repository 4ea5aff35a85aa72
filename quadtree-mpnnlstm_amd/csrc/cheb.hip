// Chebyshev message aggregate (PyG ChebConv as used by model/model.py:53,96):
//   k_spmm  -- the CSR message-aggregate  out = alpha * L^ x + beta * p + gamma * q
//   k_spmm1 -- the same on single strided columns, with an optional output epilogue
// The dense products that turn the aggregated planes into outputs are in gemm.hip, the gate-cell launches in gatecell.hip.
#include "qt_aggr.h"      // the row rule: ELL head, four-edge chain
#include "qt_gemm.h"      // (act_quad: the epilogue activation, shared with the dense kernels)

namespace {

// ------------------------------------------------------------------ message aggregate
// Thread = one row x one VEC-wide channel chunk, chunk index fastest (two rows per thread, or several 256-thread slices per
// workgroup, only lengthen the chain of dependent loads rowptr -> col/nrm -> x rows that a thread walks -- measured
// 11.1 vs 10.8 us and 13.3 vs 11.0 us at N = 1.2e5, C = 20: the rows-per-thread parameter is gone).  Measured with PMC
// counters at the same shape: FETCH_SIZE equals the algorithmic reads once workgroups are mapped XCD-wise (below), waves
// spend ~60 % of their cycles waiting on memory and the launch moves ~3 TB/s against the 7 TB/s a plain copy of
// the same buffers reaches.
// One launch serves one or two column parts of the same rows (x, p, q, out of width C each): Z = [X | H] of the
// recurrent cells is propagated as its two matrices, never concatenated.  Part b's workgroups follow part a's.
struct SpmmPart {
    const float* x;
    const float* p;
    const float* q;
    float* out;
    int C, ldx, ldp, ldq, xcd_chunk;      // row strides of x / p / q in floats (out rows are dense)
};
static constexpr int QT_SPMM_BS = 64;      // one wave per workgroup: 11.08 ms per training step against 11.12 (128) and 11.18 (256)
template <int VEC, int EPT>
__global__ __launch_bounds__(QT_SPMM_BS) void k_spmm(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const float* __restrict__ nrm, const int4* __restrict__ ell, int Ncap,
                                              const int32_t* __restrict__ n_dev,
                                              SpmmPart pa, SpmmPart pb, int nblk_a,     // workgroups [nblk_a, ..) do part b
                                              float alpha, float beta, float gamma) {
    using V = fvec<VEC>;
    const bool second = (int)blockIdx.x >= nblk_a;
    const SpmmPart& P = second ? pb : pa;
    const int C = P.C, ldx = P.ldx, xcd_chunk = P.xcd_chunk;
    const float* __restrict__ x = P.x;
    const float* p = P.p;
    const float* q = P.q;
    float* out = P.out;                     // out may alias p or q (in-place Clenshaw step)
    const int bid = second ? (int)blockIdx.x - nblk_a : (int)blockIdx.x;
    const int nch = C / VEC;
    // Workgroups are dealt round-robin to the 8 XCDs, each with a private L2.  Giving XCD x the contiguous node range
    // [x * chunk, (x+1) * chunk) keeps a node's neighbours (close in the reversed-Morton order) in the L2 that reads them.
    // The chunk is an eighth of the VALID rows (read on the device in static mode), not of the capacity the grid was
    // sized for: otherwise the last XCDs idle whenever a mesh has fewer nodes than pixels.
    const int rows = qt_rows(n_dev, Ncap);
    int blk = bid;
    if (xcd_chunk) {
        const int nblk = (int)(((int64_t)rows * nch + QT_SPMM_BS - 1) / QT_SPMM_BS);
        const int chunk = (nblk + 7) >> 3;
        if ((bid >> 3) >= chunk) return;
        blk = (bid & 7) * chunk + (bid >> 3);
    }
    const unsigned idx = (unsigned)blk * (unsigned)QT_SPMM_BS + threadIdx.x;      // N * nch < 2^31 (checked by the host entry): 32-bit
    const int64_t row = idx / (unsigned)nch;                       // division, a fraction of the 64-bit one's cost
    if (row >= rows) return;
    const int ch = (int)(idx - (unsigned)row * (unsigned)nch) * VEC;
    const bool head = VEC == 4 && ell;
    int e0 = head ? 0 : rowptr[row], e1 = head ? 0 : rowptr[row + 1];
    V acc = vzero<VEC>();
    // the addends are requested now, together with the index loads, not after the gather loop: one dependent memory phase
    // less at the end of every launch (each thread reads its own p / q element before it writes out: aliasing is fine)
    V pv = vzero<VEC>(), qv = vzero<VEC>();
    if (p) pv = vload<VEC>(p + row * P.ldp + ch);
    if (q) qv = vload<VEC>(q + row * P.ldq + ch);
    if constexpr (VEC == 4) {
        if (ell) {
            // the first four edges of a row come as two 16-byte vectors (qt_edges_norm): no row pointer on the way to the
            // gathers, fully regular index loads; only rows flagged with more than four edges go on to the CSR loop below
            const EllHead h = ell_head(ell, row);
            const V f[4] = {vload<4>(x + (int64_t)h.c.x * ldx + ch), vload<4>(x + (int64_t)h.c.y * ldx + ch),
                            vload<4>(x + (int64_t)h.c.z * ldx + ch), vload<4>(x + (int64_t)h.c.w * ldx + ch)};
            fma4<4>(acc, h.w, f);
            if (h.more) {
                e0 = rowptr[row] + 4;
                e1 = rowptr[row + 1];
            }
        }
    }
    // EPT edges per trip: the index/weight loads, then the neighbour gathers, are independent and stay in flight together
    // (quadtree rows have ~4 neighbours, so most rows finish in the first trip).
    // Tried and rejected (round 1): staging each 64-row run of the reversed-Morton node order in LDS so that the ~87 %
    // internal neighbours are LDS reads -- 12.2 us vs 11.2 us per launch at N = 1.2e5, C = 20.
    auto trip = [&](int eb) -> bool {
        int cj[EPT];
        float w[EPT];
#pragma unroll
        for (int v = 0; v < EPT; ++v) {
            const bool ok = eb + v < e1;
            cj[v] = ok ? col[eb + v] : (int)row;
            w[v] = ok ? nrm[eb + v] : 0.0f;
        }
        if constexpr (VEC == 4) {
            // gathers in groups of 4 edges: the first group always (slots beyond the row's edges re-read the row itself with
            // weight 0), a further group only for the lanes whose row reaches it -- one branch per group, so a row with 4
            // neighbours costs the texture addresser 4 gathers, not EPT, while the index loads of all EPT slots (issued
            // above) stay off the critical path of the rows with many neighbours
#pragma unroll
            for (int v0 = 0; v0 < EPT; v0 += 4) {
                if (v0 > 0 && eb + v0 >= e1) continue;
                V f[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) f[v] = vload<4>(x + (int64_t)cj[v0 + v] * ldx + ch);
                fma4<4>(acc, w + v0, f);
            }
        } else {
            // (scalar rows: the compiler has always emitted these sums as separate multiplies and adds, so the intrinsic chain
            // of fma4 would change their bits; contraction is switched off to keep them so: profiles/aggr_shared.txt)
#pragma clang fp contract(off)
            float f[EPT];
#pragma unroll
            for (int v = 0; v < EPT; ++v) f[v] = x[(int64_t)cj[v] * ldx + ch];
#pragma unroll
            for (int v = 0; v < EPT; ++v) acc[0] += w[v] * f[v];
        }
        return eb + EPT < e1;
    };
    int eb = e0;
    bool any = e0 < e1;
    while (any) {
        any = trip(eb);
        eb = any ? eb + EPT : e1;       // a finished row keeps an empty edge range
    }
    // The finish, spelled out as the compiler had always contracted  r = alpha acc; r += beta p; r += gamma q  (read from the
    // listing; the intrinsic form fma(beta, p, rn(alpha acc)) in every channel would change bits): scalar rows add the
    // separately rounded products alpha acc and beta p; a 4-channel chunk has fma(beta, p, rn(alpha acc)) in channels 0, 2, 3
    // and fma(alpha, acc, rn(beta p)) in channel 1; gamma q is fused everywhere.  (profiles/aggr_shared.txt)
    V r;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float aa = alpha * acc[k];
            r[k] = aa;
            if (p) {
                const float bp = beta * pv[k];
                r[k] = VEC == 1 ? aa + bp : k == 1 ? __builtin_fmaf(alpha, acc[k], bp) : __builtin_fmaf(beta, pv[k], aa);
            }
            if (q) r[k] = __builtin_fmaf(gamma, qv[k], r[k]);
        }
    }
    vstore<VEC>(out + row * C + ch, r);
}

// One-column message aggregate with strided operands and an optional output epilogue: the Clenshaw recurrence of a
// ChebConv with ONE output channel (the decoder's fc_out2, model/seq2seq.py:121) after its coefficient columns have been
// applied -- u = z [w_0 w_1 w_2] first, then y = u_0 + L^ (u_1 + 2 L^ u_2) - u_2 on single columns of the (N, 4) matrix u:
// the two propagations move 4 bytes per row and neighbour instead of the 64-byte rows of z.  Thread = row.
struct Spmm1Args {
    const int32_t* rowptr;
    const int32_t* col;
    const float* nrm;
    const int4* ell;
    int Ncap;
    const int32_t* n_dev;
    const float *x, *p, *q;
    int ldx, ldp, ldq;
    float alpha, beta, gamma;
    float* out;
    int ldo, pad4;          // pad4: the row is written as (v, 0, 0, 0)
    int act;                // QT_ACT_NONE or QT_ACT_TANH_RES: v = tanh(drop * v) + res
    const float* res;
    int ldr;
    const float* drop;
};
__global__ __launch_bounds__(64) void k_spmm1(Spmm1Args a) {
    const int rows = qt_rows(a.n_dev, a.Ncap);
    const int nblk = (rows + 63) >> 6, chunk = (nblk + 7) >> 3;           // XCD-wise row ranges, as k_spmm
    const int bid = blockIdx.x;
    if ((bid >> 3) >= chunk) return;
    const int64_t row = (int64_t)((bid & 7) * chunk + (bid >> 3)) * 64 + threadIdx.x;
    if (row >= rows) return;
    const float pv = a.p ? a.p[row * a.ldp] : 0.0f, qv = a.q ? a.q[row * a.ldq] : 0.0f;
    const float* __restrict__ x = a.x;
    // (the sums below mirror fma4 but are separate multiplies and adds, as the compiler has always emitted them: the
    // intrinsic would change this kernel's bits, so contraction is switched off where they stand: profiles/aggr_shared.txt)
    float acc = 0.0f;
    int e0, e1;
    if (a.ell) {
#pragma clang fp contract(off)
        const EllHead h = ell_head(a.ell, row);
        const float f0 = x[(int64_t)h.c.x * a.ldx], f1 = x[(int64_t)h.c.y * a.ldx], f2 = x[(int64_t)h.c.z * a.ldx],
                    f3 = x[(int64_t)h.c.w * a.ldx];
        acc += h.w[0] * f0;
        acc += h.w[1] * f1;
        acc += h.w[2] * f2;
        acc += h.w[3] * f3;
        e0 = e1 = 0;
        if (h.more) {
            e0 = a.rowptr[row] + 4;
            e1 = a.rowptr[row + 1];
        }
    } else {
        e0 = a.rowptr[row];
        e1 = a.rowptr[row + 1];
    }
    for (int eb = e0; eb < e1; eb += 4) {
#pragma clang fp contract(off)
        int cj[4];
        float w[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const bool ok = eb + v < e1;
            cj[v] = ok ? a.col[eb + v] : (int)row;
            w[v] = ok ? a.nrm[eb + v] : 0.0f;
        }
        float f[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) f[v] = x[(int64_t)cj[v] * a.ldx];
#pragma unroll
        for (int v = 0; v < 4; ++v) acc += w[v] * f[v];
    }
    float v = a.alpha * acc;       // (the finish as k_spmm's scalar rows have it: + beta p unfused, gamma q fused)
    {
#pragma clang fp contract(off)
        if (a.p) v = v + a.beta * pv;
    }
    if (a.q) v = __builtin_fmaf(a.gamma, qv, v);
    if (a.act == QT_ACT_TANH_RES) v = act_quad(v, QT_ACT_TANH_RES, a.drop ? a.drop[row] : 1.0f, a.res[row * a.ldr]);
    if (a.pad4)
        *reinterpret_cast<float4*>(a.out + row * a.ldo) = make_float4(v, 0.0f, 0.0f, 0.0f);
    else
        a.out[row * a.ldo] = v;
}

}  // namespace

static int spmm_part(SpmmPart* P, int* nblk, int N, int C, const float* x, int ldx, const float* p, int ldp, const float* q,
                     int ldq, float* out) {
    P->x = x; P->p = p; P->q = q; P->out = out; P->C = C;
    P->ldx = ldx > 0 ? ldx : C; P->ldp = ldp > 0 ? ldp : C; P->ldq = ldq > 0 ? ldq : C;
    int grid = qt_cdiv((int64_t)N * (C / 4), QT_SPMM_BS);
    P->xcd_chunk = 0;
    if (grid >= 64) {
        P->xcd_chunk = qt_cdiv(grid, 8);
        grid = P->xcd_chunk * 8;    // surplus workgroups fall past the row count and exit
    }
    *nblk = grid;
    return 0;
}

// 8 edges per trip for rows of up to this many channels (see qt_spmm: wider rows are bandwidth bound and prefer fewer registers)
static constexpr int QT_EPT8_MAXC = 20;

extern "C" int qt_spmm2(const int32_t* rowptr, const int32_t* col, const float* nrm, int N, const int32_t* n_dev, int Ca,
                        const float* xa, int ldxa, const float* pa, int ldpa, const float* qa, int ldqa, float* outa, int Cb,
                        const float* xb, int ldxb, const float* pb, int ldpb, const float* qb, int ldqb, float* outb,
                        float alpha, float beta, float gamma, const int32_t* ell, void* stream) {
    QT_ARG((ldxa | ldpa | ldqa | ldxb | ldpb | ldqb) % 4 == 0, "row strides must be multiples of 4");
    QT_ARG(rowptr && col && nrm && xa && outa && Ca > 0 && Ca % 4 == 0 && Cb >= 0 && Cb % 4 == 0, "bad arguments");
    QT_ARG(Cb == 0 || (xb && outb && (pb != nullptr) == (pa != nullptr) && (qb != nullptr) == (qa != nullptr)),
           "part b must mirror part a");
    QT_ARG(xa != outa && (Cb == 0 || xb != outb), "out must not alias x");
    QT_ARG((int64_t)N * max(Ca, Cb) / 4 + 2048 < (int64_t)1 << 31, "N * C too large for 32-bit thread indices");
    QT_ARG((((uintptr_t)xa | (uintptr_t)outa | (uintptr_t)pa | (uintptr_t)qa | (uintptr_t)xb | (uintptr_t)outb | (uintptr_t)pb |
             (uintptr_t)qb | (uintptr_t)ell) & 15) == 0, "operands must be 16-byte aligned");
    if (N <= 0) return QT_OK;
    SpmmPart A, B = {};
    int na = 0, nb = 0;
    spmm_part(&A, &na, N, Ca, xa, ldxa, pa, ldpa, qa, ldqa, outa);
    if (Cb) spmm_part(&B, &nb, N, Cb, xb, ldxb, pb, ldpb, qb, ldqb, outb);
    // the wider part decides
    if (max(Ca, Cb) <= QT_EPT8_MAXC)
        hipLaunchKernelGGL((k_spmm<4, 8>), dim3(na + nb), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, reinterpret_cast<const int4*>(ell), N, n_dev, A, B, na, alpha, beta, gamma);
    else
        hipLaunchKernelGGL((k_spmm<4, 4>), dim3(na + nb), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, reinterpret_cast<const int4*>(ell), N, n_dev, A, B, na, alpha, beta, gamma);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_spmm1(const int32_t* rowptr, const int32_t* col, const float* nrm, const int32_t* ell, int N, const int32_t* n_dev,
                        const float* x, int ldx, float alpha, const float* p, int ldp, float beta, const float* q, int ldq,
                        float gamma, float* out, int ldo, int pad4, int act, const float* res, int ldr, const float* drop,
                        void* stream) {
    QT_ARG(rowptr && col && nrm && x && out && ldx >= 1 && ldo >= 1 && (!p || ldp >= 1) && (!q || ldq >= 1), "bad arguments");
    QT_ARG(act == QT_ACT_NONE || (act == QT_ACT_TANH_RES && res && ldr >= 1), "the epilogue is none or tanh(drop v) + res");
    QT_ARG(!pad4 || (ldo % 4 == 0 && ((uintptr_t)out & 15) == 0), "pad4 writes 16-byte rows");
    QT_ARG(((uintptr_t)ell & 15) == 0, "ell must be 16-byte aligned");
    if (N <= 0) return QT_OK;
    Spmm1Args a = {rowptr, col, nrm, reinterpret_cast<const int4*>(ell), N, n_dev, x, p, q, ldx, ldp, ldq, alpha, beta, gamma,
                   out, ldo, pad4, act, res, ldr, drop};
    const int grid = qt_cdiv(qt_cdiv(N, 64), 8) * 8;
    hipLaunchKernelGGL(k_spmm1, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_spmm(const int32_t* rowptr, const int32_t* col, const float* nrm, int N, const int32_t* n_dev, int C,
                       const float* x, float alpha, const float* p, float beta, const float* q, float gamma, float* out,
                       void* stream) {
    QT_ARG(rowptr && col && nrm && x && out && C > 0, "bad arguments");
    QT_ARG(x != out, "out must not alias x");
    if (N <= 0) return QT_OK;
    const bool v4 = (C % 4 == 0) && ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)p | (uintptr_t)q) % 16) == 0);
    if (v4) return qt_spmm2(rowptr, col, nrm, N, n_dev, C, x, 0, p, 0, q, 0, out, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, alpha, beta, gamma, nullptr, stream);
    // scalar rows (C not a multiple of 4): one float per thread
    SpmmPart A, B = {};
    A.x = x; A.p = p; A.q = q; A.out = out; A.C = C; A.ldx = A.ldp = A.ldq = C; A.xcd_chunk = 0;
    const int grid = qt_cdiv((int64_t)N * C, QT_SPMM_BS);
    // Edges per trip: a trip is two dependent loads (col/nrm, then the x rows), and the few rows with many neighbours
    // (a 4x4 cell next to 1x1 cells has 16) set the length of the whole launch.  8 per trip: 6.6 -> 4.5 us at C = 4,
    // 9.3 -> 7.5 us at C = 16 (N = 1.2e5, inside a hipGraph); wider rows are bandwidth bound and prefer fewer registers.
    hipLaunchKernelGGL((k_spmm<1, 8>), dim3(grid), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, (const int4*)nullptr, N, n_dev, A, B, grid, alpha, beta, gamma);
    QT_LAUNCHED();
    return QT_OK;
}
