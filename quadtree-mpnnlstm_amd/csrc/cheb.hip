// Chebyshev message aggregate (PyG ChebConv as used by model/model.py:53,96):
//   k_spmm  -- the CSR message-aggregate  out = alpha * L^ x + beta * p + gamma * q
//   k_spmm1 -- the same on single strided columns, with an optional output epilogue
// The dense products that turn the aggregated planes into outputs are in gemm.hip, the gate-cell launches in gatecell.hip.
#include "qt_gemm.h"      // (act_quad: the epilogue activation, shared with the dense kernels)

namespace {

// ------------------------------------------------------------------ message aggregate
// Thread = (RPT consecutive rows) x (one VEC-wide channel chunk), chunk index fastest (RPT = 1 in every launch: two rows
// per thread, or several 256-thread slices per workgroup, only lengthen the chain of dependent loads rowptr -> col/nrm ->
// x rows that a thread walks -- measured 11.1 vs 10.8 us and 13.3 vs 11.0 us at N = 1.2e5, C = 20).  Measured with PMC
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
template <int VEC, int RPT, int EPT>
__global__ __launch_bounds__(QT_SPMM_BS) void k_spmm(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const float* __restrict__ nrm, const int4* __restrict__ ell, int Ncap,
                                              const int32_t* __restrict__ n_dev,
                                              SpmmPart pa, SpmmPart pb, int nblk_a,     // workgroups [nblk_a, ..) do part b
                                              float alpha, float beta, float gamma) {
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
        const int nblk = (int)(((int64_t)((rows + RPT - 1) / RPT) * nch + QT_SPMM_BS - 1) / QT_SPMM_BS);
        const int chunk = (nblk + 7) >> 3;
        if ((bid >> 3) >= chunk) return;
        blk = (bid & 7) * chunk + (bid >> 3);
    }
    const unsigned idx = (unsigned)blk * (unsigned)QT_SPMM_BS + threadIdx.x;      // N * nch < 2^31 (checked by the host entry): 32-bit
    const int64_t rp = idx / (unsigned)nch;                        // division, a fraction of the 64-bit one's cost
    if (rp * RPT >= rows) return;
    const int ch = (int)(idx - (unsigned)rp * (unsigned)nch) * VEC;
    int e0[RPT], e1[RPT];
    int64_t row[RPT];
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        row[u] = rp * RPT + u;
        const bool ok = row[u] < rows;
        if (!ok) row[u] = rows - 1;                // duplicate of a valid row; its result is not stored
        e0[u] = (ok && !(VEC == 4 && ell)) ? rowptr[row[u]] : 0;
        e1[u] = (ok && !(VEC == 4 && ell)) ? rowptr[row[u] + 1] : 0;
    }
    float acc[RPT][VEC];
#pragma unroll
    for (int u = 0; u < RPT; ++u)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[u][k] = 0.0f;
    // the addends are requested now, together with the index loads, not after the gather loop: one dependent memory phase
    // less at the end of every launch (each thread reads its own p / q element before it writes out: aliasing is fine)
    float pv[RPT][VEC], qv[RPT][VEC];
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        if constexpr (VEC == 4) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (p) a = *reinterpret_cast<const float4*>(p + row[u] * P.ldp + ch);
            if (q) b = *reinterpret_cast<const float4*>(q + row[u] * P.ldq + ch);
            pv[u][0] = a.x; pv[u][1] = a.y; pv[u][2] = a.z; pv[u][3] = a.w;
            qv[u][0] = b.x; qv[u][1] = b.y; qv[u][2] = b.z; qv[u][3] = b.w;
        } else {
            pv[u][0] = p ? p[row[u] * P.ldp + ch] : 0.0f;
            qv[u][0] = q ? q[row[u] * P.ldq + ch] : 0.0f;
        }
    }
    if constexpr (VEC == 4) {
        if (ell) {
            // the first four edges of a row come as two 16-byte vectors (qt_edges_norm): no row pointer on the way to the
            // gathers, fully regular index loads; only rows flagged with more than four edges go on to the CSR loop below
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                int4 c4 = ell[2 * row[u]];
                const int4 wb = ell[2 * row[u] + 1];
                const bool more4 = c4.w < 0;
                if (more4) c4.w = ~c4.w;
                const float4 f0 = *reinterpret_cast<const float4*>(x + (int64_t)c4.x * ldx + ch);
                const float4 f1 = *reinterpret_cast<const float4*>(x + (int64_t)c4.y * ldx + ch);
                const float4 f2 = *reinterpret_cast<const float4*>(x + (int64_t)c4.z * ldx + ch);
                const float4 f3 = *reinterpret_cast<const float4*>(x + (int64_t)c4.w * ldx + ch);
                const float w0 = __int_as_float(wb.x), w1 = __int_as_float(wb.y), w2 = __int_as_float(wb.z), w3 = __int_as_float(wb.w);
                acc[u][0] += w0 * f0.x; acc[u][1] += w0 * f0.y; acc[u][2] += w0 * f0.z; acc[u][3] += w0 * f0.w;
                acc[u][0] += w1 * f1.x; acc[u][1] += w1 * f1.y; acc[u][2] += w1 * f1.z; acc[u][3] += w1 * f1.w;
                acc[u][0] += w2 * f2.x; acc[u][1] += w2 * f2.y; acc[u][2] += w2 * f2.z; acc[u][3] += w2 * f2.w;
                acc[u][0] += w3 * f3.x; acc[u][1] += w3 * f3.y; acc[u][2] += w3 * f3.z; acc[u][3] += w3 * f3.w;
                if (more4 && rp * RPT + u < rows) {
                    e0[u] = rowptr[row[u]] + 4;
                    e1[u] = rowptr[row[u] + 1];
                }
            }
        }
    }
    // 4 edges per trip: the index/weight loads, then the neighbour gathers, are independent and stay in flight together
    // (quadtree rows have ~4 neighbours, so most rows finish in the first trip, which is issued for all RPT rows at once).
    // Tried and rejected (round 1): staging each 64-row run of the reversed-Morton node order in LDS so that the ~87 %
    // internal neighbours are LDS reads -- 12.2 us vs 11.2 us per launch at N = 1.2e5, C = 20.
    auto trip = [&](const int (&eb)[RPT], bool (&more)[RPT]) {
        int cj[RPT][EPT];
        float w[RPT][EPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u)
#pragma unroll
            for (int v = 0; v < EPT; ++v) {
                const bool ok = eb[u] + v < e1[u];
                cj[u][v] = ok ? col[eb[u] + v] : (int)row[u];
                w[u][v] = ok ? nrm[eb[u] + v] : 0.0f;
            }
        if constexpr (VEC == 4) {
            // gathers in groups of 4 edges: the first group always (slots beyond the row's edges re-read the row itself with
            // weight 0), a further group only for the lanes whose row reaches it -- one branch per group, so a row with 4
            // neighbours costs the texture addresser 4 gathers, not EPT, while the index loads of all EPT slots (issued
            // above) stay off the critical path of the rows with many neighbours
#pragma unroll
            for (int v0 = 0; v0 < EPT; v0 += 4) {
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    if (v0 > 0 && eb[u] + v0 >= e1[u]) continue;
                    float4 f[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) f[v] = *reinterpret_cast<const float4*>(x + (int64_t)cj[u][v0 + v] * ldx + ch);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        acc[u][0] += w[u][v0 + v] * f[v].x; acc[u][1] += w[u][v0 + v] * f[v].y;
                        acc[u][2] += w[u][v0 + v] * f[v].z; acc[u][3] += w[u][v0 + v] * f[v].w;
                    }
                }
            }
        } else {
            float f[RPT][EPT];
#pragma unroll
            for (int u = 0; u < RPT; ++u)
#pragma unroll
                for (int v = 0; v < EPT; ++v) f[u][v] = x[(int64_t)cj[u][v] * ldx + ch];
#pragma unroll
            for (int u = 0; u < RPT; ++u)
#pragma unroll
                for (int v = 0; v < EPT; ++v) acc[u][0] += w[u][v] * f[u][v];
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) more[u] = eb[u] + EPT < e1[u];
    };
    int eb[RPT];
    bool more[RPT];
    bool any = false;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        eb[u] = e0[u];
        any |= e0[u] < e1[u];
    }
    while (any) {
        trip(eb, more);
        any = false;
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            eb[u] = more[u] ? eb[u] + EPT : e1[u];       // a finished row keeps an empty edge range
            any |= more[u];
        }
    }
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        if (rp * RPT + u >= rows) continue;
        const int64_t o = row[u] * C + ch;
        float r[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            r[k] = alpha * acc[u][k];
            if (p) r[k] += beta * pv[u][k];
            if (q) r[k] += gamma * qv[u][k];
        }
        if constexpr (VEC == 4) {
            *reinterpret_cast<float4*>(out + o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            out[o] = r[0];
        }
    }
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
    float acc = 0.0f;
    int e0, e1;
    if (a.ell) {
        int4 c4 = a.ell[2 * row];
        const int4 wb = a.ell[2 * row + 1];
        const bool more4 = c4.w < 0;
        if (more4) c4.w = ~c4.w;
        const float f0 = x[(int64_t)c4.x * a.ldx], f1 = x[(int64_t)c4.y * a.ldx], f2 = x[(int64_t)c4.z * a.ldx],
                    f3 = x[(int64_t)c4.w * a.ldx];
        acc += __int_as_float(wb.x) * f0;
        acc += __int_as_float(wb.y) * f1;
        acc += __int_as_float(wb.z) * f2;
        acc += __int_as_float(wb.w) * f3;
        e0 = e1 = 0;
        if (more4) {
            e0 = a.rowptr[row] + 4;
            e1 = a.rowptr[row + 1];
        }
    } else {
        e0 = a.rowptr[row];
        e1 = a.rowptr[row + 1];
    }
    for (int eb = e0; eb < e1; eb += 4) {
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
    float v = a.alpha * acc;
    if (a.p) v += a.beta * pv;
    if (a.q) v += a.gamma * qv;
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
        hipLaunchKernelGGL((k_spmm<4, 1, 8>), dim3(na + nb), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, reinterpret_cast<const int4*>(ell), N, n_dev, A, B, na, alpha, beta, gamma);
    else
        hipLaunchKernelGGL((k_spmm<4, 1, 4>), dim3(na + nb), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, reinterpret_cast<const int4*>(ell), N, n_dev, A, B, na, alpha, beta, gamma);
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
    hipLaunchKernelGGL((k_spmm<1, 1, 8>), dim3(grid), dim3(QT_SPMM_BS), 0, (hipStream_t)stream, rowptr, col, nrm, (const int4*)nullptr, N, n_dev, A, B, grid, alpha, beta, gamma);
    QT_LAUNCHED();
    return QT_OK;
}
